"""An independent numpy restatement of the mono_fisheye driver's input path, written from the reference lines
(Examples/Monocular/mono_fisheye.cc:94-116 applyMask / crop / resize, :202-212 applyMask, :244-271 ConvertMaskBirdview;
Tracking.cc:278-307 cvtColor), not from csrc/prep_def.h.  Whole-array int64 arithmetic; no loops over pixels."""
import numpy as np

GRAY = -1                       # a one-channel frame
RGB, BGR, RGBA, BGRA = 0, 1, 2, 3


def channels(code):
    return {GRAY: 1, RGB: 3, BGR: 3, RGBA: 4, BGRA: 4}[code]


def mask_plane(mask):
    """The byte applyMask compares: mask.at<Vec3b>(i, j)[1] of a 3-channel mask, the only channel of a 1-channel one."""
    m = np.asarray(mask)
    return m if m.ndim == 2 else m[:, :, 1]


def cvt_gray(c3, code):
    """OpenCV 3.2 RGB2Gray<uchar>: (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14 on (..., >= 3) integer channels."""
    c3 = c3.astype(np.int64)
    r, b = (c3[..., 2], c3[..., 0]) if code in (BGR, BGRA) else (c3[..., 0], c3[..., 2])
    return (r * 4899 + c3[..., 1] * 9617 + b * 1868 + 8192) >> 14


def half(img):
    """cv::resize(..., 0.5, 0.5) at an exact factor of 2 (the INTER_AREA fast path): (a + b + c + d + 2) >> 2 per channel."""
    a = img.astype(np.int64)
    return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2


def front_prep(image, mask, crop, code=GRAY):
    """applyMask over the whole frame, crop Rect(cx, cy, cw, ch), half-size resize, cvtColor, in the driver's order."""
    img = np.asarray(image).copy()
    if img.ndim == 2:
        img = img[:, :, None]
    if mask is not None:
        img[mask_plane(mask) > 250] = 0
    cx, cy, cw, ch = crop
    small = half(img[cy:cy + ch, cx:cx + cw])
    out = small[:, :, 0] if code == GRAY else cvt_gray(small, code)
    return np.ascontiguousarray(out.astype(np.uint8))


def gray_then_half(image, crop, code):
    """The other order (convert, then resize): what the product must NOT compute."""
    cx, cy, cw, ch = crop
    return half(cvt_gray(np.asarray(image)[cy:cy + ch, cx:cx + cw], code)).astype(np.uint8)


def footprint_rect(w, h):
    """Frame.cc:320-327 as C++ evaluates it: int / 2 first, the doubles truncated toward zero by cv::Rect, the
    rectangle clipped to the image.  Returns (x0, y0, x1, y1)."""
    p2m, length, wid, boundary = 0.03984 * 1.7, 4.63, 1.901, 15.0
    x = w // 2 - (wid / 2 / p2m) - boundary
    y = h // 2 - (length / 2 / p2m) - boundary
    rw, rh = int(wid / p2m + 2 * boundary), int(length / p2m + 2 * boundary)
    rx, ry = int(x), int(y)
    return max(rx, 0), max(ry, 0), min(rx + rw, w), min(ry + rh, h)


def bird_mask(mask_image):
    """ConvertMaskBirdview: 0 where G < 20, else 250, then the vehicle footprint zeroed."""
    m = np.asarray(mask_image)
    out = np.where(m[:, :, 1] < 20, 0, 250).astype(np.uint8)
    x0, y0, x1, y1 = footprint_rect(m.shape[1], m.shape[0])
    out[y0:y1, x0:x1] = 0
    return out
