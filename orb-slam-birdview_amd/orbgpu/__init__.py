"""orbgpu — MI355X-native ORB front-end (Python mirror of the reference C++ interface).

ORBextractor / ORBmatcher keep the names, argument meaning and return conventions of
donglinb/ORB-SLAM-BIRDVIEW include/ORBextractor.h:45-111 and include/ORBmatcher.h:37-119, with
OpenCV containers replaced by numpy: keypoints are a structured array with cv::KeyPoint's 28-byte
layout (KP_DTYPE), descriptors an (n, 32) uint8 array, FeatureVectors a dict {node_id: [indices]}.
Every call runs on the GPU through liborbgpu.so (include/orbgpu.h); there is no CPU fallback.
"""
import ctypes

import numpy as np

from ._lib import (VARIANT_BLUR_HALFUP, VARIANT_DEFAULT, VARIANT_NO_FMA, VARIANT_RESIZE_GENERIC,
                   VARIANT_TIE_REVERSE, OrbBirdParams, OrbError, OrbFeatVec, OrbFrameGrid, OrbParams, OrbProjFrameTarget,
                   OrbProjTarget, OrbCamera, OrbDepthMap, OrbDistortion, OrbFusePointsTarget, KfdbNeighboursFn, check, lib)

__all__ = ["ORBextractor", "ORBmatcher", "BatchExtractor", "KP_DTYPE", "OrbError", "device_count",
           "features_in_area", "frame_grid", "Frame", "PROJ_QUERY_DTYPE", "PROJ_BEST", "PROJ_RATIO_SAME_LEVEL",
           "PROJ_GATE_NONE", "PROJ_GATE_FUSE", "proj_queries", "project_best_host",
           "COLOR_RGB", "COLOR_BGR", "COLOR_RGBA", "COLOR_BGRA", "DEPTH_U16", "DEPTH_F32", "to_gray_host", "depth_map",
           "stereo_from_rgbd_host", "remap_host", "rectify_maps_host", "remap_device", "Rectifier", "PREP_GRAY", "front_prep_host", "bird_mask_host", "front_prep_device",
           "bird_mask_device", "FrontPrep", "distortion", "undistort_points_host", "image_bounds", "undistort_keypoints", "undistort_guard",
           "MapPoints", "POINT_PROJ_DTYPE", "FRUSTUM_FRAME", "FRUSTUM_FUSE", "camera", "project_points_host",
           "compute_stereo_matches", "ORBVocabulary", "KeyFrameDatabase", "bow_score", "KFDB_RELOC", "KFDB_LOOP",
           "BirdORB", "cornerSubPix",
           "bird_footprint_mask", "VARIANT_DEFAULT", "VARIANT_TIE_REVERSE", "VARIANT_RESIZE_GENERIC",
           "VARIANT_BLUR_HALFUP", "VARIANT_NO_FMA"]

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30   # ORBmatcher.cc:37-39

# orb_proj_query (include/orbgpu.h): one projected map point of the projection-gated searches
PROJ_QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("r", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                             ("ur", "<f4"), ("ur_tol", "<f4"), ("angle", "<f4"), ("blocks", "<i4")])
assert PROJ_QUERY_DTYPE.itemsize == 36
PROJ_BEST, PROJ_RATIO_SAME_LEVEL = 0, 1   # ORB_PROJ_*
PROJ_GATE_NONE, PROJ_GATE_FUSE = 0, 1     # ORB_PROJ_GATE_*

# orb_point_proj (include/orbgpu.h): the projection of one resident map point
POINT_PROJ_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("invz", "<f4"), ("dist", "<f4"),
                             ("view_cos", "<f4"), ("r", "<f4"), ("level", "<i4"), ("verdict", "<i4")])
assert POINT_PROJ_DTYPE.itemsize == 36
FRUSTUM_FRAME, FRUSTUM_FUSE = 0, 1        # ORB_FRUSTUM_*


COLOR_RGB, COLOR_BGR, COLOR_RGBA, COLOR_BGRA = 0, 1, 2, 3   # ORB_COLOR_*
DEPTH_U16, DEPTH_F32 = 0, 1                                  # ORB_DEPTH_*
PREP_GRAY = -1                                               # ORB_PREP_GRAY: a one-channel fisheye frame


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _color_image(image, color):
    """An H x W x 3 / 4 uint8 array with unit-stride pixels, as the colour entry points take it (rows may be padded)."""
    img = np.asarray(image)
    ch = 3 if color in (COLOR_RGB, COLOR_BGR) else 4
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == ch, "H x W x %d uint8 expected" % ch
    if not (img.strides[2] == 1 and img.strides[1] == ch and img.strides[0] >= img.shape[1] * ch):
        img = np.ascontiguousarray(img)
    return img


def to_gray_host(image, color):
    """orb_to_gray_host: cvtColor(image, gray, CV_{RGB,BGR,RGBA,BGRA}2GRAY) as OpenCV 3.2 computes it, on the CPU (the
    definition the GPU forms equal byte for byte).  image: H x W x 3 / 4 uint8; color: COLOR_*; no context, no GPU."""
    img = _color_image(image, color)
    h, w = img.shape[:2]
    out = np.zeros((h, w), np.uint8)
    check(lib().orb_to_gray_host(color, _p(img), w, h, img.strides[0], _p(out), w), "orb_to_gray_host")
    return out


def depth_map(data, type, w, h, row_stride=None, frame_pitch=None, factor=1.0):
    """orb_depth_map: data is a device pointer (int) or a host numpy array (kept alive by the caller); type DEPTH_U16 /
    DEPTH_F32; row_stride / frame_pitch in bytes (default: packed); factor = mDepthMapFactor (already inverted)."""
    es = 2 if type == DEPTH_U16 else 4
    rs = w * es if row_stride is None else row_stride
    ptr = data.ctypes.data if isinstance(data, np.ndarray) else data
    return OrbDepthMap(ctypes.c_void_p(ptr), type, w, h, rs, rs * h if frame_pitch is None else frame_pitch,
                       float(np.float32(factor)))


def stereo_from_rgbd_host(depth_image, factor, kps, kps_un, mbf):
    """orb_stereo_from_rgbd_host: Frame::ComputeStereoFromRGBD (with GrabImageRGBD's convertTo folded in) on the CPU, the
    definition, and the right call for one frame whose keypoints are on the host.  depth_image: H x W uint16 or float32
    (the RAW depth image; rows may be padded); kps: mvKeys (the pixel read), kps_un: mvKeysUn (the x of mvuRight).
    Returns (mvuRight, mvDepth, number of keypoints with a depth).  No context, no GPU."""
    d = np.asarray(depth_image)
    assert d.ndim == 2 and d.dtype in (np.uint16, np.float32), "H x W uint16 or float32 expected"
    if d.strides[1] != d.itemsize or d.strides[0] < d.shape[1] * d.itemsize:
        d = np.ascontiguousarray(d)
    k = np.ascontiguousarray(kps, KP_DTYPE)
    ku = np.ascontiguousarray(kps_un, KP_DTYPE)
    assert len(k) == len(ku)
    m = depth_map(d, DEPTH_U16 if d.dtype == np.uint16 else DEPTH_F32, d.shape[1], d.shape[0], d.strides[0],
                  factor=factor)
    ur = np.zeros(len(k), np.float32)
    dep = np.zeros(len(k), np.float32)
    nv = ctypes.c_int(0)
    check(lib().orb_stereo_from_rgbd_host(ctypes.byref(m), float(np.float32(mbf)), len(k), _p(k), _p(ku), _p(ur), _p(dep),
                                          ctypes.byref(nv)), "orb_stereo_from_rgbd_host")
    return ur, dep, nv.value


def _gray_image(image):
    """An H x W uint8 array with unit-stride pixels (rows may be padded), as the gray entry points take it."""
    img = np.asarray(image)
    assert img.dtype == np.uint8 and img.ndim == 2, "CV_8UC1 expected"
    if not (img.strides[1] == 1 and img.strides[0] >= img.shape[1]):
        img = np.ascontiguousarray(img)
    return img


def _float_maps(map_x, map_y):
    mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
    assert mx.ndim == 2 and mx.shape == my.shape, "two H x W float32 maps expected"
    return mx, my


def remap_host(image, map_x, map_y):
    """orb_remap_host: cv::remap(image, out, map_x, map_y, INTER_LINEAR) with BORDER_CONSTANT 0 as OpenCV 3.2 computes
    it for 8-bit one-channel images and CV_32FC1 maps, on the CPU (the definition the GPU forms equal byte for byte).
    The result has the maps' size.  No context, no GPU."""
    img = _gray_image(image)
    mx, my = _float_maps(map_x, map_y)
    dh, dw = mx.shape
    out = np.zeros((dh, dw), np.uint8)
    check(lib().orb_remap_host(_p(img), img.shape[1], img.shape[0], img.strides[0], _p(mx), _p(my), dw * 4, dw, dh,
                               _p(out), dw), "orb_remap_host")
    return out


def rectify_maps_host(K, D, R, P, size):
    """orb_rectify_maps_host: cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F) of OpenCV 3.2, on the CPU.  K, R: 3 x 3;
    P: 3 x 3 or 3 x 4 (its left 3 x 3 is read); D: 4, 5 or 8 coefficients; size = (width, height).  Returns (map_x,
    map_y), float32 of shape (height, width).  A caller that has OpenCV may pass its own maps to Rectifier instead."""
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(3, 3))
    P33 = np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, -1)[:, :3])
    D = np.ascontiguousarray(np.asarray(D, np.float64).ravel())
    w, h = int(size[0]), int(size[1])
    mx, my = np.zeros((max(h, 0), max(w, 0)), np.float32), np.zeros((max(h, 0), max(w, 0)), np.float32)
    check(lib().orb_rectify_maps_host(_p(K), _p(D), len(D), _p(R), _p(P33), w, h, _p(mx), _p(my), w * 4),
          "orb_rectify_maps_host")
    return mx, my


def remap_device(ctx_or_matcher, rectifiers, d_src, nframes, sw, sh, src_frame_pitch, src_row_stride, d_dst,
                 dst_frame_pitch, dst_row_stride):
    """orb_remap_device: nframes frames in device memory through rectifiers[f % len(rectifiers)] in one launch,
    asynchronous on the context's stream (one Rectifier: a mono camera; two: interleaved left / right frames)."""
    hs = (ctypes.c_void_p * len(rectifiers))(*[r.h for r in rectifiers])
    check(lib().orb_remap_device(_ctx_handle(ctx_or_matcher), len(rectifiers), hs, d_src, nframes, sw, sh,
                                 src_frame_pitch, src_row_stride, d_dst, dst_frame_pitch, dst_row_stride),
          "orb_remap_device")


class Rectifier:
    """orb_rectify: one camera's rectification maps resident on the device, built once per camera from the CV_32FC1
    maps of cv::initUndistortRectifyMap (or rectify_maps_host).  remap(image) / rectifier(image) is cv::remap(image, out,
    M1, M2, cv::INTER_LINEAR) on the GPU (orb_remap).  Close it before the context that created it."""

    def __init__(self, ctx_or_matcher, map_x, map_y):
        mx, my = _float_maps(map_x, map_y)
        self._ctx = ctx_or_matcher
        self.h = ctypes.c_void_p()
        dh, dw = mx.shape
        check(lib().orb_rectify_create(_ctx_handle(ctx_or_matcher), dw, dh, _p(mx), _p(my), dw * 4,
                                       ctypes.byref(self.h)), "orb_rectify_create")

    @property
    def size(self):
        """(width, height) of the maps, which is the rectified image's."""
        w, h = ctypes.c_int(), ctypes.c_int()
        check(lib().orb_rectify_size(self.h, ctypes.byref(w), ctypes.byref(h)), "orb_rectify_size")
        return w.value, h.value

    def remap(self, image, ctx_or_matcher=None):
        img = _gray_image(image)
        dw, dh = self.size
        out = np.zeros((dh, dw), np.uint8)
        check(lib().orb_remap(_ctx_handle(ctx_or_matcher or self._ctx), self.h, _p(img), img.shape[1], img.shape[0],
                              img.strides[0], _p(out), dw), "orb_remap")
        return out

    __call__ = remap

    def close(self):
        if getattr(self, "h", None):
            lib().orb_rectify_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _front_image(image, color):
    """The fisheye camera's frame as the front-image entry points take it: H x W uint8 (color None or PREP_GRAY) or
    H x W x 3 / 4 uint8 (color = COLOR_*).  Returns (array, code)."""
    if color is None or color == PREP_GRAY:
        return _gray_image(image), PREP_GRAY
    return _color_image(image, color), color


def _mask_image(mask, shape):
    """The camera mask: None, H x W uint8 or H x W x 3 uint8 (channel 1 is read), of the frame's size.  Returns
    (array or None, channels, row stride)."""
    if mask is None:
        return None, 1, 0
    m = np.asarray(mask)
    assert m.dtype == np.uint8 and (m.ndim == 2 or (m.ndim == 3 and m.shape[2] == 3)), "H x W (x 3) uint8 mask expected"
    assert m.shape[:2] == tuple(shape), "the mask has the frame's size"
    m = np.ascontiguousarray(m)
    return m, 1 if m.ndim == 2 else 3, m.strides[0]


def front_prep_host(image, mask, crop, color=None):
    """orb_front_prep_host: the mono_fisheye driver's applyMask, crop (x, y, w, h; even sides) and half-size cv::resize,
    then Tracking's cvtColor, as OpenCV 3.2 computes them, on the CPU (the definition the GPU forms equal byte for
    byte).  image: H x W uint8, or H x W x 3 / 4 uint8 with color = COLOR_*; mask: None, H x W or H x W x 3 uint8 of the
    image's size (a pixel is zeroed where its mask byte, channel 1 of three, is > 250).  Returns the (h / 2, w / 2) gray
    image.  No context, no GPU."""
    img, code = _front_image(image, color)
    sh, sw = img.shape[:2]
    m, mc, ms = _mask_image(mask, (sh, sw))
    cx, cy, cw, ch = (int(v) for v in crop)
    out = np.zeros((max(ch, 0) // 2, max(cw, 0) // 2), np.uint8)
    check(lib().orb_front_prep_host(code, _p(img), sw, sh, img.strides[0], _p(m), mc, ms, cx, cy, cw, ch, _p(out),
                                    out.shape[1]), "orb_front_prep_host")
    return out


def bird_mask_host(mask_image):
    """orb_bird_mask_host: mono_fisheye.cc's ConvertMaskBirdview on the CPU.  mask_image: H x W x 3 / 4 uint8; returns
    the H x W mask, 0 where G < 20, else 250, with the vehicle footprint (bird_footprint_mask's rectangle) zeroed."""
    m = np.asarray(mask_image)
    assert m.dtype == np.uint8 and m.ndim == 3 and m.shape[2] in (3, 4), "H x W x 3 / 4 uint8 expected"
    m = np.ascontiguousarray(m)
    h, w, c = m.shape
    out = np.zeros((h, w), np.uint8)
    check(lib().orb_bird_mask_host(c, _p(m), w, h, m.strides[0], _p(out), w), "orb_bird_mask_host")
    return out


def front_prep_device(ctx_or_matcher, prep, color, d_src, nframes, src_frame_pitch, src_row_stride, d_dst,
                      dst_frame_pitch, dst_row_stride):
    """orb_front_prep_device: nframes camera frames in device memory through prep (a FrontPrep) in one launch,
    asynchronous on the context's stream; color is PREP_GRAY or COLOR_*.  d_dst is what
    BatchExtractor / orb_extract_batch_device consumes on the same stream."""
    check(lib().orb_front_prep_device(_ctx_handle(ctx_or_matcher), prep.h, PREP_GRAY if color is None else color, d_src,
                                      nframes, src_frame_pitch, src_row_stride, d_dst, dst_frame_pitch, dst_row_stride),
          "orb_front_prep_device")


def bird_mask_device(ctx_or_matcher, channels, d_src, nframes, w, h, src_frame_pitch, src_row_stride, d_dst,
                     dst_frame_pitch, dst_row_stride):
    """orb_bird_mask_device: ConvertMaskBirdview of nframes 3- or 4-channel masks in device memory in one launch,
    asynchronous on the context's stream.  d_dst is what BirdORB.extract_batch_device takes as d_masks; the birdview
    object has a stream of its own, so synchronise the context first."""
    check(lib().orb_bird_mask_device(_ctx_handle(ctx_or_matcher), channels, d_src, nframes, w, h, src_frame_pitch,
                                     src_row_stride, d_dst, dst_frame_pitch, dst_row_stride), "orb_bird_mask_device")


class FrontPrep:
    """orb_prep: the fisheye camera's mask and crop resident on the device, built once per camera.  size = (width,
    height) of the camera's frames; mask: None, H x W or H x W x 3 uint8 of that size; crop = (x, y, w, h) with even
    sides.  ORBextractor(frame, prep=this) is then the driver's applyMask, crop and half-size resize plus Tracking's
    cvtColor on the GPU in front of the extraction.  Close it before the context that created it."""

    def __init__(self, ctx_or_matcher, size, mask, crop):
        sw, sh = int(size[0]), int(size[1])
        m, mc, ms = _mask_image(mask, (sh, sw))
        cx, cy, cw, ch = (int(v) for v in crop)
        self.h = ctypes.c_void_p()
        check(lib().orb_prep_create(_ctx_handle(ctx_or_matcher), sw, sh, _p(m), mc, ms, cx, cy, cw, ch,
                                    ctypes.byref(self.h)), "orb_prep_create")

    def _pair(self, fn):
        w, h = ctypes.c_int(), ctypes.c_int()
        check(getattr(lib(), fn)(self.h, ctypes.byref(w), ctypes.byref(h)), fn)
        return w.value, h.value

    @property
    def size(self):
        """(width, height) of the prepared image: half the crop's."""
        return self._pair("orb_prep_size")

    @property
    def source_size(self):
        """(width, height) every frame given with this handle must have."""
        return self._pair("orb_prep_source_size")

    def close(self):
        if getattr(self, "h", None):
            lib().orb_prep_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def device_count():
    return lib().orb_device_count()


class _Ctx:
    def __init__(self, nfeatures, scale_factor, nlevels, ini_th, min_th, device=0, max_width=0,
                 max_height=0, max_batch=1, variant=0):
        self.params = OrbParams(nfeatures, scale_factor, nlevels, ini_th, min_th, device, max_width,
                                max_height, max_batch, variant)
        st = ctypes.c_int()
        self.h = lib().orb_create(ctypes.byref(self.params), ctypes.byref(st))
        if not self.h:
            raise OrbError(st.value, "orb_create")
        self.nlevels = nlevels

    def close(self):
        if getattr(self, "h", None):
            lib().orb_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    # debug views (parity tests pinpoint the failing stage)
    def debug_candidates(self, level, frame=0):
        cap = 1 << 16
        while True:
            out = np.zeros((cap, 3), np.int32)
            n = lib().orb_debug_candidates(self.h, frame, level, _p(out), cap)
            if n >= 0:
                return out[:n]
            if n == -1:
                raise OrbError(n, "orb_debug_candidates")
            cap = -n

    def debug_level_image(self, level, frame=0):
        """Pyramid level `level` of frame `frame` of the last extraction (orb_debug_level_image)."""
        w, h = ctypes.c_int(), ctypes.c_int()
        check(lib().orb_debug_level_image(self.h, frame, level, None, ctypes.byref(w), ctypes.byref(h)),
              "orb_debug_level_image")
        out = np.zeros((h.value, w.value), np.uint8)
        check(lib().orb_debug_level_image(self.h, frame, level, _p(out), ctypes.byref(w), ctypes.byref(h)),
              "orb_debug_level_image")
        return out

    def debug_level_keypoints(self, level, frame=0):
        out = np.zeros((1 << 15, 3), np.int32)
        n = lib().orb_debug_level_keypoints(self.h, frame, level, _p(out), len(out))
        if n < 0:
            raise OrbError(n, "orb_debug_level_keypoints")
        return out[:n]


class ORBextractor(_Ctx):
    """ORB_SLAM2::ORBextractor (ORBextractor.cc:410-470, 1043-1132) on one MI355X.  `variant` selects the
    OpenCV arithmetic the reference build links (VARIANT_* bits; 0 = the pinned OpenCV 3.2 default)."""

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0, variant=0):
        super().__init__(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, variant=variant)
        n = nlevels
        self._t = [np.zeros(n, np.float32) for _ in range(4)]
        self._npl = np.zeros(n, np.int32)
        self._umax = np.zeros(16, np.int32)
        check(lib().orb_scale_tables(self.h, *[_p(a) for a in self._t], _p(self._npl), _p(self._umax)),
              "orb_scale_tables")
        self._last_shape = None

    # getters (ORBextractor.h:63-83)
    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return float(self.params.scaleFactor)

    def GetScaleFactors(self):
        return self._t[0].copy()

    def GetInverseScaleFactors(self):
        return self._t[1].copy()

    def GetScaleSigmaSquares(self):
        return self._t[2].copy()

    def GetInverseScaleSigmaSquares(self):
        return self._t[3].copy()

    @property
    def mnFeaturesPerLevel(self):
        return self._npl.copy()

    @property
    def umax(self):
        return self._umax.copy()

    def __call__(self, image, mask=None, keypoints=None, descriptors=None, color=None, rectify=None, prep=None):
        """operator()(image, mask, keypoints, descriptors): returns (keypoints, descriptors).

        An empty image returns the given outputs untouched (ORBextractor.cc:1046-1047); mask is
        ignored as in the reference (ORBextractor.h:58).  color=COLOR_*: image is the camera's H x W x 3 / 4 colour
        image; the cvtColor of Tracking::GrabImage* runs on the GPU in front of the extraction (orb_extract_color) and
        mvImagePyramid[0] is then mImGray.  rectify=Rectifier: image is the camera's raw gray image; the cv::remap of the
        stereo examples runs on the GPU in front of the extraction (orb_extract_rectified) and mvImagePyramid[0] is then
        the rectified image.  prep=FrontPrep: image is the fisheye camera's raw frame (gray, or colour with color=);
        the mono_fisheye driver's applyMask, crop and half-size resize and the cvtColor run on the GPU in front of the
        extraction (orb_extract_fisheye) and mvImagePyramid[0] is then the prepared gray image."""
        img = np.asarray(image)
        if img.size == 0:
            return keypoints, descriptors
        assert color is None or rectify is None, "a colour image is converted before it is rectified"
        assert prep is None or rectify is None, "a fisheye frame is not rectified"
        if color == PREP_GRAY:
            color = None
        if color is None:
            assert img.dtype == np.uint8 and img.ndim == 2, "CV_8UC1 expected (ORBextractor.cc:1050)"
            if not (img.strides[1] == 1 and img.strides[0] >= img.shape[1]):   # rows with padding go down as they are
                img = np.ascontiguousarray(img)
        else:
            img = _color_image(img, color)
        h, w = img.shape[:2]
        # the entry point, what it takes between the context and the image, and the image's size where it takes one
        if prep is not None:
            assert (w, h) == prep.source_size, "the frame has the FrontPrep's source size"
            name, lead, dims = "orb_extract_fisheye", (prep.h, PREP_GRAY if color is None else color), ()
        elif rectify is not None:
            name, lead, dims = "orb_extract_rectified", (rectify.h,), (w, h)
        elif color is not None:
            name, lead, dims = "orb_extract_color", (color,), (w, h)
        else:
            name, lead, dims = "orb_extract", (), (w, h)
        fn = getattr(lib(), name)
        cap = 4 * max(self.params.nfeatures, 1) + 256
        while True:
            kps = np.zeros(cap, KP_DTYPE)
            desc = np.zeros((cap, 32), np.uint8)
            n = ctypes.c_int(0)
            st = fn(self.h, *lead, _p(img), *dims, img.strides[0], _p(kps), cap, ctypes.byref(n), _p(desc))
            if st == -3:
                cap = n.value
                continue
            check(st, name)
            break
        self._last_shape = prep.size[::-1] if prep is not None else (h, w) if rectify is None else rectify.size[::-1]
        return kps[:n.value].copy(), desc[:n.value].copy()

    @property
    def mvImagePyramid(self):
        """Host views of the last frame's pyramid levels (ORBextractor.h:85)."""
        out = []
        for l in range(self.nlevels):
            ptr, w, h, stride = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
            check(lib().orb_get_level(self.h, l, ctypes.byref(ptr), ctypes.byref(w), ctypes.byref(h),
                                      ctypes.byref(stride)), "orb_get_level")
            buf = (ctypes.c_uint8 * (stride.value * h.value)).from_address(ptr.value)
            out.append(np.ctypeslib.as_array(buf).reshape(h.value, stride.value)[:, :w.value].copy())
        return out

class BatchExtractor(_Ctx):
    """Device-resident batched extraction (orb_extract_batch_device): frames already in HBM."""

    def __init__(self, nfeatures, width, height, batch, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7,
                 device=0, variant=0):
        super().__init__(nfeatures, scale_factor, nlevels, ini_th, min_th, device, width, height, batch, variant)
        self.w, self.hgt, self.batch = width, height, batch
        self.kp_cap = lib().orb_batch_kp_cap(self.h, width, height)
        if self.kp_cap < 0:
            raise OrbError(self.kp_cap, "orb_batch_kp_cap")
        self.pitch = width
        self.d_frames = self._alloc(batch * width * height)
        self.d_kps = self._alloc(batch * self.kp_cap * 28)
        self.d_desc = self._alloc(batch * self.kp_cap * 32)
        self.d_counts = self._alloc(batch * 4)

    def _alloc(self, nbytes):
        p = lib().orb_device_alloc(self.h, nbytes)
        if not p:
            raise OrbError(-5, "orb_device_alloc")
        return p

    def _stage(self, name, frames):
        """frames into the device staging buffer self.<name> (d_color / d_raw), grown when it is too small."""
        if getattr(self, name + "_bytes", 0) < frames.nbytes:
            if getattr(self, name, None):
                lib().orb_device_free(self.h, getattr(self, name))
                setattr(self, name, None)
            setattr(self, name, self._alloc(frames.nbytes))
            setattr(self, name + "_bytes", frames.nbytes)
        check(lib().orb_memcpy_h2d(self.h, getattr(self, name), _p(frames), frames.nbytes), "h2d")

    def upload(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.shape == (self.batch, self.hgt, self.w)
        check(lib().orb_memcpy_h2d(self.h, self.d_frames, _p(frames), frames.nbytes), "h2d")

    def upload_color(self, frames, color):
        """The batch as the camera's colour frames ((batch, H, W, 3 / 4) uint8, color=COLOR_*): uploaded, then
        converted to gray on the device into the buffer launch() reads (orb_to_gray_device; asynchronous on the
        context's stream, so launch() may follow at once)."""
        ch = 3 if color in (COLOR_RGB, COLOR_BGR) else 4
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.shape == (self.batch, self.hgt, self.w, ch)
        self._stage("d_color", frames)
        check(lib().orb_to_gray_device(self.h, color, self.d_color, self.batch, self.w, self.hgt,
                                       self.w * self.hgt * ch, self.w * ch, self.d_frames, self.w * self.hgt, self.w),
              "orb_to_gray_device")

    def upload_raw(self, frames, rectifiers):
        """The batch as the cameras' raw gray frames ((batch, h, w) uint8, any raw size): uploaded, then rectified on
        the device into the buffer launch() reads (orb_remap_device, frame f through rectifiers[f % len(rectifiers)];
        asynchronous on the context's stream, so launch() may follow at once).  The maps have the extractor's size."""
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.ndim == 3 and frames.shape[0] == self.batch
        assert all(r.size == (self.w, self.hgt) for r in rectifiers), "the maps' size is the extractor's"
        sh, sw = frames.shape[1:]
        self._stage("d_raw", frames)
        remap_device(self, rectifiers, self.d_raw, self.batch, sw, sh, sw * sh, sw, self.d_frames, self.w * self.hgt,
                     self.w)

    def upload_fisheye(self, frames, prep, color=None):
        """The batch as the fisheye camera's raw frames ((batch, H, W) uint8, or (batch, H, W, 3 / 4) with
        color=COLOR_*; H x W is prep's source size): uploaded, then masked, cropped, halved and converted on the device
        into the buffer launch() reads (orb_front_prep_device; asynchronous on the context's stream, so launch() may
        follow at once).  prep's size is the extractor's."""
        ch = 1 if color in (None, PREP_GRAY) else 3 if color in (COLOR_RGB, COLOR_BGR) else 4
        frames = np.ascontiguousarray(frames, np.uint8)
        sw, sh = prep.source_size
        assert frames.shape == ((self.batch, sh, sw) if ch == 1 else (self.batch, sh, sw, ch))
        assert prep.size == (self.w, self.hgt), "the prepared image's size is the extractor's"
        self._stage("d_fisheye", frames)
        front_prep_device(self, prep, color, self.d_fisheye, self.batch, sw * sh * ch, sw * ch, self.d_frames,
                          self.w * self.hgt, self.w)

    def stereo_from_rgbd(self, dmap, mbf, d_kps_un, d_uright, d_depth, d_nvalid=None, nframes=None):
        """Frame::ComputeStereoFromRGBD for the frames of the last launch, on the device (orb_stereo_from_rgbd_device;
        asynchronous).  dmap: depth_map(...) over device memory; d_kps_un: the undistorted keypoints in the layout of
        d_kps (d_kps itself without distortion); outputs at [f * kp_cap + i] (device pointers)."""
        n = self.batch if nframes is None else nframes
        check(lib().orb_stereo_from_rgbd_device(self.h, ctypes.byref(dmap), float(np.float32(mbf)), n, self.d_kps,
                                                d_kps_un, self.d_counts, self.kp_cap, d_uright, d_depth, d_nvalid),
              "orb_stereo_from_rgbd_device")

    def launch(self, nframes=None):
        n = self.batch if nframes is None else nframes
        check(lib().orb_extract_batch_device(self.h, self.d_frames, n, self.w, self.hgt, self.w * self.hgt,
                                             self.w, self.d_kps, self.d_desc, self.d_counts, self.kp_cap),
              "orb_extract_batch_device")

    def sync(self):
        check(lib().orb_sync(self.h), "orb_sync")

    def counts(self):
        out = np.zeros(self.batch, np.int32)
        check(lib().orb_memcpy_d2h(self.h, _p(out), self.d_counts, out.nbytes), "d2h")
        return out

    def results(self, frame):
        n = int(self.counts()[frame])
        kps = np.zeros(self.kp_cap, KP_DTYPE)
        desc = np.zeros((self.kp_cap, 32), np.uint8)
        check(lib().orb_memcpy_d2h(self.h, _p(kps), self.d_kps + frame * self.kp_cap * 28, kps.nbytes), "d2h")
        check(lib().orb_memcpy_d2h(self.h, _p(desc), self.d_desc + frame * self.kp_cap * 32, desc.nbytes), "d2h")
        return kps[:n], desc[:n]

    def frame_slots(self, frame):
        """(n, d_desc, d_kps): the keypoint count and the device pointers of frame `frame`'s output slots of the last
        launch, as Frame.from_device takes them: a resident Frame without a host copy of the descriptors."""
        n = int(self.counts()[frame])
        return n, self.d_desc + frame * self.kp_cap * 32, self.d_kps + frame * self.kp_cap * 28

    def profile(self, on=True):
        check(lib().orb_profile_enable(self.h, int(on)), "orb_profile_enable")

    def profile_read(self):
        ms = np.zeros(7, np.float64)   # ORB_K_COUNT
        n = np.zeros(7, np.int32)
        check(lib().orb_profile_read(self.h, _p(ms), _p(n)), "orb_profile_read")
        return ms, n

    def stereo(self, npairs, mb, mbf, d_uright, d_depth, d_nmatched):
        """Frame::ComputeStereoMatches for frame pairs (2p, 2p+1) of the last launch, on the device."""
        check(lib().orb_stereo_batch_device(self.h, npairs, mb, mbf, d_uright, d_depth, d_nmatched),
              "orb_stereo_batch_device")

    def hamming_top2_frames(self, q_frames, t_frames, d_best, d_idx, d_second):
        """All-pairs top-2 between frames q_frames[p] and t_frames[p] of the last launch, one launch."""
        qf = np.ascontiguousarray(q_frames, np.int32)
        tf = np.ascontiguousarray(t_frames, np.int32)
        check(lib().orb_hamming_top2_frames_device(self.h, self.d_desc, self.d_counts, self.kp_cap, len(qf), _p(qf),
                                                   _p(tf), d_best, d_idx, d_second), "orb_hamming_top2_frames_device")

    def hamming_top2(self, d_q, nq, d_t, nt, d_best, d_idx, d_second):
        check(lib().orb_hamming_top2_device(self.h, d_q, nq, d_t, nt, d_best, d_idx, d_second),
              "orb_hamming_top2_device")

    def close(self):
        if getattr(self, "h", None):
            for p in ("d_frames", "d_kps", "d_desc", "d_counts", "d_color", "d_raw", "d_fisheye"):
                if getattr(self, p, None):
                    lib().orb_device_free(self.h, getattr(self, p))
                    setattr(self, p, None)
        super().close()


def _featvec(fv):
    """dict {node_id: [indices]} (DBoW2::FeatureVector) -> (OrbFeatVec, keepalive)."""
    ids = np.array(sorted(fv.keys()), np.uint32)
    groups = [np.asarray(fv[int(k)], np.int32) for k in ids]
    off = np.zeros(len(groups) + 1, np.int32)
    if groups:
        off[1:] = np.cumsum([len(g) for g in groups])
    idx = np.ascontiguousarray(np.concatenate(groups) if groups else np.zeros(1, np.int32), np.int32)
    s = OrbFeatVec(len(ids), ids.ctypes.data if len(ids) else None, off.ctypes.data, idx.ctypes.data)
    return s, (ids, off, idx)


def compute_stereo_matches(left, right, kpsL, descL, kpsR, descR, mb, mbf):
    """Frame::ComputeStereoMatches (Frame.cc:662-836): left / right are the ORBextractors that
    extracted the rectified left / right images last.  Returns (mvuRight, mvDepth, n_with_depth)."""
    kl = np.ascontiguousarray(kpsL, KP_DTYPE)
    kr = np.ascontiguousarray(kpsR, KP_DTYPE)
    dl = np.ascontiguousarray(descL, np.uint8)
    dr = np.ascontiguousarray(descR, np.uint8)
    u = np.zeros(max(len(kl), 1), np.float32)
    d = np.zeros(max(len(kl), 1), np.float32)
    n = ctypes.c_int(0)
    check(lib().orb_compute_stereo_matches(left.h, right.h, len(kl), _p(kl), _p(dl), len(kr), _p(kr), _p(dr), mb, mbf,
                                           _p(u), _p(d), ctypes.byref(n)), "orb_compute_stereo_matches")
    return u[:len(kl)], d[:len(kl)], n.value


def features_in_area(kps_un, min_x, max_x, min_y, max_y, x, y, r, min_level=-1, max_level=-1):
    """Frame::GetFeaturesInArea (Frame.cc:494-547) over the 64x48 grid."""
    k = np.ascontiguousarray(kps_un, KP_DTYPE)
    out = np.zeros(max(1, len(k)), np.int32)
    n = lib().orb_features_in_area(len(k), _p(k), min_x, max_x, min_y, max_y, x, y, r, min_level, max_level,
                                   _p(out), len(out))
    return out[:n]


def frame_grid(kps_un, min_x, max_x, min_y, max_y):
    """Frame::AssignFeaturesToGrid (Frame.cc:378-393, PosInGrid :549-559) as the C-ABI's orb_frame_grid
    CSR: cell (ix, iy) holds its keypoint indices in order at cell_idx[cell_off[ix*48+iy] ..].  Returns
    (inv_w, inv_h, cell_off, cell_idx) with the float32 arithmetic of the reference."""
    k = np.asarray(kps_un, KP_DTYPE)
    f32 = np.float32
    inv_w = f32(64) / (f32(max_x) - f32(min_x))
    inv_h = f32(48) / (f32(max_y) - f32(min_y))
    vx = ((k["x"].astype(f32) - f32(min_x)) * inv_w).astype(np.float64)
    vy = ((k["y"].astype(f32) - f32(min_y)) * inv_h).astype(np.float64)
    px = (np.sign(vx) * np.floor(np.abs(vx) + 0.5)).astype(np.int64)   # std::round: half away from zero
    py = (np.sign(vy) * np.floor(np.abs(vy) + 0.5)).astype(np.int64)
    ok = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    cell = np.where(ok, px * 48 + py, -1)
    order = np.argsort(np.where(ok, cell, 1 << 30), kind="stable")[: int(ok.sum())]
    off = np.zeros(64 * 48 + 1, np.int32)
    np.add.at(off, cell[ok] + 1, 1)
    return float(inv_w), float(inv_h), np.cumsum(off).astype(np.int32), order.astype(np.int32)


def _frame_grid_arg(grid, min_xy=(0.0, 0.0)):
    """A frame_grid(...) tuple as the C-ABI's orb_frame_grid, and the arrays it points into, which the caller keeps
    alive for as long as the struct is in use.  An empty cell_idx goes down as one unused slot, not as a NULL."""
    inv_w, inv_h, off, idx = grid
    off = np.ascontiguousarray(off, np.int32)
    idx = np.ascontiguousarray(idx, np.int32) if len(idx) else np.zeros(1, np.int32)
    g = OrbFrameGrid(float(min_xy[0]), float(min_xy[1]), inv_w, inv_h, off.ctypes.data, idx.ctypes.data)
    return g, (off, idx)


def _ctx_handle(ctx_or_matcher):
    c = getattr(ctx_or_matcher, "_ctx", ctx_or_matcher)
    return c.h


class Frame:
    """A device-resident Frame / KeyFrame (orb_frame): descriptors, undistorted keypoints and optionally mvuRight,
    uploaded once, with the Frame grid built on the GPU (Frame::AssignFeaturesToGrid).  The grid searches of ORBmatcher
    take it as their train side (frame=...), so a frame searched several times is staged once.

    Frame(ctx_or_matcher, desc, kps_un, bounds=(mnMinX, mnMaxX, mnMinY, mnMaxY), uright=None) derives the inverse cell
    sizes as frame_grid() does; Frame(..., inv=(inv_w, inv_h)) gives them directly with origin min_xy (default (0, 0):
    the birdview grid).  ctx_or_matcher: an ORBmatcher, or any object of this module that owns a context (its GPU is
    the frame's).  close() frees it; close every Frame before its context."""

    def __init__(self, ctx_or_matcher, desc, kps_un, bounds=None, inv=None, uright=None, min_xy=(0.0, 0.0)):
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        k = np.ascontiguousarray(kps_un, KP_DTYPE)
        ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
        assert len(d) == len(k) and (ur is None or len(ur) == len(k))
        self._create("orb_frame_create", ctx_or_matcher, len(k), _p(d), _p(k), _p(ur), bounds, inv, min_xy)

    @classmethod
    def from_device(cls, ctx_or_matcher, n, d_desc, d_kps, bounds=None, inv=None, d_uright=None, min_xy=(0.0, 0.0)):
        """A Frame from n descriptors / keypoints (and optionally uright) already in device memory of the context's
        GPU (ints: e.g. BatchExtractor.frame_slots(f)); copied device-to-device."""
        self = cls.__new__(cls)
        vp = ctypes.c_void_p
        self._create("orb_frame_create_device", ctx_or_matcher, int(n), vp(d_desc), vp(d_kps),
                     None if d_uright is None else vp(d_uright), bounds, inv, min_xy)
        return self

    @classmethod
    def from_extraction(cls, ctx_or_matcher, dist, n, d_desc, d_kps_raw, bounds=None, inv=None, d_uright=None,
                        min_xy=(0.0, 0.0)):
        """A Frame from n descriptors and RAW keypoints in device memory (BatchExtractor.frame_slots(f)):
        orb_frame_create_from_extract undistorts them on the GPU (dist: distortion(...)) and builds the grid from the
        undistorted ones, so the extraction's output becomes a searchable frame without leaving the device.  bounds
        is image_bounds(dist, w, h)."""
        self = cls.__new__(cls)
        vp = ctypes.c_void_p
        self._create("orb_frame_create_from_extract", ctx_or_matcher, int(n), vp(d_desc), vp(d_kps_raw),
                     None if d_uright is None else vp(d_uright), bounds, inv, min_xy, dist=dist)
        return self

    @classmethod
    def from_batch(cls, ctx_or_matcher, dist, nframes, d_desc, d_kps_raw, d_counts, kp_cap, bounds=None, inv=None,
                   min_xy=(0.0, 0.0)):
        """nframes Frames from a whole batch in orb_extract_batch_device's output layout (BatchExtractor's d_desc,
        d_kps, d_counts, kp_cap): orb_frames_create_from_batch, one undistort launch for all frames."""
        proto = cls.__new__(cls)
        proto.h = None
        proto._set_grid(bounds, inv, min_xy)
        vp = ctypes.c_void_p
        handles = (vp * max(int(nframes), 1))()
        fn = "orb_frames_create_from_batch"
        check(getattr(lib(), fn)(_ctx_handle(ctx_or_matcher), ctypes.byref(dist), int(nframes), vp(d_desc),
                                 vp(d_kps_raw), vp(d_counts), int(kp_cap), proto.min_xy[0], proto.min_xy[1],
                                 proto.inv[0], proto.inv[1], handles), fn)
        frames = []
        for f in range(int(nframes)):
            self = cls.__new__(cls)
            self.min_xy, self.inv, self.has_uright = proto.min_xy, proto.inv, False
            self.h = vp(handles[f])
            self.n = lib().orb_frame_count(self.h)
            frames.append(self)
        return frames

    @classmethod
    def from_batch_rgbd(cls, ctx_or_matcher, dist, dmap, mbf, nframes, d_desc, d_kps_raw, d_counts, kp_cap, bounds=None,
                        inv=None, min_xy=(0.0, 0.0), d_uright=None, d_depth=None):
        """The RGB-D Frame constructor after extraction for a whole batch (orb_frames_create_from_batch_rgbd): from_batch
        with Frame::ComputeStereoFromRGBD on the undistorted keypoints; dmap: depth_map(...) over device memory.  Every
        Frame carries its uright; d_uright / d_depth (device pointers, nframes * kp_cap floats, optional) receive
        mvuRight / mvDepth."""
        proto = cls.__new__(cls)
        proto.h = None
        proto._set_grid(bounds, inv, min_xy)
        vp = ctypes.c_void_p
        handles = (vp * max(int(nframes), 1))()
        fn = "orb_frames_create_from_batch_rgbd"
        check(getattr(lib(), fn)(_ctx_handle(ctx_or_matcher), ctypes.byref(dist), ctypes.byref(dmap),
                                 float(np.float32(mbf)), int(nframes), vp(d_desc), vp(d_kps_raw), vp(d_counts),
                                 int(kp_cap), proto.min_xy[0], proto.min_xy[1], proto.inv[0], proto.inv[1],
                                 None if d_uright is None else vp(d_uright), None if d_depth is None else vp(d_depth),
                                 handles), fn)
        frames = []
        for f in range(int(nframes)):
            self = cls.__new__(cls)
            self.min_xy, self.inv, self.has_uright = proto.min_xy, proto.inv, True
            self.h = vp(handles[f])
            self.n = lib().orb_frame_count(self.h)
            frames.append(self)
        return frames

    @classmethod
    def from_batch_stereo(cls, ctx_or_matcher, dist, npairs, mb, mbf, d_desc, d_kps_raw, d_counts, kp_cap, bounds=None,
                          inv=None, min_xy=(0.0, 0.0), d_uright=None, d_depth=None):
        """The stereo Frame constructor after extraction for a whole batch (orb_frames_create_from_batch_stereo), after
        a launch of 2 * npairs frames on the same context (slots 2p, 2p + 1 = left, right): undistortion of the left
        keypoints, Frame::ComputeStereoMatches on the raw ones, the left frames' grids.  Every Frame carries its uright;
        d_uright / d_depth (device pointers, npairs * kp_cap floats, optional) receive mvuRight / mvDepth."""
        proto = cls.__new__(cls)
        proto.h = None
        proto._set_grid(bounds, inv, min_xy)
        vp = ctypes.c_void_p
        handles = (vp * max(int(npairs), 1))()
        fn = "orb_frames_create_from_batch_stereo"
        check(getattr(lib(), fn)(_ctx_handle(ctx_or_matcher), ctypes.byref(dist), int(npairs), float(np.float32(mb)),
                                 float(np.float32(mbf)), vp(d_desc), vp(d_kps_raw), vp(d_counts), int(kp_cap),
                                 proto.min_xy[0], proto.min_xy[1], proto.inv[0], proto.inv[1],
                                 None if d_uright is None else vp(d_uright), None if d_depth is None else vp(d_depth),
                                 handles), fn)
        frames = []
        for f in range(int(npairs)):
            self = cls.__new__(cls)
            self.min_xy, self.inv, self.has_uright = proto.min_xy, proto.inv, True
            self.h = vp(handles[f])
            self.n = lib().orb_frame_count(self.h)
            frames.append(self)
        return frames

    def _set_grid(self, bounds, inv, min_xy):
        assert (bounds is None) != (inv is None), "give bounds=(min_x, max_x, min_y, max_y) or inv=(inv_w, inv_h)"
        f32 = np.float32
        if bounds is not None:
            min_x, max_x, min_y, max_y = bounds
            inv_w = f32(64) / (f32(max_x) - f32(min_x))   # Frame.cc:102-103, as frame_grid()
            inv_h = f32(48) / (f32(max_y) - f32(min_y))
        else:
            (min_x, min_y), (inv_w, inv_h) = min_xy, inv
        self.min_xy, self.inv = (float(f32(min_x)), float(f32(min_y))), (float(inv_w), float(inv_h))

    def _create(self, fn, ctx_or_matcher, n, desc, kps, ur, bounds, inv, min_xy, dist=None):
        self.h = None
        if dist is not None:
            self._set_grid(bounds, inv, min_xy)
            self.has_uright = ur is not None
            out = ctypes.c_void_p()
            check(getattr(lib(), fn)(_ctx_handle(ctx_or_matcher), ctypes.byref(dist), n, desc, kps, ur, self.min_xy[0],
                                     self.min_xy[1], self.inv[0], self.inv[1], ctypes.byref(out)), fn)
            self.h = out
            self.n = lib().orb_frame_count(self.h)
            return
        assert (bounds is None) != (inv is None), "give bounds=(min_x, max_x, min_y, max_y) or inv=(inv_w, inv_h)"
        f32 = np.float32
        if bounds is not None:
            min_x, max_x, min_y, max_y = bounds
            inv_w = f32(64) / (f32(max_x) - f32(min_x))   # Frame.cc:102-103, as frame_grid()
            inv_h = f32(48) / (f32(max_y) - f32(min_y))
        else:
            (min_x, min_y), (inv_w, inv_h) = min_xy, inv
        self.min_xy, self.inv = (float(f32(min_x)), float(f32(min_y))), (float(inv_w), float(inv_h))
        self.has_uright = ur is not None
        out = ctypes.c_void_p()
        check(getattr(lib(), fn)(_ctx_handle(ctx_or_matcher), n, desc, kps, ur, self.min_xy[0], self.min_xy[1],
                                 self.inv[0], self.inv[1], ctypes.byref(out)), fn)
        self.h = out
        self.n = lib().orb_frame_count(self.h)

    def __len__(self):
        return self.n

    def grid(self):
        """(cell_off, cell_idx) of the grid the GPU built, as frame_grid() returns them."""
        off = np.zeros(64 * 48 + 1, np.int32)
        idx = np.zeros(max(self.n, 1), np.int32)
        ns = ctypes.c_int()
        check(lib().orb_frame_grid_read(self.h, _p(off), _p(idx), self.n, ctypes.byref(ns)), "orb_frame_grid_read")
        return off, idx[:ns.value]

    def compute_bow(self, vocab, levelsup=4, ctx_or_matcher=None):
        """Frame::ComputeBoW on the device (orb_frame_compute_bow): the handle then carries its FeatureVector (and
        the per-feature triples) for the vocabulary-gated searches; bow() reads both vectors back."""
        compute_bow(vocab, [self], levelsup, ctx_or_matcher)

    def set_featvec(self, featvec, ctx_or_matcher):
        """Attach a FeatureVector the caller holds ({node: [feature indices]}, a KeyFrame's mFeatVec)."""
        fv, keep = _featvec(featvec)
        check(lib().orb_frame_set_featvec(_ctx_handle(ctx_or_matcher), self.h, fv), "orb_frame_set_featvec")
        self._fv_sizes = (len(keep[0]), int(keep[1][-1]))

    @property
    def has_bow(self):
        return lib().orb_frame_has_bow(self.h) != 0

    def bow(self, vocab=None):
        """(BowVector {word: value}, FeatureVector {node: [i]}) as ORBVocabulary.transform returns them; the BowVector
        is empty for a handle whose FeatureVector came from set_featvec."""
        n = max(self.n, 1)
        bw, bv = np.zeros(n, np.int32), np.zeros(n, np.float64)
        size = max(n, *(getattr(self, "_fv_sizes", None) or (0, 0)))   # a given CSR may hold more than n entries
        fn, fo, fi = np.zeros(size, np.uint32), np.zeros(size + 1, np.int32), np.zeros(size, np.int32)
        nb, nf = ctypes.c_int(), ctypes.c_int()
        v = None if vocab is None else vocab.v
        check(lib().orb_frame_bow_read(v, self.h, _p(bw), _p(bv), ctypes.byref(nb), _p(fn), _p(fo), _p(fi),
                                       ctypes.byref(nf)), "orb_frame_bow_read")
        bowv = {int(bw[i]): float(bv[i]) for i in range(nb.value)}
        fv = {int(fn[j]): fi[fo[j]:fo[j + 1]].tolist() for j in range(nf.value)}
        return bowv, fv

    def close(self):
        if getattr(self, "h", None):
            lib().orb_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def compute_bow(vocab, frames, levelsup=4, ctx_or_matcher=None):
    """orb_frame_compute_bow for a list of Frames in one call: one vocabulary-transform launch over all their resident
    descriptors and one FeatureVector launch.  vocab: an ORBVocabulary of the frames' GPU (its context runs the call
    unless ctx_or_matcher is given)."""
    hs = (ctypes.c_void_p * max(len(frames), 1))(*[f.h for f in frames])
    h = vocab._ctx.h if ctx_or_matcher is None else _ctx_handle(ctx_or_matcher)
    check(lib().orb_frame_compute_bow(h, vocab.v, int(levelsup), len(frames), hs), "orb_frame_compute_bow")
    for f in frames:
        f._fv_sizes = None


def distortion(fx, fy, cx, cy, k):
    """orb_distortion from mK's entries and mDistCoef's four floats (Camera.k1, k2, p1, p2 in Tracking.cc's order; the
    fisheye model reads them as k1..k4), all taken as float32."""
    k = np.asarray(k, np.float32).ravel()
    assert len(k) == 4, "four coefficients (a fifth is out of scope: cv::fisheye::undistortPoints asserts on it)"
    d = OrbDistortion()
    d.fx, d.fy, d.cx, d.cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    d.k[:] = [float(v) for v in k]
    return d


def undistort_points_host(dist, xy):
    """orb_undistort_points_host: cv::fisheye::undistortPoints as Frame::UndistortKeyPoints calls it, on the CPU (the
    definition the GPU forms equal byte for byte).  xy: (n, 2) float32; no context, no GPU."""
    p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros_like(p)
    check(lib().orb_undistort_points_host(ctypes.byref(dist), len(p), _p(p), _p(out)), "orb_undistort_points_host")
    return out


def image_bounds(dist, w, h):
    """orb_image_bounds: Frame::ComputeImageBounds' (mnMinX, mnMaxX, mnMinY, mnMaxY) as float32; no context, no GPU."""
    b = [ctypes.c_float() for _ in range(4)]
    check(lib().orb_image_bounds(ctypes.byref(dist), int(w), int(h), *[ctypes.byref(v) for v in b]), "orb_image_bounds")
    return np.array([v.value for v in b], np.float32)


def undistort_keypoints(ctx_or_matcher, dist, kps):
    """orb_undistort_keypoints: Frame::UndistortKeyPoints on the GPU.  Returns (mvKeysUn, n_redone): the keypoints with
    x, y undistorted (the bytes of undistort_points_host) and how many the host recomputed."""
    k = np.ascontiguousarray(kps, KP_DTYPE)
    out = np.zeros(len(k), KP_DTYPE)
    n = ctypes.c_int(0)
    check(lib().orb_undistort_keypoints(_ctx_handle(ctx_or_matcher), ctypes.byref(dist), len(k), _p(k), _p(out),
                                        ctypes.byref(n)), "orb_undistort_keypoints")
    return out, n.value


def undistort_guard(ctx_or_matcher, g=0.0):
    """orb_debug_undistort_guard: the guard band's relative half-width for this context (0: the default)."""
    check(lib().orb_debug_undistort_guard(_ctx_handle(ctx_or_matcher), float(g)), "orb_debug_undistort_guard")


def camera(Rcw, tcw, Ow, fx, fy, cx, cy, mbf, bounds, scale_factors, log_scale_factor):
    """orb_camera from a Frame's / KeyFrame's members: Rcw (3x3), tcw, Ow, the intrinsics, bounds = (mnMinX, mnMaxX,
    mnMinY, mnMaxY), mvScaleFactors and mfLogScaleFactor, all taken as float32."""
    f32 = np.float32
    sf = np.asarray(scale_factors, f32).ravel()
    assert len(sf) <= 16
    c = OrbCamera()
    c.Rcw[:] = np.asarray(Rcw, f32).ravel().tolist()
    c.tcw[:] = np.asarray(tcw, f32).ravel().tolist()
    c.Ow[:] = np.asarray(Ow, f32).ravel().tolist()
    c.fx, c.fy, c.cx, c.cy, c.mbf = (float(f32(x)) for x in (fx, fy, cx, cy, mbf))
    c.min_x, c.max_x, c.min_y, c.max_y = (float(f32(x)) for x in bounds)
    c.nlevels, c.log_scale_factor = len(sf), float(f32(log_scale_factor))
    for i, x in enumerate(sf):
        c.scale_factors[i] = float(x)
    return c


def _point_arrays(pos, normal, min_dist, max_dist):
    f32 = np.float32
    p = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    nr = np.ascontiguousarray(normal, f32).reshape(-1, 3)
    lo, hi = np.ascontiguousarray(min_dist, f32).ravel(), np.ascontiguousarray(max_dist, f32).ravel()
    assert len(p) == len(nr) == len(lo) == len(hi)
    return p, nr, lo, hi


def project_points_host(mode, cam, pos, normal, min_dist, max_dist, view_cos_limit=0.5, th=1.0):
    """orb_project_points_host: the records of orb_project_points on the CPU, from host arrays; no context, no GPU."""
    p, nr, lo, hi = _point_arrays(pos, normal, min_dist, max_dist)
    out = np.zeros(len(p), POINT_PROJ_DTYPE)
    check(lib().orb_project_points_host(int(mode), ctypes.byref(cam), float(view_cos_limit), float(th), len(p), _p(p),
                                        _p(nr), _p(lo), _p(hi), _p(out)), "orb_project_points_host")
    return out


class MapPoints:
    """Map points resident on the device (orb_points): per slot GetWorldPos, GetNormal, the raw mfMinDistance /
    mfMaxDistance and GetDescriptor.  write() fills or rewrites a slot range (and grows the handle), project() runs
    Frame::isInFrustum (FRUSTUM_FRAME) or Fuse's projection (FRUSTUM_FUSE) for a list of slot ids on the GPU; the
    fused searches are ORBmatcher.SearchLocalPoints / FuseSearchPoints.  len() is the capacity.  close() frees it;
    close it before its context."""

    def __init__(self, ctx_or_matcher, capacity=0):
        self.h = None
        self._ctx_h = _ctx_handle(ctx_or_matcher)
        out = ctypes.c_void_p()
        check(lib().orb_points_create(self._ctx_h, int(capacity), ctypes.byref(out)), "orb_points_create")
        self.h = out

    def write(self, first, pos, normal, min_dist, max_dist, desc):
        p, nr, lo, hi = _point_arrays(pos, normal, min_dist, max_dist)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert len(d) == len(p)
        check(lib().orb_points_write(self.h, int(first), len(p), _p(p), _p(nr), _p(lo), _p(hi), _p(d)),
              "orb_points_write")

    def __len__(self):
        return lib().orb_points_capacity(self.h)

    def project(self, mode, cam, ids, view_cos_limit=0.5, th=1.0, ctx_or_matcher=None):
        """orb_project_points: POINT_PROJ_DTYPE records for the slots ids, in ids order."""
        ids = np.ascontiguousarray(ids, np.int32).ravel()
        out = np.zeros(len(ids), POINT_PROJ_DTYPE)
        h = self._ctx_h if ctx_or_matcher is None else _ctx_handle(ctx_or_matcher)
        check(lib().orb_project_points(h, self.h, int(mode), ctypes.byref(cam), float(view_cos_limit), float(th),
                                       len(ids), _p(ids) if len(ids) else None, _p(out)), "orb_project_points")
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().orb_points_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class _ProjFrameTargets:
    """orb_proj_frame_target array over target dicts: q, qdesc, frame (a Frame) and optionally inv_sigma2."""

    def __init__(self, targets):
        self.keep, self.out = [], []
        self.arr = (OrbProjFrameTarget * max(len(targets), 1))()
        for k, t in enumerate(targets):
            q = np.ascontiguousarray(t["q"], PROJ_QUERY_DTYPE)
            qd = np.ascontiguousarray(t["qdesc"], np.uint8).reshape(-1, 32)
            assert len(q) == len(qd)
            inv = None if t.get("inv_sigma2") is None else np.ascontiguousarray(t["inv_sigma2"], np.float32)
            bi, bd = np.full(max(len(q), 1), -1, np.int32), np.full(max(len(q), 1), -1, np.int32)
            self.arr[k] = OrbProjFrameTarget(len(q), _p(q), _p(qd), t["frame"].h, _p(inv),
                                             0 if inv is None else len(inv), _p(bi), _p(bd))
            self.keep.append((q, qd, inv, t["frame"]))
            self.out.append((bi[:len(q)], bd[:len(q)]))


def proj_queries(u, v, radius, level, ur=None, level_above=0, angle=None):
    """PROJ_QUERY_DTYPE array of projected map points with predicted levels `level`: the window (u, v, radius), the
    level range (level - 1, level + level_above), ur (Fuse's gate), angle (the rotation check); blocks = 1."""
    level = np.asarray(level, np.int32)
    q = np.zeros(len(level), PROJ_QUERY_DTYPE)
    q["u"], q["v"], q["r"] = np.asarray(u, np.float32), np.asarray(v, np.float32), np.asarray(radius, np.float32)
    q["min_level"], q["max_level"] = level - 1, level + int(level_above)
    if ur is not None:
        q["ur"] = np.asarray(ur, np.float32)
    if angle is not None:
        q["angle"] = np.asarray(angle, np.float32)
    q["blocks"] = 1
    return q


class _ProjTargets:
    """orb_proj_target array over a list of target dicts: q (PROJ_QUERY_DTYPE), qdesc, tdesc, kps_t, grid
    (frame_grid(...)), and optionally min_xy ((mnMinX, mnMinY), default (0, 0)), t_uright (mvuRight), inv_sigma2
    (mvInvLevelSigma2).  Holds the marshalled arrays alive and the per-target outputs (best_idx, best_dist)."""

    def __init__(self, targets):
        self.keep, self.out = [], []
        self.arr = (OrbProjTarget * max(len(targets), 1))()
        for k, t in enumerate(targets):
            q = np.ascontiguousarray(t["q"], PROJ_QUERY_DTYPE)
            qd = np.ascontiguousarray(t["qdesc"], np.uint8).reshape(-1, 32)
            td = np.ascontiguousarray(t["tdesc"], np.uint8).reshape(-1, 32)
            kt = np.ascontiguousarray(t["kps_t"], KP_DTYPE)
            assert len(q) == len(qd) and len(td) == len(kt)
            ur = None if t.get("t_uright") is None else np.ascontiguousarray(t["t_uright"], np.float32)
            inv = None if t.get("inv_sigma2") is None else np.ascontiguousarray(t["inv_sigma2"], np.float32)
            assert ur is None or len(ur) == len(kt)
            g, grid_arrays = _frame_grid_arg(t["grid"], t.get("min_xy", (0.0, 0.0)))
            bi, bd = np.full(max(len(q), 1), -1, np.int32), np.full(max(len(q), 1), -1, np.int32)
            self.arr[k] = OrbProjTarget(len(q), _p(q), _p(qd), len(kt), _p(td), _p(kt), _p(ur), _p(inv),
                                        0 if inv is None else len(inv), g, _p(bi), _p(bd))
            self.keep.append((q, qd, td, kt, ur, inv) + grid_arrays)
            self.out.append((bi[:len(q)], bd[:len(q)]))


def project_best_host(gate, target, query):
    """orb_project_best_host: one query of one target (a dict as for ORBmatcher.project_best_batch) on the CPU, with
    the arithmetic and the result of the batched GPU call; no context, no GPU.  Returns (best_idx, best_dist)."""
    T = _ProjTargets([target])
    bi, bd = ctypes.c_int(-1), ctypes.c_int(-1)
    check(lib().orb_project_best_host(int(gate), ctypes.addressof(T.arr), int(query), ctypes.byref(bi),
                                      ctypes.byref(bd)), "orb_project_best_host")
    return bi.value, bd.value


def _kf_target(kf, pts, level_above=0):
    """A target dict from a keyframe dict (desc, kps, grid, and optionally min_xy, uright, inv_sigma2; or frame (a
    Frame) and optionally inv_sigma2) and its projected points (u, v, radius, level, desc, and optionally ur)."""
    if kf.get("frame") is not None:
        return dict(q=proj_queries(pts["u"], pts["v"], pts["radius"], pts["level"], pts.get("ur"), level_above),
                    qdesc=pts["desc"], frame=kf["frame"], inv_sigma2=kf.get("inv_sigma2"))
    return dict(q=proj_queries(pts["u"], pts["v"], pts["radius"], pts["level"], pts.get("ur"), level_above),
                qdesc=pts["desc"], tdesc=kf["desc"], kps_t=kf["kps"], grid=kf["grid"],
                min_xy=kf.get("min_xy", (0.0, 0.0)), t_uright=kf.get("uright"), inv_sigma2=kf.get("inv_sigma2"))


class ORBmatcher:
    """ORB_SLAM2::ORBmatcher's descriptor matchers (ORBmatcher.cc) on the GPU."""

    _shared_ctx = {}

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        key = device
        if key not in ORBmatcher._shared_ctx:   # matchers are stack objects in the reference: share a context
            ORBmatcher._shared_ctx[key] = _Ctx(1000, 1.2, 8, 20, 7, device)
        self._ctx = ORBmatcher._shared_ctx[key]

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib().orb_descriptor_distance(_p(a), _p(b))

    def hamming_topk(self, q, t, k=2, cand_off=None, cand_idx=None, train_thr=None):
        q = np.ascontiguousarray(q, np.uint8)
        t = np.ascontiguousarray(t, np.uint8)
        nq = len(q)
        dist = np.zeros((nq, k), np.int32)
        idx = np.zeros((nq, k), np.int32)
        nv = np.zeros(nq, np.int32)
        co = None if cand_off is None else np.ascontiguousarray(cand_off, np.int32)
        cx = None if cand_idx is None else np.ascontiguousarray(cand_idx, np.int32)
        th = None if train_thr is None else np.ascontiguousarray(train_thr, np.int32)
        check(lib().orb_hamming_topk(self._ctx.h, _p(q), nq, _p(t), len(t), _p(co), _p(cx), _p(th), k,
                                     _p(dist), _p(idx), _p(nv)), "orb_hamming_topk")
        return dist, idx, nv

    def SearchByBoW_KF_F(self, desc_kf, angle_kf, mp_kf, featvec_kf, desc_f, angle_f, featvec_f):
        """SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (ORBmatcher.cc:159-288).
        Returns (nmatches, match_f) with match_f[iF] = KF feature index or -1."""
        fa, ka = _featvec(featvec_kf)
        fb, kb = _featvec(featvec_f)
        a = [np.ascontiguousarray(x) for x in (desc_kf, np.asarray(angle_kf, np.float32),
                                                np.asarray(mp_kf, np.uint8), desc_f,
                                                np.asarray(angle_f, np.float32))]
        out = np.full(len(a[3]), -1, np.int32)
        nm = ctypes.c_int()
        check(lib().orb_search_by_bow_kf_f(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation), len(a[0]),
                                           _p(a[0]), _p(a[1]), _p(a[2]), fa, len(a[3]), _p(a[3]), _p(a[4]), fb,
                                           _p(out), ctypes.byref(nm)), "SearchByBoW(KF,F)")
        return nm.value, out

    def SearchByBoW_KF_KF(self, desc1, angle1, mp1, featvec1, desc2, angle2, mp2, featvec2):
        """SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (ORBmatcher.cc:522-655)."""
        fa, ka = _featvec(featvec1)
        fb, kb = _featvec(featvec2)
        a = [np.ascontiguousarray(x) for x in (desc1, np.asarray(angle1, np.float32), np.asarray(mp1, np.uint8),
                                                desc2, np.asarray(angle2, np.float32), np.asarray(mp2, np.uint8))]
        out = np.full(len(a[0]), -1, np.int32)
        nm = ctypes.c_int()
        check(lib().orb_search_by_bow_kf_kf(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation), len(a[0]),
                                            _p(a[0]), _p(a[1]), _p(a[2]), fa, len(a[3]), _p(a[3]), _p(a[4]),
                                            _p(a[5]), fb, _p(out), ctypes.byref(nm)), "SearchByBoW(KF,KF)")
        return nm.value, out

    def _bow_entries(self, kfs, nout):
        """(ctypes array of orb_bow_kf, outputs, counts, keepalive) for dicts {desc, angle, mp, featvec}."""
        from ._lib import OrbBowKf
        arr, outs, counts, keep = (OrbBowKf * max(len(kfs), 1))(), [], [], []
        for p, k in enumerate(kfs):
            f, kf = _featvec(k["featvec"])
            a = [np.ascontiguousarray(x) for x in (k["desc"], np.asarray(k["angle"], np.float32),
                                                    np.asarray(k["mp"], np.uint8))]
            out = np.full(max(nout, 1), -1, np.int32)
            n = ctypes.c_int()
            keep += [kf, a, out, n]
            outs.append(out[:nout])
            counts.append(n)
            arr[p] = OrbBowKf(len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), f, _p(out), ctypes.pointer(n))
        return arr, outs, counts, keep

    def SearchByBoW_KF_F_batch(self, kfs, desc_f, angle_f, featvec_f):
        """orb_search_by_bow_kf_f_batch: SearchByBoW(pKF, F) for every keyframe of kfs (dicts with desc, angle, mp,
        featvec) in one call (Tracking::Relocalization's candidate loop, Tracking.cc:1931-1938).  Returns a list of
        (nmatches, match_f), each equal to SearchByBoW_KF_F's."""
        fb, kb = _featvec(featvec_f)
        d = np.ascontiguousarray(desc_f)
        ang = np.ascontiguousarray(angle_f, np.float32)
        arr, outs, counts, keep = self._bow_entries(kfs, len(d))
        check(lib().orb_search_by_bow_kf_f_batch(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation), len(d),
                                                 _p(d), _p(ang), fb, len(kfs), ctypes.cast(arr, ctypes.c_void_p)),
              "SearchByBoW(KF,F) batch")
        return [(n.value, o) for n, o in zip(counts, outs)]

    def SearchByBoW_KF_KF_batch(self, desc1, angle1, mp1, featvec1, kf2s):
        """orb_search_by_bow_kf_kf_batch: SearchByBoW(KF1, pKF2) for every KF2 of kf2s (dicts with desc, angle, mp,
        featvec) in one call (LoopClosing::ComputeSim3's candidate loop, LoopClosing.cc:252-265).  Returns a list
        of (nmatches, match12), each equal to SearchByBoW_KF_KF's."""
        fa, ka = _featvec(featvec1)
        a = [np.ascontiguousarray(x) for x in (desc1, np.asarray(angle1, np.float32), np.asarray(mp1, np.uint8))]
        arr, outs, counts, keep = self._bow_entries(kf2s, len(a[0]))
        check(lib().orb_search_by_bow_kf_kf_batch(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation),
                                                  len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), fa, len(kf2s),
                                                  ctypes.cast(arr, ctypes.c_void_p)), "SearchByBoW(KF,KF) batch")
        return [(n.value, o) for n, o in zip(counts, outs)]

    def SearchForTriangulation(self, desc1, kps1, has_mp1, uright1, featvec1, desc2, kps2, has_mp2, uright2,
                               featvec2, F12, ex, ey, scale_factors2, level_sigma2_2, bOnlyStereo=False):
        """SearchForTriangulation (ORBmatcher.cc:657-823). Returns an (n, 2) array of (idx1, idx2)."""
        fa, ka = _featvec(featvec1)
        fb, kb = _featvec(featvec2)
        a = [np.ascontiguousarray(x) for x in (desc1, np.asarray(kps1, KP_DTYPE), np.asarray(has_mp1, np.uint8),
                                                np.asarray(uright1, np.float32), desc2, np.asarray(kps2, KP_DTYPE),
                                                np.asarray(has_mp2, np.uint8), np.asarray(uright2, np.float32),
                                                np.asarray(F12, np.float32).reshape(9),
                                                np.asarray(scale_factors2, np.float32),
                                                np.asarray(level_sigma2_2, np.float32))]
        cap = len(a[0]) + 1
        pairs = np.zeros((cap, 2), np.int32)
        n = ctypes.c_int()
        check(lib().orb_search_for_triangulation(self._ctx.h, int(self.mbCheckOrientation), int(bOnlyStereo),
                                                 len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), fa, len(a[4]),
                                                 _p(a[4]), _p(a[5]), _p(a[6]), _p(a[7]), fb, _p(a[8]), ex, ey,
                                                 _p(a[9]), _p(a[10]), len(a[9]), _p(pairs), cap, ctypes.byref(n)),
              "SearchForTriangulation")
        return pairs[:n.value]

    def SearchForTriangulationBatch(self, desc1, kps1, has_mp1, uright1, featvec1, others, bOnlyStereo=False):
        """orb_search_for_triangulation_batch: KF1 against several KF2s in one call (LocalMapping.cc:247-278's
        loop).  others: a list of dicts with the single call's KF2 arguments (desc2, kps2, has_mp2, uright2,
        featvec2, F12, ex, ey, scale_factors2, level_sigma2_2).  Returns one (n, 2) array per KF2, each equal to
        SearchForTriangulation's for the same inputs."""
        from ._lib import OrbTriPair
        fa, ka = _featvec(featvec1)
        a = [np.ascontiguousarray(x) for x in (desc1, np.asarray(kps1, KP_DTYPE), np.asarray(has_mp1, np.uint8),
                                                np.asarray(uright1, np.float32))]
        keep, arr, outs, counts = [ka, a], (OrbTriPair * max(len(others), 1))(), [], []
        for p, o in enumerate(others):
            fb, kb = _featvec(o["featvec2"])
            b = [np.ascontiguousarray(x) for x in (o["desc2"], np.asarray(o["kps2"], KP_DTYPE),
                                                    np.asarray(o["has_mp2"], np.uint8), np.asarray(o["uright2"], np.float32),
                                                    np.asarray(o["F12"], np.float32).reshape(9),
                                                    np.asarray(o["scale_factors2"], np.float32),
                                                    np.asarray(o["level_sigma2_2"], np.float32))]
            cap = len(a[0]) + 1
            out = np.zeros((cap, 2), np.int32)
            n = ctypes.c_int()
            keep += [kb, b, out, n]
            outs.append(out)
            counts.append(n)
            arr[p] = OrbTriPair(len(b[0]), _p(b[0]), _p(b[1]), _p(b[2]), _p(b[3]), fb, _p(b[4]), float(o["ex"]),
                                float(o["ey"]), _p(b[5]), _p(b[6]), len(b[5]), _p(out), cap, ctypes.pointer(n))
        check(lib().orb_search_for_triangulation_batch(self._ctx.h, int(self.mbCheckOrientation), int(bOnlyStereo),
                                                       len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), fa,
                                                       len(others), ctypes.cast(arr, ctypes.c_void_p)),
              "SearchForTriangulationBatch")
        return [out[:n.value] for out, n in zip(outs, counts)]

    def SearchForTriangulationFrames(self, frame1, has_mp1, others, bOnlyStereo=False, cap=None):
        """orb_search_for_triangulation_frames: SearchForTriangulationBatch between Frame handles that carry BoW
        (compute_bow / set_featvec) and uright.  others: a list of dicts with frame2, has_mp2, F12, ex, ey,
        scale_factors2, level_sigma2_2.  Returns one (n, 2) array per KF2.  cap: the pair capacity per KF2 (default
        len(frame1) + 1; a smaller one raises ORB_ERR_CAPACITY as the C call does)."""
        from ._lib import OrbTriFramePair
        m1 = np.ascontiguousarray(has_mp1, np.uint8)
        assert len(m1) == len(frame1)
        cap = len(frame1) + 1 if cap is None else int(cap)
        keep, arr, outs, counts = [m1], (OrbTriFramePair * max(len(others), 1))(), [], []
        for p, o in enumerate(others):
            b = [np.ascontiguousarray(x) for x in (np.asarray(o["has_mp2"], np.uint8),
                                                    np.asarray(o["F12"], np.float32).reshape(9),
                                                    np.asarray(o["scale_factors2"], np.float32),
                                                    np.asarray(o["level_sigma2_2"], np.float32))]
            assert len(b[0]) == len(o["frame2"])
            out = np.zeros((max(cap, 1), 2), np.int32)
            n = ctypes.c_int()
            keep += [b, out, n]
            outs.append(out)
            counts.append(n)
            arr[p] = OrbTriFramePair(o["frame2"].h, _p(b[0]), _p(b[1]), float(o["ex"]), float(o["ey"]), _p(b[2]), _p(b[3]),
                                     len(b[2]), _p(out), cap, ctypes.pointer(n))
        self.last_tri_counts = counts
        check(lib().orb_search_for_triangulation_frames(self._ctx.h, int(self.mbCheckOrientation), int(bOnlyStereo),
                                                        frame1.h, _p(m1), len(others), ctypes.cast(arr, ctypes.c_void_p)),
              "SearchForTriangulationFrames")
        return [out[:n.value] for out, n in zip(outs, counts)]

    def SearchByBoW_Frames_KF_F(self, kfs, frame_f):
        """orb_search_by_bow_frames_kf_f: SearchByBoW(pKF, F) for every keyframe of kfs (dicts with frame, mp) against
        the Frame handle frame_f; all handles carry BoW.  Returns a list of (nmatches, match_f)."""
        from ._lib import OrbBowFrameKf
        nf = len(frame_f)
        arr, outs, counts, keep = (OrbBowFrameKf * max(len(kfs), 1))(), [], [], []
        for p, k in enumerate(kfs):
            mp = np.ascontiguousarray(k["mp"], np.uint8)
            assert len(mp) == len(k["frame"])
            out = np.full(max(nf, 1), -1, np.int32)
            n = ctypes.c_int()
            keep += [mp, out, n]
            outs.append(out[:nf])
            counts.append(n)
            arr[p] = OrbBowFrameKf(k["frame"].h, _p(mp), _p(out), ctypes.pointer(n))
        check(lib().orb_search_by_bow_frames_kf_f(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation), frame_f.h,
                                                  len(kfs), ctypes.cast(arr, ctypes.c_void_p)), "SearchByBoW(KF,F) frames")
        return [(n.value, o) for n, o in zip(counts, outs)]

    def SearchByBoW_Frames_KF_KF(self, kf1, mp1, kf2, mp2):
        """orb_search_by_bow_frames_kf_kf: SearchByBoW(pKF1, pKF2) between two Frame handles that carry BoW.  Returns
        (nmatches, match12)."""
        a = [np.ascontiguousarray(x, np.uint8) for x in (mp1, mp2)]
        assert len(a[0]) == len(kf1) and len(a[1]) == len(kf2)
        out = np.full(max(len(kf1), 1), -1, np.int32)
        nm = ctypes.c_int()
        check(lib().orb_search_by_bow_frames_kf_kf(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation), kf1.h,
                                                   _p(a[0]), kf2.h, _p(a[1]), _p(out), ctypes.byref(nm)),
              "SearchByBoW(KF,KF) frames")
        return nm.value, out[:len(kf1)]

    def _window(self, level0_only, desc1, kps1, desc2, kps2, cand_off, cand_idx):
        a = [np.ascontiguousarray(x) for x in (desc1, np.asarray(kps1, KP_DTYPE), desc2, np.asarray(kps2, KP_DTYPE),
                                                np.asarray(cand_off, np.int32), np.asarray(cand_idx, np.int32))]
        if len(a[5]) == 0:
            a[5] = np.zeros(1, np.int32)
        out = np.full(len(a[0]), -1, np.int32)
        nm = ctypes.c_int()
        check(lib().orb_window_match(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation), int(level0_only),
                                     len(a[0]), _p(a[0]), _p(a[1]), len(a[2]), _p(a[2]), _p(a[3]), _p(a[4]),
                                     _p(a[5]), _p(out), ctypes.byref(nm)), "window match")
        return nm.value, out

    def window_match_grid(self, level0_only, desc1, kps1, desc2=None, kps2=None, grid=None, window=None, centres=None,
                          min_xy=(0.0, 0.0), frame=None):
        """orb_window_match_grid: the window searches with GetFeaturesInArea on the device over F2's grid
        (frame_grid(...)); centres: (n1, 2) float32 window centres or None = kps1 positions.  frame: F2 as a
        resident Frame (orb_window_match_frame; desc2, kps2 and grid are then not read)."""
        cen = None if centres is None else np.ascontiguousarray(centres, np.float32).reshape(-1, 2)
        assert window is not None, "window_match_grid: window"
        assert (frame is None) != (desc2 is None and kps2 is None and grid is None), \
            "window_match_grid: give F2 as desc2, kps2 and grid, or as frame=, not both"
        if frame is not None:
            d1, k1 = np.ascontiguousarray(desc1), np.ascontiguousarray(np.asarray(kps1, KP_DTYPE))
            out = np.full(max(len(d1), 1), -1, np.int32)
            nm = ctypes.c_int()
            check(lib().orb_window_match_frame(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation),
                                               int(level0_only), len(d1), _p(d1), _p(k1), _p(cen), float(window),
                                               frame.h, _p(out), ctypes.byref(nm)), "window match (frame)")
            return nm.value, out[:len(d1)]
        a = [np.ascontiguousarray(x) for x in (desc1, np.asarray(kps1, KP_DTYPE), desc2, np.asarray(kps2, KP_DTYPE))]
        g, _grid_arrays = _frame_grid_arg(grid, min_xy)
        out = np.full(max(len(a[0]), 1), -1, np.int32)
        nm = ctypes.c_int()
        check(lib().orb_window_match_grid(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation), int(level0_only),
                                          len(a[0]), _p(a[0]), _p(a[1]), _p(cen), float(window), len(a[2]), _p(a[2]),
                                          _p(a[3]), g, _p(out), ctypes.byref(nm)), "window match (grid)")
        return nm.value, out[:len(a[0])]

    def search_by_projection(self, mode, queries, qdesc, tdesc=None, kps_t=None, grid=None, t_uright=None,
                             t_taken=None, min_xy=(0.0, 0.0), max_dist=TH_HIGH, frame=None, use_uright=False):
        """orb_search_by_projection: the projection-gated searches' core.  queries: PROJ_QUERY_DTYPE array (one per
        projected map point) with descriptors qdesc; trains tdesc / kps_t with their grid (frame_grid(...)),
        t_uright (mvuRight; None = no stereo gate) and t_taken (mvpMapPoints[t] && Observations() > 0; None = none).
        Returns (nmatches, match_t): match_t[t] = the last query assigned to train t, -1 = untouched, -2 = reset
        by the rotation cull.  frame: the trains as a resident Frame (orb_search_by_projection_frame) in place of
        tdesc, kps_t, grid, min_xy and t_uright; use_uright then says whether the stereo gate reads the Frame's own
        uright (it is not read without frame=)."""
        assert (frame is None) != (tdesc is None and kps_t is None and grid is None and t_uright is None), \
            "search_by_projection: give the trains as tdesc, kps_t, grid (and t_uright), or as frame=, not both"
        qa = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE)
        qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        if frame is not None:
            assert len(qa) == len(qd)
            tk = None if t_taken is None else np.ascontiguousarray(t_taken, np.uint8)
            assert tk is None or len(tk) == len(frame)
            out = np.full(max(len(frame), 1), -1, np.int32)
            nm = ctypes.c_int()
            check(lib().orb_search_by_projection_frame(self._ctx.h, int(mode), self.mfNNratio,
                                                       int(self.mbCheckOrientation), int(max_dist), len(qa), _p(qa),
                                                       _p(qd), frame.h, _p(tk),
                                                       int(bool(use_uright)), _p(out),
                                                       ctypes.byref(nm)), "orb_search_by_projection_frame")
            return nm.value, out[:len(frame)]
        td = np.ascontiguousarray(tdesc, np.uint8).reshape(-1, 32)
        kt = np.ascontiguousarray(kps_t, KP_DTYPE)
        assert len(qa) == len(qd) and len(td) == len(kt)
        ur = None if t_uright is None else np.ascontiguousarray(t_uright, np.float32)
        tk = None if t_taken is None else np.ascontiguousarray(t_taken, np.uint8)
        assert (ur is None or len(ur) == len(kt)) and (tk is None or len(tk) == len(kt))
        g, _grid_arrays = _frame_grid_arg(grid, min_xy)
        out = np.full(max(len(kt), 1), -1, np.int32)
        nm = ctypes.c_int()
        check(lib().orb_search_by_projection(self._ctx.h, int(mode), self.mfNNratio, int(self.mbCheckOrientation),
                                             int(max_dist), len(qa), _p(qa), _p(qd), len(kt), _p(td), _p(kt), _p(ur),
                                             _p(tk), g, _p(out), ctypes.byref(nm)), "orb_search_by_projection")
        return nm.value, out[:len(kt)]

    def SearchByProjection_CF_LF(self, u, v, invzc, octave, angle, observed, desc_mp, scale_factors, mbf, th, bMono,
                                 desc_cf=None, kps_cf=None, grid_cf=None, uright_cf=None, taken_cf=None,
                                 min_xy=(0.0, 0.0), bForward=False, bBackward=False, frame=None):
        """SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (ORBmatcher.cc:1328-1470).
        Per LastFrame map point the search keeps (the caller drops outliers, invzc < 0 and projections out of
        bounds, :1355-1376): its projection (u, v) and invzc, LastFrame.mvKeys[i].octave, mvKeysUn[i].angle,
        Observations() > 0 and descriptor.  bForward / bBackward as :1348-1349 (ignored when bMono).  The
        CurrentFrame side: mDescriptors, mvKeysUn, its grid, mvuRight, and which mvpMapPoints are observed.
        Returns (nmatches, match_cf)."""
        f32 = np.float32
        u, v, invzc = (np.asarray(a, f32) for a in (u, v, invzc))
        octave = np.asarray(octave, np.int32)
        q = np.zeros(len(u), PROJ_QUERY_DTYPE)
        q["u"], q["v"] = u, v
        q["r"] = f32(th) * np.asarray(scale_factors, f32)[octave]          # :1381
        if bForward and not bMono:                                        # :1385-1390
            q["min_level"], q["max_level"] = octave, -1
        elif bBackward and not bMono:
            q["min_level"], q["max_level"] = 0, octave
        else:
            q["min_level"], q["max_level"] = octave - 1, octave + 1
        q["ur"] = u - f32(mbf) * invzc                                     # :1409
        q["ur_tol"] = q["r"]
        q["angle"] = np.asarray(angle, f32)
        q["blocks"] = np.asarray(observed, bool)
        return self.search_by_projection(PROJ_BEST, q, desc_mp, desc_cf, kps_cf, grid_cf, uright_cf, taken_cf, min_xy,
                                         frame=frame, use_uright=frame is not None and frame.has_uright)

    def SearchByProjection_F_MapPoints(self, proj_x, proj_y, proj_xr, level, view_cos, desc_mp, scale_factors, th,
                                       desc_f=None, kps_f=None, grid_f=None, uright_f=None, taken_f=None,
                                       min_xy=(0.0, 0.0), frame=None):
        """SearchByProjection(Frame& F, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-129).  Per map point with
        mbTrackInView && !isBad() (:54-58, filtered by the caller): mTrackProjX / Y / XR, mnTrackScaleLevel,
        mTrackViewCos and its descriptor.  Returns (nmatches, match_f)."""
        f32 = np.float32
        level = np.asarray(level, np.int32)
        q = np.zeros(len(level), PROJ_QUERY_DTYPE)
        q["u"], q["v"] = np.asarray(proj_x, f32), np.asarray(proj_y, f32)
        r = np.where(np.asarray(view_cos, f32).astype(np.float64) > 0.998, f32(2.5), f32(4.0)).astype(f32)   # :131-137
        if f32(th) != 1.0:                                                 # :49, :65-66
            r = r * f32(th)
        q["r"] = r * np.asarray(scale_factors, f32)[level]                 # :69
        q["min_level"], q["max_level"] = level - 1, level
        q["ur"] = np.asarray(proj_xr, f32)
        q["ur_tol"] = q["r"]                                               # :94
        q["blocks"] = 1
        return self.search_by_projection(PROJ_RATIO_SAME_LEVEL, q, desc_mp, desc_f, kps_f, grid_f, uright_f, taken_f,
                                         min_xy, frame=frame, use_uright=frame is not None and frame.has_uright)

    def SearchByProjectionBird(self, pt_x, pt_y, desc_mp, r, desc_bird=None, kps_bird=None, grid_bird=None,
                               taken_bird=None, frame=None):
        """SearchByProjectionBird(Frame& F, const vector<MapPointBird*>&, r) (ORBmatcher.cc:1923-1998).  Per birdview
        map point the search keeps (:1933-1943, filtered by the caller): its birdview projection pt and descriptor;
        the Frame's mDescriptorsBird, mvKeysBird, birdview grid.  Returns (nmatches, match_bird)."""
        q = np.zeros(len(pt_x), PROJ_QUERY_DTYPE)
        q["u"], q["v"] = np.asarray(pt_x, np.float32), np.asarray(pt_y, np.float32)
        q["r"] = np.float32(r)
        q["min_level"], q["max_level"] = -1, -1                            # GetFeaturesInAreaBirdview's defaults
        q["blocks"] = 1
        return self.search_by_projection(PROJ_RATIO_SAME_LEVEL, q, desc_mp, desc_bird, kps_bird, grid_bird, None,
                                         taken_bird, frame=frame)

    def SearchByMatchBird(self, index, pt_x, pt_y, angle, desc_mp, r, desc_bird=None, kps_bird=None, grid_bird=None,
                          max_dist=TH_HIGH, frame=None):
        """SearchByMatchBird(KeyFrame* pKF, Frame& F, vector<MapPointBird*>&, r) (ORBmatcher.cc:2000-2114).  Per
        birdview keypoint k of the keyframe with a MapPointBird (the caller leaves the others out): index = k,
        pKF->mvKeysBird[k].pt and .angle, the map point's descriptor; the Frame's mDescriptorsBird, mvKeysBird and
        birdview grid.  Returns (nmatches, match_bird): match_bird[t] = the k whose map point feature t now holds,
        -1 = untouched, -2 = reset by the rotation cull; nmatches is the reference's return value."""
        ids = np.ascontiguousarray(index, np.int32)
        xy = np.ascontiguousarray(np.stack([np.asarray(pt_x, np.float32), np.asarray(pt_y, np.float32)], 1))
        ang = np.ascontiguousarray(angle, np.float32)
        qd = np.ascontiguousarray(desc_mp, np.uint8).reshape(-1, 32)
        if frame is not None:   # the Frame's birdview side as a resident Frame (orb_search_by_match_bird_resident)
            assert len(ids) == len(xy) == len(ang) == len(qd)
            out = np.full(max(len(frame), 1), -1, np.int32)
            nm = ctypes.c_int()
            check(lib().orb_search_by_match_bird_resident(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation),
                                                          int(max_dist), float(r), len(qd), _p(ids), _p(xy), _p(ang),
                                                          _p(qd), frame.h, _p(out), ctypes.byref(nm)),
                  "orb_search_by_match_bird_resident")
            return nm.value, out[:len(frame)]
        td = np.ascontiguousarray(desc_bird, np.uint8).reshape(-1, 32)
        kt = np.ascontiguousarray(kps_bird, KP_DTYPE)
        assert len(ids) == len(xy) == len(ang) == len(qd) and len(td) == len(kt)
        g, _grid_arrays = _frame_grid_arg(grid_bird)
        out = np.full(max(len(kt), 1), -1, np.int32)
        nm = ctypes.c_int()
        check(lib().orb_search_by_match_bird(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation), int(max_dist),
                                             float(r), len(qd), _p(ids), _p(xy), _p(ang), _p(qd), len(kt), _p(td),
                                             _p(kt), g, _p(out), ctypes.byref(nm)), "orb_search_by_match_bird")
        return nm.value, out[:len(kt)]

    def SearchByMatchBirdFrame(self, desc_last, kps_last, has_mp_last, desc_cur, kps_cur, grid_cur, windowSize):
        """SearchByMatchBird(Frame& CurrentFrame, const Frame& LastFrame, windowSize) (ORBmatcher.cc:1901-1921):
        BirdviewMatch(LastFrame, CurrentFrame) over CurrentFrame's birdview grid, then the carry-over of
        LastFrame.mvpMapPointsBird.  has_mp_last[k] = mvpMapPointsBird[k] != NULL (None: none).  Returns (nmatches,
        match_cur): match_cur[i] = the LastFrame feature whose map point CurrentFrame feature i receives, else -1."""
        dl = np.ascontiguousarray(desc_last, np.uint8).reshape(-1, 32)
        kl = np.ascontiguousarray(kps_last, KP_DTYPE)
        dc = np.ascontiguousarray(desc_cur, np.uint8).reshape(-1, 32)
        kc = np.ascontiguousarray(kps_cur, KP_DTYPE)
        mp = None if has_mp_last is None else np.ascontiguousarray(has_mp_last, np.uint8)
        assert len(dl) == len(kl) and len(dc) == len(kc) and (mp is None or len(mp) == len(kl))
        g, _grid_arrays = _frame_grid_arg(grid_cur)
        out = np.full(max(len(kc), 1), -1, np.int32)
        nm = ctypes.c_int()
        check(lib().orb_search_by_match_bird_frame(self._ctx.h, self.mfNNratio, int(self.mbCheckOrientation),
                                                   float(windowSize), len(kl), _p(dl), _p(kl), _p(mp), len(kc),
                                                   _p(dc), _p(kc), g, _p(out), ctypes.byref(nm)),
              "orb_search_by_match_bird_frame")
        return nm.value, out[:len(kc)]

    project_best_host = staticmethod(project_best_host)

    def project_best_batch(self, gate, targets):
        """orb_project_best_batch: the per-query searches (Fuse, SearchBySim3) of many targets in one GPU call.
        targets: dicts with q (PROJ_QUERY_DTYPE; proj_queries(...)), qdesc, tdesc, kps_t, grid (frame_grid(...)) and
        optionally min_xy, t_uright, inv_sigma2 (gate PROJ_GATE_FUSE needs inv_sigma2); or, for every target, frame (a
        resident Frame) in place of tdesc, kps_t, grid, min_xy and t_uright (orb_project_best_frames).  Returns per target
        (best_idx, best_dist): the train with the smallest distance (first in GetFeaturesInArea order on ties) among
        the candidates that pass the level filter and the gate, -1 / -1 where none does."""
        if targets and all(t.get("frame") is not None for t in targets):   # every target's trains resident
            T = _ProjFrameTargets(targets)
            check(lib().orb_project_best_frames(self._ctx.h, int(gate), len(targets), ctypes.addressof(T.arr)),
                  "orb_project_best_frames")
            return T.out
        T = _ProjTargets(targets)
        check(lib().orb_project_best_batch(self._ctx.h, int(gate), len(targets), ctypes.addressof(T.arr)),
              "orb_project_best_batch")
        return T.out

    def SearchLocalPoints(self, points, cam, ids, frame, th=1.0, view_cos_limit=0.5, taken=None, use_uright=False,
                          want_proj=True):
        """orb_search_local_points: Tracking::SearchLocalPoints' isInFrustum loop (view_cos_limit 0.5, Tracking.cc:1641)
        and SearchByProjection(Frame&, vector<MapPoint*>, th) over resident map points (a MapPoints, the slots ids) and
        a resident Frame, in one call.  Returns (match_t, nmatches, proj): match_t[t] = the position in ids of the point
        assigned to feature t (-1: none), proj = the POINT_PROJ_DTYPE records (None without want_proj)."""
        ids = np.ascontiguousarray(ids, np.int32).ravel()
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        assert tk is None or len(tk) == len(frame)
        match_t = np.full(max(len(frame), 1), -1, np.int32)
        proj = np.zeros(len(ids), POINT_PROJ_DTYPE) if want_proj else None
        nm = ctypes.c_int(0)
        check(lib().orb_search_local_points(self._ctx.h, points.h, ctypes.byref(cam), float(view_cos_limit), float(th),
                                            self.mfNNratio, len(ids), _p(ids) if len(ids) else None, frame.h, _p(tk),
                                            int(bool(use_uright)), _p(match_t), ctypes.byref(nm), _p(proj)),
              "orb_search_local_points")
        return match_t[:len(frame)], nm.value, proj

    def FuseSearchPoints(self, points, targets, want_proj=True):
        """orb_fuse_search_points: the projection and search of Fuse(KeyFrame*, vector<MapPoint*>, th) for many target
        keyframes in one call, over resident map points.  targets: dicts with camera (camera(...)), frame (a Frame),
        inv_sigma2 (mvInvLevelSigma2), th and ids.  Returns per target (best_idx, best_dist, proj)."""
        arr = (OrbFusePointsTarget * max(len(targets), 1))()
        keep, out = [], []
        for k, t in enumerate(targets):
            ids = np.ascontiguousarray(t["ids"], np.int32).ravel()
            inv = np.ascontiguousarray(t["inv_sigma2"], np.float32)
            n = len(ids)
            bi, bd = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32)
            proj = np.zeros(max(n, 1), POINT_PROJ_DTYPE) if want_proj else None
            arr[k] = OrbFusePointsTarget(t["camera"], t["frame"].h, _p(inv), float(t["th"]), n, _p(ids), _p(bi), _p(bd),
                                         _p(proj))
            keep.append((ids, inv, t["frame"]))
            out.append((bi[:n], bd[:n], None if proj is None else proj[:n]))
        check(lib().orb_fuse_search_points(self._ctx.h, points.h, len(targets), ctypes.addressof(arr)),
              "orb_fuse_search_points")
        return out

    def Fuse(self, targets):
        """The search of Fuse(KeyFrame* pKF, const vector<MapPoint*>&, th) (ORBmatcher.cc:823-975) for every target
        keyframe of LocalMapping::SearchInNeighbors in one call.  targets: (kf, pts) pairs; kf = dict(desc
        (mDescriptors), kps (mvKeysUn), grid, min_xy, uright (mvuRight), inv_sigma2 (mvInvLevelSigma2)); pts = the
        points left after the tests of :846-885, dict(u, v, ur (:863-870), level (nPredictedLevel), radius (:890),
        desc).  Returns per target (bestIdx, bestDist) per point; bestDist <= TH_LOW and the graph updates of
        :952-971 are the caller's (INTEGRATION.md has the replay rule)."""
        return self.project_best_batch(PROJ_GATE_FUSE, [_kf_target(kf, pts) for kf, pts in targets])

    def Fuse_Scw(self, targets):
        """The search of Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>&, th, vpReplacePoint)
        (ORBmatcher.cc:977-1100) for every corrected keyframe of LoopClosing::SearchAndFuse in one call: as Fuse,
        without the reprojection gate (ur, uright and inv_sigma2 are not read)."""
        return self.project_best_batch(PROJ_GATE_NONE, [_kf_target(kf, pts) for kf, pts in targets])

    def SearchBySim3(self, kf1, kf2, pts1in2, pts2in1):
        """SearchBySim3 (ORBmatcher.cc:1102-1326).  pts1in2: KF1's map points projected into KF2 that pass
        :1150-1183 and are not already matched: dict(index (i1), u, v, level, radius, desc); pts2in1 likewise with
        index = i2.  Both directions are one GPU call.  Returns (nFound, vnMatch12): vnMatch12[i1] = the KF2
        feature both directions agree on, else -1."""
        (b1, d1), (b2, d2) = self.project_best_batch(PROJ_GATE_NONE, [_kf_target(kf2, pts1in2), _kf_target(kf1, pts2in1)])
        n1, n2 = (len(k["frame"]) if k.get("frame") is not None else len(k["kps"]) for k in (kf1, kf2))
        vn1, vn2 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
        ok1, ok2 = (b1 >= 0) & (d1 <= TH_HIGH), (b2 >= 0) & (d2 <= TH_HIGH)      # :1221, :1301
        vn1[np.asarray(pts1in2["index"], np.int64)[ok1]] = b1[ok1]
        vn2[np.asarray(pts2in1["index"], np.int64)[ok2]] = b2[ok2]
        out = np.full(n1, -1, np.int32)
        for i1 in range(n1):                                                    # :1308-1323
            idx2 = vn1[i1]
            if idx2 >= 0 and vn2[idx2] == i1:
                out[i1] = idx2
        return int((out >= 0).sum()), out

    def SearchByProjection_KF_Scw(self, pts, kf, matched):
        """SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vpMatched, th)
        (ORBmatcher.cc:290-403).  pts: the points left after :317-355: dict(u, v, level, radius, desc); kf: dict(desc,
        kps, grid, min_xy); matched[idx] = vpMatched[idx] != NULL.  Returns (nmatches, match_kf): match_kf[idx] = the
        point now matched to feature idx, -1 where the call matched none."""
        q = proj_queries(pts["u"], pts["v"], pts["radius"], pts["level"])
        m = ORBmatcher(self.mfNNratio, False)
        return m.search_by_projection(PROJ_BEST, q, pts["desc"], kf.get("desc"), kf.get("kps"), kf.get("grid"), None,
                                      matched, kf.get("min_xy", (0.0, 0.0)), max_dist=TH_LOW, frame=kf.get("frame"))

    def SearchByProjection_F_KF(self, pts, frame, has_mp, orb_dist):
        """SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
        (ORBmatcher.cc:1472-1599).  pts: the keyframe's map points left after :1492-1521: dict(u, v, level, radius,
        angle (pKF->mvKeysUn[i].angle), desc); frame: dict(desc, kps, grid, min_xy); has_mp[i2] =
        CurrentFrame.mvpMapPoints[i2] != NULL.  Returns (nmatches, match_f) as search_by_projection does."""
        q = proj_queries(pts["u"], pts["v"], pts["radius"], pts["level"], None, 1, pts["angle"])
        return self.search_by_projection(PROJ_BEST, q, pts["desc"], frame.get("desc"), frame.get("kps"),
                                         frame.get("grid"), None, has_mp, frame.get("min_xy", (0.0, 0.0)),
                                         max_dist=int(orb_dist), frame=frame.get("frame"))

    def SearchForInitialization(self, desc1, kps1, desc2, kps2, cand_off, cand_idx):
        """SearchForInitialization (ORBmatcher.cc:405-520); candidates = F2.GetFeaturesInArea per query.
        Returns (nmatches, vnMatches12)."""
        return self._window(True, desc1, kps1, desc2, kps2, cand_off, cand_idx)

    def ComputeDistinctiveDescriptors(self, descriptor_sets):
        """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307) for a batch of map points:
        descriptor_sets[m] = (n_m, 32) descriptors of point m's observations.  Returns the index of the
        chosen descriptor per point (-1 for an empty set)."""
        sets = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descriptor_sets]
        off = np.zeros(len(sets) + 1, np.int32)
        off[1:] = np.cumsum([len(d) for d in sets])
        allv = np.ascontiguousarray(np.concatenate(sets) if off[-1] else np.zeros((1, 32), np.uint8))
        out = np.zeros(max(len(sets), 1), np.int32)
        check(lib().orb_distinctive_descriptors(self._ctx.h, len(sets), _p(off), _p(allv), _p(out)),
              "orb_distinctive_descriptors")
        return out[:len(sets)]

    def BirdviewMatch(self, desc1, kps1, desc2, kps2, cand_off, cand_idx):
        """BirdviewMatch(const Frame&, const Frame&, vector<int>&, int) (ORBmatcher.cc:1790-1899)."""
        return self._window(False, desc1, kps1, desc2, kps2, cand_off, cand_idx)


class ORBVocabulary:
    """DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (include/ORBVocabulary.h:32) on the GPU:
    loadFromBinaryFile (TemplatedVocabulary.h:1466-1510) and transform(features, BowVector&,
    FeatureVector&, levelsup) (:1139-1210).  BowVector -> {word: value}, FeatureVector -> {node: [i]}."""

    def __init__(self, device=0):
        self._ctx = _Ctx(1000, 1.2, 8, 20, 7, device)
        self.v = None

    def loadFromBinaryFile(self, path):
        if self.v:
            lib().orb_vocab_destroy(self.v)
            self.v = None
        out = ctypes.c_void_p()
        check(lib().orb_vocab_load(self._ctx.h, path.encode(), ctypes.byref(out)), "orb_vocab_load")
        self.v = out
        vals = [ctypes.c_int() for _ in range(6)]
        check(lib().orb_vocab_info(self.v, *[ctypes.byref(x) for x in vals]), "orb_vocab_info")
        self.k, self.L, self.scoring, self.weighting, self.nnodes, self.nwords = [x.value for x in vals]
        return True

    def transform_each(self, desc, levelsup=4):
        """Per-feature (word id, weight, node id levelsup above the leaf)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        w = np.zeros(max(n, 1), np.int32)
        wt = np.zeros(max(n, 1), np.float32)
        nd = np.zeros(max(n, 1), np.uint32)
        check(lib().orb_vocab_transform(self._ctx.h, self.v, _p(d), n, levelsup, _p(w), _p(wt), _p(nd)),
              "orb_vocab_transform")
        return w[:n], wt[:n], nd[:n]

    def bow(self, word, weight, node):
        n = len(word)
        bw = np.zeros(max(n, 1), np.int32)
        bv = np.zeros(max(n, 1), np.float64)
        fn = np.zeros(max(n, 1), np.uint32)
        fo = np.zeros(n + 1, np.int32)
        fi = np.zeros(max(n, 1), np.int32)
        nb, nf = ctypes.c_int(), ctypes.c_int()
        args = [np.ascontiguousarray(word, np.int32), np.ascontiguousarray(weight, np.float32),
                np.ascontiguousarray(node, np.uint32)]
        check(lib().orb_vocab_bow(self.v, n, *[_p(a) for a in args], _p(bw), _p(bv), ctypes.byref(nb), _p(fn),
                                  _p(fo), _p(fi), ctypes.byref(nf)), "orb_vocab_bow")
        bowv = {int(bw[i]): float(bv[i]) for i in range(nb.value)}
        fv = {int(fn[j]): fi[fo[j]:fo[j + 1]].tolist() for j in range(nf.value)}
        return bowv, fv

    def transform(self, desc, levelsup=4):
        """transform(features, BowVector&, FeatureVector&, levelsup) -> (bow, featvec)."""
        return self.bow(*self.transform_each(desc, levelsup))

    def close(self):
        if getattr(self, "v", None):
            lib().orb_vocab_destroy(self.v)
            self.v = None

    def __del__(self):
        self.close()


class BirdORB:
    """cv::ORB as the birdview stream uses it (Frame.cc:329: ORB::create(2000) -> nfeatures 2000,
    scaleFactor 1.2, nlevels 8, edgeThreshold 31, HARRIS_SCORE, patchSize 31, fastThreshold 20),
    plus cornerSubPix and the fused Frame.cc:320-342 sequence, on one MI355X (orb_bird_* C-ABI)."""

    def __init__(self, nfeatures=2000, scaleFactor=1.2, nlevels=8, edgeThreshold=31, fastThreshold=20, device=0,
                 variant=0):
        self.params = OrbBirdParams(nfeatures, scaleFactor, nlevels, edgeThreshold, fastThreshold, device, variant)
        st = ctypes.c_int()
        self.h = lib().orb_bird_create(ctypes.byref(self.params), ctypes.byref(st))
        if not self.h:
            raise OrbError(st.value, "orb_bird_create")
        self.nlevels = nlevels

    def close(self):
        if getattr(self, "h", None):
            lib().orb_bird_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _img(image):
        img = np.asarray(image)
        assert img.dtype == np.uint8 and img.ndim == 2, "CV_8UC1 expected"
        return np.ascontiguousarray(img)

    def detect(self, image, mask=None):
        """cv::ORB::detect(image, keypoints, mask) -> keypoints (KP_DTYPE)."""
        img = self._img(image)
        if img.size == 0:
            return np.zeros(0, KP_DTYPE)
        h, w = img.shape
        m = None if mask is None else self._img(mask)
        cap = 2 * max(self.params.nfeatures, 1) + 256
        while True:
            kps = np.zeros(cap, KP_DTYPE)
            n = ctypes.c_int(0)
            st = lib().orb_bird_detect(self.h, _p(img), w, h, img.strides[0], _p(m), w if m is None else m.strides[0],
                                       _p(kps), cap, ctypes.byref(n))
            if st == -3:
                cap = n.value
                continue
            check(st, "orb_bird_detect")
            return kps[:n.value].copy()

    def compute(self, image, keypoints):
        """cv::ORB::compute(image, keypoints, descriptors) -> (keypoints, descriptors); keypoints are
        border-culled and level-sorted as the reference does in place."""
        img = self._img(image)
        k = np.ascontiguousarray(keypoints, KP_DTYPE).copy()
        if img.size == 0:
            return k, np.zeros((0, 32), np.uint8)
        h, w = img.shape
        desc = np.zeros((max(len(k), 1), 32), np.uint8)
        n = ctypes.c_int(len(k))
        check(lib().orb_bird_compute(self.h, _p(img), w, h, img.strides[0], _p(k) if len(k) else None,
                                     ctypes.byref(n), _p(desc)), "orb_bird_compute")
        return k[:n.value].copy(), desc[:n.value].copy()

    def cornerSubPix(self, image, corners, winSize=(5, 5), maxCount=40, epsilon=0.001):
        img = self._img(image)
        h, w = img.shape
        p = np.ascontiguousarray(corners, np.float32).reshape(-1, 2).copy()
        check(lib().orb_corner_subpix(self.h, _p(img), w, h, img.strides[0], _p(p), len(p), winSize[0], winSize[1],
                                      maxCount, epsilon), "orb_corner_subpix")
        return p

    def extract(self, image, mask=None):
        """Frame.cc:320-342 fused: footprint-masked detect, cornerSubPix(5x5, 40, 0.001), compute."""
        img = self._img(image)
        if img.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        h, w = img.shape
        m = None if mask is None else self._img(mask)
        cap = 2 * max(self.params.nfeatures, 1) + 256
        while True:
            kps = np.zeros(cap, KP_DTYPE)
            desc = np.zeros((cap, 32), np.uint8)
            n = ctypes.c_int(0)
            st = lib().orb_bird_extract(self.h, _p(img), w, h, img.strides[0], _p(m), w if m is None else m.strides[0],
                                        _p(kps), cap, ctypes.byref(n), _p(desc))
            if st == -3:
                cap = n.value
                continue
            check(st, "orb_bird_extract")
            return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_device(self, d_img, w, h, d_mask=None, cap=None):
        """Fused extract on a device-resident image (and mask) — device pointers as ints."""
        cap = cap or 2 * max(self.params.nfeatures, 1) + 256
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = ctypes.c_int(0)
        check(lib().orb_bird_extract_device(self.h, ctypes.c_void_p(d_img), w, h, w,
                                            None if d_mask is None else ctypes.c_void_p(d_mask), w, _p(kps), cap,
                                            ctypes.byref(n), _p(desc)), "orb_bird_extract_device")
        return kps[:n.value], desc[:n.value]

    def _batch(self, n, cap, call, where):
        """Run a batch call into fresh (n, cap) outputs; a frame that does not fit raises cap and repeats."""
        cap = cap or 2 * max(self.params.nfeatures, 1) + 256
        while True:
            kps = np.zeros((max(n, 1), cap), KP_DTYPE)
            desc = np.zeros((max(n, 1), cap, 32), np.uint8)
            counts = np.zeros(max(n, 1), np.int32)
            st = call(_p(kps), _p(desc), cap, _p(counts))
            if st == -3:
                cap = int(counts[:n].max())
                continue
            check(st, where)
            return [(kps[f, :counts[f]].copy(), desc[f, :counts[f]].copy()) for f in range(n)]

    def extract_batch(self, images, masks=None):
        """Frame.cc:320-342 for a list of equally sized images in one call.  masks: None, one array shared by
        all frames, or a list with one mask per frame.  Returns [(keypoints, descriptors)] per frame, each
        what extract(image, mask) returns."""
        imgs = [self._img(i) for i in images]
        n = len(imgs)
        if n == 0:
            return []
        h, w = imgs[0].shape
        assert all(i.shape == (h, w) for i in imgs), "one size per batch"
        if masks is None:
            ms = []
        elif isinstance(masks, (list, tuple)):
            ms = [self._img(m) for m in masks]
        else:
            ms = [self._img(masks)]
        assert all(m.shape == (h, w) for m in ms), "masks have the image size"
        if imgs[0].size == 0:
            return [(np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)) for _ in imgs]
        ip = (ctypes.c_void_p * n)(*[i.ctypes.data for i in imgs])
        mp = (ctypes.c_void_p * max(len(ms), 1))(*[m.ctypes.data for m in ms])
        return self._batch(n, None, lambda k, d, cap, c: lib().orb_bird_extract_batch(
            self.h, n, ip, w, h, w, mp if ms else None, len(ms), w, k, d, cap, c), "orb_bird_extract_batch")

    def extract_batch_device(self, d_imgs, n, w, h, frame_pitch=None, d_masks=None, mask_frame_pitch=0, cap=None,
                             stride=None, mask_stride=None):
        """Batch extract on n device-resident frames (device pointers as ints): frame f at d_imgs + f *
        frame_pitch (default stride * h), its mask at d_masks + f * mask_frame_pitch (0: one shared mask)."""
        stride = stride or w
        mask_stride = mask_stride or w
        frame_pitch = stride * h if frame_pitch is None else frame_pitch
        return self._batch(n, cap, lambda k, d, cp, c: lib().orb_bird_extract_batch_device(
            self.h, n, ctypes.c_void_p(d_imgs), w, h, stride, frame_pitch,
            None if d_masks is None else ctypes.c_void_p(d_masks), mask_stride, mask_frame_pitch, k, d, cp, c),
            "orb_bird_extract_batch_device")

    def batch_group(self, group=0):
        """Frames per post-selection group of the batch calls; group > 0 sets it.  Returns the value in force."""
        return lib().orb_bird_batch_group(self.h, group)

    def debug_candidates(self, level):
        cap = 1 << 16
        while True:
            out = np.zeros(cap, KP_DTYPE)
            n = lib().orb_bird_debug_candidates(self.h, level, _p(out), cap)
            if n >= 0:
                return out[:n]
            if n < -1:
                cap = -n - 1
                continue
            check(n, "orb_bird_debug_candidates")

    def debug_level(self, level):
        w, h = ctypes.c_int(), ctypes.c_int()
        check(lib().orb_bird_debug_level(self.h, level, None, ctypes.byref(w), ctypes.byref(h)), "debug_level")
        out = np.zeros((h.value, w.value), np.uint8)
        check(lib().orb_bird_debug_level(self.h, level, _p(out), ctypes.byref(w), ctypes.byref(h)), "debug_level")
        return out


def cornerSubPix(image, corners, winSize=(5, 5), maxCount=40, epsilon=0.001, device=0):
    """cv::cornerSubPix(image, corners, winSize, Size(-1,-1), TermCriteria(EPS+MAX_ITER, maxCount, epsilon))."""
    b = BirdORB(device=device)
    try:
        return b.cornerSubPix(image, corners, winSize, maxCount, epsilon)
    finally:
        b.close()


def bird_footprint_mask(mask):
    """Frame.cc:320-327: copy of `mask` with the vehicle footprint (+15 px) zeroed (host helper)."""
    m = np.ascontiguousarray(mask, np.uint8).copy()
    h, w = m.shape
    check(lib().orb_bird_footprint_mask(_p(m), w, h, m.strides[0]), "orb_bird_footprint_mask")
    return m


KFDB_RELOC, KFDB_LOOP = 0, 1   # ORB_KFDB_*


def _bow_arrays(words, values=None):
    """A BowVector as (int32 words ascending, float64 values): two arrays, or a {word: value} dict (sorted here)."""
    if values is None:
        items = sorted(dict(words).items())
        words, values = [w for w, _ in items], [v for _, v in items]
    w = np.ascontiguousarray(words, np.int64)
    assert len(w) == 0 or (0 <= w.min() and w.max() < 2 ** 31), "word ids are non-negative int32"
    w, v = np.ascontiguousarray(w, np.int32), np.ascontiguousarray(values, np.float64)
    assert w.ndim == 1 and w.shape == v.shape
    return w, v


def bow_score(words1, values1, words2, values2):
    """ORBVocabulary::score(v1, v2) of an L1 vocabulary (DBoW2 L1Scoring::score, ScoringObject.cpp:23-68): the double.
    Pure host."""
    w1, v1 = _bow_arrays(words1, values1)
    w2, v2 = _bow_arrays(words2, values2)
    out = ctypes.c_double()
    check(lib().orb_bow_score(len(w1), _p(w1), _p(v1), len(w2), _p(w2), _p(v2), ctypes.byref(out)), "orb_bow_score")
    return out.value


class KeyFrameDatabase:
    """ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h:42-70, src/KeyFrameDatabase.cc) with the keyframes'
    BowVectors resident on the GPU (orb_kfdb).  Keyframes are named by the id add() returns (the add sequence: from 0,
    never reused).  BowVectors are (words, values) arrays with words ascending, or {word: value} dicts with values=None.
    Only L1 scoring (the ORB vocabulary's).

    KeyFrameDatabase(ctx_or_matcher) shares that object's context (several databases may); KeyFrameDatabase(device=d)
    owns one.  close() frees the database; close it before its context."""

    def __init__(self, ctx_or_matcher=None, device=0):
        self.h = None
        self._ctx = _Ctx(1000, 1.2, 8, 20, 7, device) if ctx_or_matcher is None else getattr(ctx_or_matcher, "_ctx",
                                                                                           ctx_or_matcher)
        out = ctypes.c_void_p()
        check(lib().orb_kfdb_create(self._ctx.h, ctypes.byref(out)), "orb_kfdb_create")
        self.h = out

    def add(self, words, values=None):
        """KeyFrameDatabase::add (:40-46) -> the keyframe's id."""
        w, v = _bow_arrays(words, values)
        out = ctypes.c_int(-1)
        check(lib().orb_kfdb_add(self._ctx.h, self.h, len(w), _p(w), _p(v), ctypes.byref(out)), "orb_kfdb_add")
        return out.value

    def erase(self, kf_id):
        check(lib().orb_kfdb_erase(self.h, int(kf_id)), "orb_kfdb_erase")

    def clear(self):
        check(lib().orb_kfdb_clear(self.h), "orb_kfdb_clear")

    def __len__(self):
        return lib().orb_kfdb_size(self.h)

    def query(self, words, values=None, exclude=()):
        """The sharing list of a query BowVector -> (ids, common, score, excl_score): the live keyframes outside
        `exclude` that share a word, in the reference's lKFsSharingWords order, their common-word counts and the
        doubles L1Scoring::score(query, keyframe) returns; excl_score[j] is that double for exclude[j] (-0.0: no word
        shared; NaN: erased, not scored)."""
        w, v = _bow_arrays(words, values)
        ex = np.ascontiguousarray(list(exclude), np.int32)
        xs = np.full(max(len(ex), 1), np.nan, np.float64)
        cap = len(self)
        ids, common = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        score = np.zeros(max(cap, 1), np.float64)
        n = ctypes.c_int()
        check(lib().orb_kfdb_query(self._ctx.h, self.h, len(w), _p(w), _p(v), len(ex), _p(ex), _p(xs), cap, _p(ids),
                                   _p(common), _p(score), ctypes.byref(n)), "orb_kfdb_query")
        return ids[:n.value], common[:n.value], score[:n.value], xs[:len(ex)]

    def candidates(self, mode, ids, common, score, neighbours, min_score=0.0):
        """Everything after the sharing list (orb_kfdb_candidates) -> candidate ids.  neighbours(id) returns the ids of
        GetBestCovisibilityKeyFrames(10) of that keyframe, best first (more than 10 are cut to 10)."""
        ids = np.ascontiguousarray(ids, np.int32)
        common = np.ascontiguousarray(common, np.int32)
        score = np.ascontiguousarray(score, np.float64)
        n = len(ids)
        out = np.zeros(max(n, 1), np.int32)
        nc = ctypes.c_int()
        failure = []

        def nb(_user, kf_id, dst, cap):
            try:
                got = [int(x) for x in neighbours(kf_id)][:cap]
            except Exception as e:   # (an exception cannot cross the C frame)
                failure.append(e)
                return -1
            for i, x in enumerate(got):
                dst[i] = x
            return len(got)

        st = lib().orb_kfdb_candidates(self.h, mode, float(min_score), n, _p(ids), _p(common), _p(score),
                                       KfdbNeighboursFn(nb), None, _p(out), ctypes.byref(nc))
        if failure:
            raise failure[0]
        check(st, "orb_kfdb_candidates")
        return out[:nc.value].copy()

    def detect_relocalization_candidates(self, words, values=None, neighbours=lambda kf_id: ()):
        """KeyFrameDatabase::DetectRelocalizationCandidates (:199-309) of a frame's BowVector -> keyframe ids."""
        ids, common, score, _ = self.query(words, values)
        return self.candidates(KFDB_RELOC, ids, common, score, neighbours)

    def detect_loop_candidates(self, words, values=None, connected=(), min_score=0.0, neighbours=lambda kf_id: ()):
        """KeyFrameDatabase::DetectLoopCandidates (:76-197) of a keyframe's BowVector; connected = the ids of
        GetConnectedKeyFrames() -> keyframe ids."""
        ids, common, score, _ = self.query(words, values, connected)
        return self.candidates(KFDB_LOOP, ids, common, score, neighbours, min_score)

    def close(self):
        if getattr(self, "h", None):
            lib().orb_kfdb_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
