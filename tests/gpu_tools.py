"""Helpers of the GPU tests that drive liborbgpu themselves (tests/test_gpu_resize_rows.py,
tests/test_gpu_pyramid_small.py): the pyramid levels of a batched extraction from a device buffer the test lays out,
and which task kinds of the dataflow launch ran."""
import numpy as np

FLOW_RESIZE, FLOW_CHAIN = 0, 4   # FlowKind (orbgpu_internal.h): resize, fast, octree, describe, chain


def flow_task_ends(orbgpu_mod, e, nframes=1):
    """{task kind: latest end stamp} of the dataflow launch's tasks so far (ORBGPU_FLOW_STAMPS=1 at orb_create:
    [ticket, wait over, done, kind | level << 8 | frame << 16 | workgroup << 32] per task; only k_extract_flow writes
    them, and the buffer exists only once a plan for this batch was built).  The buffer is not cleared and is larger
    than the task list: a stamp counts only with a known kind, a level and a frame of the batch; the caller compares two
    launches, since rows no task owns never change."""
    st = np.zeros(1 << 16, np.uint64)
    n = orbgpu_mod._lib.lib().orb_debug_fast_stamps(e.h, st.ctypes.data, len(st))
    assert n > 0, "no dataflow plan was built for this batch: the per-kernel launches ran"
    ends = {}
    for ticket, _, end, ident in st[:n - n % 4].reshape(-1, 4).tolist():
        if ticket and end > ticket and ident & 0xFF <= 4 and (ident >> 8) & 0xFF < 16 and (ident >> 16) & 0xFFFF < nframes:
            ends[ident & 0xFF] = max(ends.get(ident & 0xFF, 0), end)
    return ends


def batch_levels(orbgpu_mod, frames, scale, nlevels, variant, stride, base_off=0, runs=1, after_run=None):
    """Pyramid levels 1.. of every frame after each of `runs` batched extractions (the graph's capture, then replays)
    from a device buffer with row stride `stride` that starts `base_off` bytes into its allocation: [run][frame][l - 1].
    after_run(extractor) is called after each run, before the levels are read."""
    from orbgpu._lib import check, lib
    n, h, w = frames.shape
    e = orbgpu_mod.BatchExtractor(500, w, h, n, scale_factor=scale, nlevels=nlevels, variant=variant)
    padded = np.full((n, h, stride), 0xA5, np.uint8)   # the pad bytes are never read: any value must do
    padded[:, :, :w] = frames
    host = np.full(base_off + padded.nbytes, 0xA5, np.uint8)
    host[base_off:] = padded.reshape(-1)
    d = e._alloc(host.nbytes)
    try:
        check(lib().orb_memcpy_h2d(e.h, d, host.ctypes.data, host.nbytes), "h2d")
        out = []
        for _ in range(runs):
            check(lib().orb_extract_batch_device(e.h, d + base_off, n, w, h, stride * h, stride, e.d_kps, e.d_desc,
                                                 e.d_counts, e.kp_cap), "orb_extract_batch_device")
            e.sync()
            if after_run:
                after_run(e)
            out.append([[e.debug_level_image(l, f) for l in range(1, nlevels)] for f in range(n)])
        return out
    finally:
        lib().orb_device_free(e.h, d)
        e.close()
