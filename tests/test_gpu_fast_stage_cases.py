"""The planted staging frames of tests/fast_stage_cases.py through k_fast_wave / flow_fast: FAST candidates of every
level, keypoints and descriptors equal the oracle's byte for byte.  No tolerance anywhere.

Each size runs as one frame per launch (one cell per wave), as one batch of its planted frames and the noise frame
(two cells per wave: the second cell's ROI is issued before the first is processed), with the per-kernel and the
dataflow launch, and through ORBextractor's operator().  BatchExtractor passes rowStride = width, so the odd widths
(179, 91) take the per-byte store there; operator() uploads into rows of ((w + 63) & ~63) bytes
(csrc/orbgpu_abi.hip, orb_extract: `const size_t pitch = ...` handed to run_extract as row_stride), which makes level
0 dword aligned whatever the width: the same frames then go through both load paths and must give the same bytes.

A failure names the cells and plants that differ, each with its (pitch, B, nruns, round, run, late row) tuple."""
import os
import re

import pytest

import fast_stage_cases as fc

NAMES = list(fc.SIZES)


def _compare(e, geo, planted, frame, slot, per, what, results=None):
    cands, kps, desc = per[frame]
    for l in range(geo.nlevels):
        g = e.debug_candidates(l, slot)
        if g.tobytes() != cands[l].tobytes():      # (a string: pytest prints it whole)
            pytest.fail("%s: FAST candidates differ, frame %d level %d: %d for the oracle's %d\n%s" % (
                what, frame, l, len(g), len(cands[l]),
                "\n".join(fc.explain(geo, planted, frame, l, g, cands[l])) or "the same candidates in another order"))
    gk, gd = results if results is not None else e.results(slot)
    assert len(gk) == len(kps) and gk.tobytes() == kps.tobytes(), (what, "keypoints differ", frame)
    assert gd.tobytes() == desc.tobytes(), (what, "descriptors differ", frame)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_frame_launch_matches_oracle(orbgpu_mod, oracle_mod, name):
    """One frame per launch: one cell per wave."""
    geo, planted, frames, per = fc.expected(oracle_mod, name)
    e = orbgpu_mod.BatchExtractor(fc.NFEAT, geo.w, geo.h, 1, nlevels=geo.nlevels, ini_th=fc.INI_TH, min_th=fc.MIN_TH)
    try:
        for f in range(len(frames)):
            e.upload(frames[f][None])
            e.launch()
            e.sync()
            _compare(e, geo, planted, f, 0, per, (name, "one frame"))
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["kernels", "flow"])
@pytest.mark.parametrize("name", NAMES)
def test_batch_launch_matches_oracle(orbgpu_mod, oracle_mod, monkeypatch, name, launch):
    """The planted frames and the noise frame in one batch: two cells per wave (k_fast_wave), and flow_fast."""
    geo, planted, frames, per = fc.expected(oracle_mod, name)
    monkeypatch.setenv("ORBGPU_FLOW", "1" if launch == "flow" else "0")   # read at orb_create
    e = orbgpu_mod.BatchExtractor(fc.NFEAT, geo.w, geo.h, len(frames), nlevels=geo.nlevels, ini_th=fc.INI_TH,
                                  min_th=fc.MIN_TH)
    try:
        e.upload(frames)
        e.launch()
        e.sync()
        for f in range(len(frames)):
            _compare(e, geo, planted, f, f, per, (name, launch))
    finally:
        e.close()


def test_host_path_pitch_is_dword_aligned():
    """CPU only: the host-image path (extract_host behind orb_extract) uploads into rows of a multiple of 64 bytes and
    passes that pitch as the row stride; its staging function receives that buffer and pitch and uploads with them."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb-slam-birdview_amd",
                            "csrc", "orbgpu_abi.hip")).read()

    def body_of(head):
        body = src[src.index(head):]
        return body[:body.index("\n}\n")]

    assert "return extract_host(c, HostImage{img, w, hgt, stride}," in body_of("int orb_extract(")
    body = body_of("int extract_host(")
    assert re.search(r"const size_t pitch = \(\(size_t\)w \+ 63\) & ~\(size_t\)63;", body)
    assert re.search(r"run_extract\(c->d_in\.get\(\), 1, \(long long\)pitch \* hgt, \(int\)pitch,", body)
    assert "stage_host_image(c, im, w, hgt, c->d_in.get(), pitch," in body
    stage = body_of("static int stage_host_image(Ctx* c, const HostImage& im, int w, int hgt, uint8_t* d_in, size_t pitch,")
    assert "hipMemcpy2DAsync(d_in, pitch, im.data, im.stride, w, hgt" in stage


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_host_path_matches_oracle(orbgpu_mod, oracle_mod, name):
    """ORBextractor's operator(): level 0 aligned at every width (see test_host_path_pitch_is_dword_aligned)."""
    geo, planted, frames, per = fc.expected(oracle_mod, name)
    g = orbgpu_mod.ORBextractor(fc.NFEAT, 1.2, geo.nlevels, fc.INI_TH, fc.MIN_TH)
    try:
        for f in range(len(frames)):
            res = g(frames[f])
            _compare(g, geo, planted, f, 0, per, (name, "operator()"), res)
    finally:
        g.close()
