"""GPU parity of the pyramid that launches of one and two frames take: every level of every frame byte-identical to
the oracle's (OracleExtractor.level), at small sizes and at the alignments and contents where it can go wrong.

Launches
 * host       ORBextractor on a numpy array, packed or a view with row padding: the whole-chain plan from the frame
              (k_pyramid_chain in segments of kChainSeg; per-level launches where build_chain refuses the plan);
 * dev1/dev2  orb_extract_batch_device with 1 / 2 frames from a device buffer whose stride and base the test chooses:
              the small plan (levels 1..kSmallChainBase by k_resize_tiled / k_resize, the rest chained from level 3);
 * flow       the same single frame with ORBGPU_FLOW=1 (flow_resize: resize_tile with sc1 loads and stores);
 * flowchain  and with ORBGPU_FLOW_CHAIN=1 (flow_chain: chain_job with sc1, chain_ld8's aligned dword).
Each launch runs twice (the graph's capture, then a replay).  The sizes, layouts and planted frames are
tests/pyramid_cases.py's; what each size reaches (tilings, one-pixel last columns, one-row last tiles, the byte forms,
KP = 2 / 3 / 0, TH = 16, k_resize, the refused plan) is asserted from the CPU model in
tests/test_pyramid_chain_host.py, which also checks the planted frames on the oracle alone.

The two 8-level sizes run the host and device launches over every layout and both variants.  The dataflow launch
refuses them (its 16 FAST carves do not fit a CU's LDS when a level is one tall cell), so the flow launches run, over
every layout and both variants, on two taller frames of the same level widths (FLOW_EIGHT).  The other sizes run the
launches over the aligned and packed layouts, the flow ones where the dataflow launch takes the geometry (FLOW_OTHER;
an untiled level, UNTILED, leaves only the chain form).  Every configuration runs every content.  The flow cases
record task stamps (ORBGPU_FLOW_STAMPS=1) and assert that the dataflow launch's resize / chain tasks ran in both
runs, so none of them is the per-kernel fallback under another name.  The host launches copy the image into a
64-byte-pitched device buffer whatever the caller's stride, so "padded" tests that upload, not another alignment
form of the kernels."""
import numpy as np
import pytest

from gpu_tools import FLOW_CHAIN, FLOW_RESIZE, batch_levels, flow_task_ends
from pyramid_cases import CHAIN_TOO_LARGE, CONTENTS, EIGHT, FLOW_EIGHT, FLOW_OTHER, GENERIC, LAYOUTS, OTHER, REFUSED, UNTILED, frames, layout

pytestmark = pytest.mark.gpu

DEV = ["dev1", "dev2", "flow", "flowchain"]


def _configs():
    out = []
    for s in EIGHT:
        out += [(s, "host", lay, v) for lay in ("packed", "padded") for v in (0, GENERIC)]
        out += [(s, launch, lay, v) for launch in ("dev1", "dev2") for lay in LAYOUTS for v in (0, GENERIC)]
    for s in FLOW_EIGHT:
        out += [(s, launch, lay, v) for launch in ("flow", "flowchain") for lay in LAYOUTS for v in (0, GENERIC)]
    for s in OTHER:
        out += [(s, "host", "packed", 0), (s, "host", "padded", GENERIC), (s, "dev1", "s64", 0),
                (s, "dev2", "packed", GENERIC)]
        if s in FLOW_OTHER and s not in CHAIN_TOO_LARGE:
            out.append((s, "flowchain", "packed", 0))
        if s in FLOW_OTHER:
            if s not in UNTILED:   # (the chain tasks need no tiled level; build_flow refuses the resize tasks)
                out.append((s, "flow", "s64", GENERIC))
    out += [(REFUSED, "host", "packed", 0), (REFUSED, "host", "padded", GENERIC)]
    return out


def _cases():
    return [pytest.param(s, launch, lay, v, c, id="%dx%d_%g_%d-%s-%s-v%d-%s" % (s + (launch, lay, v, c)))
            for s, launch, lay, v in _configs() for c in CONTENTS]


_REF = {}


def _oracle(oracle_mod, size, content, variant, n):
    """The oracle's levels 1.. of the n frames of one content (computed once, shared by the launches)."""
    key = (size, content, variant, n)
    if key not in _REF:
        w, h, scale, nl = size
        o = oracle_mod.OracleExtractor(500, scale, nl, flags=variant)
        ref = []
        for f in frames(w, h, content, n):
            o(f)
            ref.append([o.level(l).copy() for l in range(1, nl)])
        _REF[key] = ref
    return _REF[key]


@pytest.mark.parametrize("size,launch,lay,variant,content", _cases())
def test_levels_match_the_oracle(orbgpu_mod, oracle_mod, monkeypatch, size, launch, lay, variant, content):
    w, h, scale, nl = size
    n = 2 if launch == "dev2" else 1
    fr = frames(w, h, content, n)
    monkeypatch.setenv("ORBGPU_FLOW", "1" if launch in ("flow", "flowchain") else "0")   # read at orb_create
    monkeypatch.setenv("ORBGPU_FLOW_CHAIN", "1" if launch == "flowchain" else "0")       # read when the plan is built
    if launch == "host":
        img = fr[0]
        if lay == "padded":   # rows 13 bytes apart from packed: the upload's source stride, the kernels see the same buffer
            buf = np.full((h, w + 13), 0xA5, np.uint8)
            buf[:, :w] = img
            img = buf[:, :w]
        e = orbgpu_mod.ORBextractor(500, scale, nl, 20, 7, variant=variant)
        try:
            runs = []
            for _ in range(2):
                e(img)
                runs.append([[e.debug_level_image(l) for l in range(1, nl)]])
        finally:
            e.close()
    else:
        stride, off = layout(w, lay)
        ends = []
        flow = launch in ("flow", "flowchain")
        if flow:
            monkeypatch.setenv("ORBGPU_FLOW_STAMPS", "1")
            monkeypatch.delenv("ORBGPU_FLOW_BLOCKS", raising=False)
        runs = batch_levels(orbgpu_mod, fr, scale, nl, variant, stride, base_off=off, runs=2,
                            after_run=(lambda e: ends.append(flow_task_ends(orbgpu_mod, e))) if flow else None)
        if flow:   # the dataflow launch ran, with the pyramid tasks the case is about, in both runs
            kind = FLOW_CHAIN if launch == "flowchain" else FLOW_RESIZE
            other = FLOW_RESIZE if launch == "flowchain" else FLOW_CHAIN
            assert kind in ends[0] and ends[1][kind] > ends[0][kind], (launch, ends)
            assert ends[1].get(other) == ends[0].get(other), (launch, "tasks of the other pyramid form ran", ends)
    ref = _oracle(oracle_mod, size, content, variant, n)
    for run, got in enumerate(runs):
        for f in range(n):
            for l in range(1, nl):
                g, r = got[f][l - 1], ref[f][l - 1]
                assert g.shape == r.shape, (run, f, l, g.shape, r.shape)
                bad = np.argwhere(g != r)
                assert len(bad) == 0, (run, f, l, len(bad), bad[:4].tolist(), g[tuple(bad[0])], r[tuple(bad[0])])
