"""CPU: the plan, index arithmetic and values of the pyramid that launches of one and two frames take (chain_job of
k_pyramid_chain / flow_chain, resize_tile of k_resize_tiled / flow_resize), without a GPU.

tests/cpp_pyramid_chain/chain_model.cc builds the level sizes, takes the library's coefficient tables (resize_coefs)
and plan (build_chain) and walks every job and tile as the kernels do (see its header for the checks).  It runs over
every size of tests/pyramid_cases.py, both plans (the host path's: segments of kChainSeg from the frame; the small
batches': levels past kSmallChainBase in one segment), both vertical forms and three source alignments.  What the GPU
cases of tests/test_gpu_pyramid_small.py are said to reach is asserted here from the model's output.

What the model shows, beyond "no violation":
 * build_chain refuses a plan by the scale factor and the levels a segment chains, not by the width
   (test_the_plan_is_refused_by_scale_and_depth).
 * packed_ok (a dword group's bytes within 8) holds up to scale factor 2: 1.9 takes the packed form in both kernels,
   2.1 and up the byte form.  resize_tile's byte form needs a level of one tile column (at most 128 wide: the span must
   fit kRsPitch), TH = 16 a scale factor near 2.3 at such a width; both are valid geometries and are in the cases.
 * the third realigned dword reads up to 8 bytes past its region's last row in chain_job (inside sg.lds_bytes: the
   other buffer or the coefficient slots follow) and stays inside rs_span_rows * kRsPitch in resize_tile.
 * the dataflow chain's byte load (chain_ld8 with sc1) loads the aligned dword around its byte: from an odd frame base
   or to an odd end that is up to 3 bytes outside the buffer (ld8_outside), inside the same aligned dword (so the same
   page) as a byte of the buffer.

Then the planted frames of the GPU test, on the oracle alone: what each means, in both vertical forms."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from pyramid_cases import CHAIN_TOO_LARGE, CONTENTS, EIGHT, FLOW_EIGHT, FLOW_OTHER, GENERIC, OTHER, REFUSED, SIZES, UNTILED, frame

HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tests", "cpp_pyramid_chain", "chain_model.cc")
K_CHAIN_SEG, K_SMALL_CHAIN_BASE, MAX_LEVELS = 4, 3, 16   # orbgpu_internal.h, include/orbgpu.h
PLANS = {"host": (0, K_CHAIN_SEG), "small": (K_SMALL_CHAIN_BASE, MAX_LEVELS)}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain") / "chain_model")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-o", exe, SRC,
                           "-L" + PKG, "-lorbgpu", "-Wl,-rpath," + PKG])
    memo = {}

    def run(size, plan="host", generic=0, align=16, edit=None):
        key = (size, plan, generic, align, edit)
        if key not in memo:
            args = [exe] + [str(v) for v in size + PLANS[plan] + (generic, align)] + ([edit] if edit else [])
            memo[key] = subprocess.run(args, capture_output=True, text=True)
        return memo[key]
    return run


def _parse(out):
    """{'levels': [(w, h)], 'valid': bool, 'plan': bool, 'chain': {level: fields}, 'resize': {level: fields}}"""
    r = {"chain": {}, "resize": {}, "seg": [], "plan": False}
    for line in out.splitlines():
        t = line.split()
        if t[0] == "levels":
            r["levels"] = [tuple(int(v) for v in s.split("x")) for s in t[1:]]
        elif t[0] == "valid":
            r["valid"] = t[1] == "1"
        elif t[0] == "fast_wave_bytes":
            r["fwb"] = int(t[1])
        elif t[0] == "plan":
            r["plan"] = True
        elif t[0] == "seg":
            r["seg"].append({t[i]: int(t[i + 1]) for i in range(2, len(t), 2)})
        elif t[0] == "chain":
            d = {t[i]: t[i + 1] for i in range(3, len(t), 2)}
            r["chain"][int(t[2])] = {k: (v if k == "tile" else int(v)) for k, v in d.items()}
        elif t[0] == "resize":
            d = {"kernel": t[4]}
            d.update({t[i]: t[i + 1] for i in range(5, len(t) - 1, 2)})
            r["resize"][int(t[2])] = d
    return r


@pytest.mark.parametrize("align", [16, 4, 1])
@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("plan", ["host", "small"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d_%g_%d" % s)
def test_model_walk_in_bounds_and_exact(model, size, plan, generic, align):
    out = model(size, plan, generic, align)
    assert out.returncode == 0 and out.stdout.strip().endswith("\nok"), (out.stdout[-600:], out.stderr)
    r = _parse(out.stdout)
    assert r["valid"], "not a valid grid at its level count"
    assert len(r["levels"]) == size[3] and len(r["resize"]) == size[3] - 1
    if r["plan"]:   # every level past the plan's first base is some segment's
        first = PLANS[plan][0]
        assert sorted(r["chain"]) == list(range(first + 1, size[3]))


def test_cases_hold_what_their_comments_claim(model):
    res = {(s, p): _parse(model(s, p).stdout) for s in SIZES for p in PLANS}
    host = lambda s: res[(s, "host")]
    # the sizes with a level that no k_resize_tiled takes (the dataflow launch's resize tasks refuse them)
    assert [s for s in SIZES if any(d["kernel"] == "k_resize" for d in host(s)["resize"].values())] == UNTILED
    # the dataflow launch's FAST carves (16 waves) fit a CU's LDS at the flow cases' sizes, and at no other
    fits = lambda s: 16 * host(s)["fwb"] <= 160 * 1024 - 64
    assert [s for s in OTHER if fits(s)] == FLOW_OTHER and all(fits(s) for s in FLOW_EIGHT) and not any(fits(s) for s in EIGHT)
    big = lambda s: any(4 * (((sg["lds_bytes"] + 15) & ~15) + 256) > 160 * 1024 - 64 for sg in host(s)["seg"])
    assert [s for s in FLOW_OTHER if big(s)] == CHAIN_TOO_LARGE and not any(big(s) for s in FLOW_EIGHT)
    for s, t in zip(EIGHT, FLOW_EIGHT):   # the flow sizes have the 8-level sizes' level widths
        assert [w for w, _ in host(s)["levels"]] == [w for w, _ in host(t)["levels"]]
    # the refused plan: the host path's levels 1..4 from the frame at 1.9; the small plan's single level fits
    assert not host(REFUSED)["plan"] and res[(REFUSED, "small")]["plan"]
    for s in SIZES:
        assert host(s)["plan"] == (s != REFUSED), s
    # the 8-level sizes: two segments from the frame, the small plan chains 4..7 from level 3; chained level widths
    # of 1 and of 3 mod 4
    for s in EIGHT:
        assert len(host(s)["seg"]) == 2 and sorted(res[(s, "small")]["chain"]) == [4, 5, 6, 7]
        mods = {w % 4 for w, _ in host(s)["levels"][1:]}
        assert {1, 3} <= mods, (s, host(s)["levels"])
    assert host((331, 227, 1.2, 8))["levels"][7] == (92, 63)
    # small plans without a chain: at most kSmallChainBase + 1 levels
    for s in SIZES:
        assert res[(s, "small")]["plan"] == (s[3] > K_SMALL_CHAIN_BASE + 1), s
    # a last tile column of one dword group (here 1 or 2 pixels) and a one-row last tile row, in both tilings
    tiles = [(c["tile"], c["lastw"], c["lasth"]) for s in SIZES for c in host(s)["chain"].values()]
    for tiling in ("64x32", "32x16"):
        assert any(t == tiling and lw == 1 and lh == 1 for t, lw, lh in tiles), tiling
    assert host((290, 193, 1.5, 3))["chain"][1]["tile"] == "64x32" and host((327, 219, 1.5, 4))["chain"][3]["tile"] == "32x16"
    assert host((333, 229, 1.2, 8))["chain"][3]["lastw"] == 1 and host((333, 229, 1.2, 8))["chain"][4]["lastw"] == 1
    assert host((700, 420, 1.9, 3))["chain"][2]["lastw"] == 2 and host((384, 241, 1.5, 4))["chain"][1]["lasth"] == 1
    # packed_ok: holds everywhere at 1.9, fails for some group at 2.1 and up, in chain_job and in resize_tile
    assert all(c["bytes"] == 0 and c["packed"] > 0 for c in host((700, 420, 1.9, 3))["chain"].values())
    assert host((400, 300, 2.2, 2))["chain"][1]["bytes"] > 0 and host((400, 300, 2.2, 2))["chain"][1]["packed"] > 0
    assert int(host((700, 420, 1.9, 3))["resize"][1]["tiles_bytes"]) == 0
    assert int(host((260, 200, 2.1, 2))["resize"][1]["tiles_bytes"]) > 0
    # the kernels and instantiations of the per-level launches
    reached = set()
    for s in SIZES:
        for d in host(s)["resize"].values():
            reached.add((d["kernel"], d.get("TH"), d.get("KP")))
    assert reached == {("k_resize_tiled", "32", "2"), ("k_resize_tiled", "32", "3"), ("k_resize_tiled", "32", "0"),
                       ("k_resize_tiled", "16", "2"), ("k_resize_tiled", "16", "0"), ("k_resize", None, None)}, reached
    one = lambda s: (host(s)["resize"][1]["kernel"], host(s)["resize"][1].get("TH"), host(s)["resize"][1].get("KP"))
    assert one((331, 227, 1.2, 8)) == ("k_resize_tiled", "32", "2") and one((384, 241, 1.5, 4)) == ("k_resize_tiled", "32", "3")
    assert one((700, 420, 1.9, 3)) == ("k_resize_tiled", "32", "0") and one((400, 300, 2.2, 2)) == ("k_resize", None, None)
    assert one((270, 200, 2.3, 2)) == ("k_resize_tiled", "16", "0") and one((190, 200, 2.3, 2)) == ("k_resize_tiled", "16", "2")
    # the staging form follows the frame's alignment at level 1 and is the 16-byte one above it
    for align, form in ((16, "vec16"), (4, "dword"), (1, "byte")):
        r = _parse(model((331, 227, 1.2, 8), "small", 0, align).stdout)
        assert r["resize"][1]["staging"] == form and r["resize"][2]["staging"] == "vec16"
    # the third realigned dword: past a region's last row by at most 8 bytes in chain_job (the walk checks it stays
    # below lds_bytes), never past the last staged row's pitch in resize_tile
    assert max(c["over3rd"] for s in SIZES for c in host(s)["chain"].values()) == 8
    assert all(int(d["over3rd"]) <= 0 for s in SIZES for d in host(s)["resize"].values() if "over3rd" in d)
    # the sc1 byte load's aligned dword leaves the buffer only where the buffer's ends are not dword aligned
    assert all(sg["ld8_outside"] == 0 for s in SIZES for sg in host(s)["seg"])
    assert 1 <= max(sg["ld8_outside"] for sg in _parse(model((331, 227, 1.2, 8), "host", 0, 1).stdout)["seg"]) <= 3


def test_the_plan_is_refused_by_scale_and_depth(model):
    """The figures of build_chain's comment: the LDS a segment needs follows the scale factor and the levels it
    chains; the width does not enter (2560 wide fits at 1.2, 820 wide does not at 1.9 with four chained levels)."""
    lds = lambda size: [sg["lds_bytes"] for sg in _parse(model(size).stdout)["seg"]]
    assert lds((2560, 1440, 1.2, 8)) == [15456, 13728]
    assert lds((1280, 720, 1.6, 5)) == [63328] and lds((1280, 720, 1.7, 5)) == []
    assert lds((1280, 720, 1.9, 4)) == [61840] and lds(REFUSED) == []
    for size in ((1280, 720, 1.6, 5), (1280, 720, 1.9, 4), (2560, 1440, 1.2, 8)):
        assert model(size).stdout.strip().endswith("\nok")


@pytest.mark.parametrize("edit,size,line", [
    ("hkeep7", (331, 227, 1.2, 8), "px["), ("c0c0", (331, 227, 1.2, 8), ""), ("packed8chain", (400, 300, 2.2, 2), "o1[t] - bo <= 7"),
    ("packed8tile", (260, 200, 2.1, 2), "o1[i] - bo <= 7")])
def test_model_walk_notices_wrong_arithmetic(model, edit, size, line):
    """The walk with rs_hkeep's mask ~7, rs_row_entry's second weight c0, or packed_ok <= 8 in chain_job / resize_tile."""
    out = model(size, "host", 0, 16, edit)
    assert out.returncode == 1 and "violation" in out.stdout and line in out.stdout, out.stdout[-300:]


# ---- the planted frames on the oracle alone ----
@pytest.fixture(scope="module")
def oracle_levels(oracle_mod):
    memo = {}

    def get(size, content, variant):
        key = (size, content, variant)
        if key not in memo:
            w, h, scale, nl = size
            o = oracle_mod.OracleExtractor(500, scale, nl, flags=variant)
            o(frame(w, h, content))
            memo[key] = [o.level(l) for l in range(nl)]
        return memo[key]
    return get


@pytest.mark.parametrize("variant", [0, GENERIC])
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("size", [EIGHT[0], (400, 300, 2.2, 2), (384, 241, 1.5, 4)], ids=lambda s: "%dx%d_%g_%d" % s)
def test_planted_frames_mean_what_they_say(oracle_levels, size, content, variant):
    lv = oracle_levels(size, content, variant)
    assert np.array_equal(lv[0], frame(size[0], size[1], content))
    l1 = lv[1].astype(int)
    if content == "all255":      # weights sum to 2048 in both passes: 255 stays 255 at every level
        assert all((l == 255).all() for l in lv)
    elif content == "zeros":
        assert all((l == 0).all() for l in lv)
    elif content == "vstripes":  # every row the same, the columns not (the 3.x form truncates each row's two products:
        tol = 0 if variant == GENERIC else 1   # a level's rows within 1 more than its source's)
        assert all((abs(l.astype(int) - l[0].astype(int)) <= tol * i).all() for i, l in enumerate(lv)) and int(np.ptp(l1[0])) > 100
    elif content == "hstripes":
        assert all((l == l[:, :1]).all() for l in lv) and int(np.ptp(l1[:, 0])) > 100
    elif content == "checker":   # mixes of the two values in both directions
        assert len(np.unique(l1)) > 4 and not (l1 == l1[0]).all() and not (l1 == l1[:, :1]).all()
    elif content == "lastcolrow":
        assert (l1[:-2, :-2] == 0).all() and (l1[:-2, -1] > 0).all() and (l1[-1, :-2] > 0).all()
    else:
        assert len(np.unique(l1)) > 200
