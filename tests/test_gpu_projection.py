"""GPU parity of the projection-gated searches (orb_search_by_projection: k_projection_topk + the host replay)
against tests/projection_ref.py, the restated loops of ORBmatcher.cc:45-129, :1328-1470 and :1923-1998: match_t and
nmatches equal exactly, for both lane mappings of the kernel (a query per wavefront, the default, and a query per
16-lane row, ORBGPU_PROJ_LANES=16).  The inputs come from tests/projection_cases.py; tests/test_projection_ref.py checks
on the CPU that they reach every branch of the reference loops."""
import numpy as np
import pytest

import projection_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[16, 64])
def lanes(request, monkeypatch):
    monkeypatch.setenv("ORBGPU_PROJ_LANES", str(request.param))
    return request.param


def _check(orbgpu_mod, oracle_mod, name):
    want_m, want_n, _ = pc.expected(oracle_mod, name)
    n, m = pc.run_product(orbgpu_mod, pc.case(name))
    bad = np.flatnonzero(m != want_m)[:8]
    assert n == want_n and bad.size == 0, (name, n, want_n, bad.tolist(), m[bad].tolist(), want_m[bad].tolist())
    return n, m


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_three_forms_match_reference(orbgpu_mod, oracle_mod, lanes, name):
    n, m = _check(orbgpu_mod, oracle_mod, name)
    assert n >= 50


@pytest.mark.parametrize("name", ["exhaustion_best", "exhaustion_ratio"])
def test_exhausted_list_is_reranked(orbgpu_mod, oracle_mod, lanes, name):
    """Twelve identical queries on a window of 24: the ninth finds the eight trains of its list taken."""
    n, m = _check(orbgpu_mod, oracle_mod, name)
    assert n == 12


def test_lane_mapping_boundaries(orbgpu_mod, oracle_mod, lanes):
    """37 queries (the last block's rows partly idle) whose windows hold 0, 1, 5 and 80 candidates, mixed within a
    wavefront."""
    _check(orbgpu_mod, oracle_mod, "lanes")


def _core(orbgpu_mod, c, **kw):
    """A CF/LF case through the generic entry point with overrides (queries built as the wrapper builds them)."""
    p, f = c["pts"], c["frame"]
    q = np.zeros(len(p["u"]), orbgpu_mod.PROJ_QUERY_DTYPE)
    q["u"], q["v"] = p["u"], p["v"]
    q["r"] = np.float32(c["th"]) * f["scale_factors"][p["octave"]]
    q["min_level"], q["max_level"] = p["octave"] - 1, p["octave"] + 1
    q["ur_tol"] = q["r"]
    q["angle"], q["blocks"] = p["angle"], p["observed"]
    for k in ("u", "v", "r"):
        if k in kw:
            q[k] = kw.pop(k)
    sel = kw.pop("sel", slice(None))
    args = dict(mode=orbgpu_mod.PROJ_BEST, queries=q[sel], qdesc=p["desc"][sel], tdesc=f["desc"], kps_t=f["kps"],
                grid=orbgpu_mod.frame_grid(f["kps"], *f["bounds"]), t_uright=None, t_taken=f["taken"],
                min_xy=(f["bounds"][0], f["bounds"][2]))
    args.update(kw)
    return orbgpu_mod.ORBmatcher(0.9, False).search_by_projection(**args)


def test_edges(orbgpu_mod, oracle_mod, lanes, monkeypatch):
    c = pc.case("cflf_mono_th15")
    nt = len(c["frame"]["kps"])
    want_m, want_n, _ = pc.expected(oracle_mod, "cflf_mono_th15")
    n, m = _core(orbgpu_mod, c)
    assert n == want_n and np.array_equal(m, want_m)      # the generic entry point itself
    # no queries; no trains
    n, m = _core(orbgpu_mod, c, sel=slice(0, 0))
    assert n == 0 and (m == -1).all() and len(m) == nt
    empty = orbgpu_mod.frame_grid(c["frame"]["kps"][:0], *c["frame"]["bounds"])
    n, m = _core(orbgpu_mod, c, tdesc=c["frame"]["desc"][:0], kps_t=c["frame"]["kps"][:0], grid=empty, t_taken=None)
    assert n == 0 and len(m) == 0
    # every window entirely outside the grid (left of it, below it, far away)
    for u, v in [(-500.0, 100.0), (100.0, 5000.0), (1e30, -1e30)]:
        n, m = _core(orbgpu_mod, c, u=np.float32(u), v=np.float32(v))
        assert n == 0 and (m == -1).all()
    # r = 0: |dx| < 0 never holds
    n, m = _core(orbgpu_mod, c, r=np.float32(0))
    assert n == 0 and (m == -1).all()
    # every train taken
    n, m = _core(orbgpu_mod, c, t_taken=np.ones(nt, bool))
    assert n == 0 and (m == -1).all()
    # max_dist is the reference's TH_HIGH: the restated loop with another constant gives the same matches
    import projection_ref as ref
    for md in (30, 255):
        monkeypatch.setattr(ref, "TH_HIGH", md)
        rm, rn, _ = pc.reference(oracle_mod, c)
        n, m = _core(orbgpu_mod, c, max_dist=md)
        assert n == rn and np.array_equal(m, rm), md
    assert rn > want_n


def test_argument_errors_with_a_context(orbgpu_mod, lanes):
    c = pc.case("lanes")
    for kw in (dict(mode=2), dict(max_dist=257), dict(max_dist=-1), dict(u=np.float32(np.nan)),
               dict(v=np.float32(np.inf)), dict(r=np.float32(-0.5)), dict(r=np.float32(np.nan))):
        with pytest.raises(orbgpu_mod.OrbError) as e:
            _core(orbgpu_mod, c, **kw)
        assert e.value.status == -1, kw
    inv_w, inv_h, off, idx = orbgpu_mod.frame_grid(c["frame"]["kps"], *c["frame"]["bounds"])
    bad_idx = idx.copy()
    bad_idx[3] = len(c["frame"]["kps"])
    bad_off = off.copy()
    bad_off[200] = off[-1] + 1
    for g in ((inv_w, inv_h, off, bad_idx), (inv_w, inv_h, bad_off, idx)):
        with pytest.raises(orbgpu_mod.OrbError) as e:
            _core(orbgpu_mod, c, grid=g)
        assert e.value.status == -1
    # the context still works after the refusals
    n, m = _core(orbgpu_mod, c)
    assert n >= 10
