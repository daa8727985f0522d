"""CPU: the keyframe searches (Fuse, SearchBySim3, the keyframe forms of SearchByProjection).  The cases reach every
branch the restatement counts; orb_project_best_host equals the restatement; orb_project_best_batch refuses malformed
targets before it looks at the context; the replay rule of INTEGRATION.md (batched search + dirty points) gives the
reference's order of work's graph, and does not without the dirty rule."""
import ctypes

import numpy as np
import pytest

import kf_projection_cases as cases
import kf_projection_ref as ref
import kf_replay_toy as toy


def _target(orbgpu, kf, pts, level_above=0):
    from orbgpu import _kf_target
    return _kf_target(cases.product_kf(orbgpu, kf), pts, level_above)


def _host_all(orbgpu, gate, kf, pts):
    t = _target(orbgpu, kf, pts)
    out = [orbgpu.project_best_host(gate, t, i) for i in range(len(pts["u"]))]
    return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64)


def test_round_f32_helper():
    rng = np.random.default_rng(0)
    for x in rng.uniform(-1e3, 1e3, 200):
        assert ref.round_f32(float(np.float32(x))) == np.float32(x)
    one, eps = np.float32(1.0), np.float32(2.0 ** -24)
    assert ref.fmaf(one, one, eps) == one                                  # a tie goes to even
    assert ref.fmaf(one + np.float32(2.0 ** -23), one, eps) == one + np.float32(2.0 ** -22)
    # a case where rounding the exact sum to float64 first would double-round: 1 + 2^-24 + 2^-60 is above the tie
    assert ref.round_f32(1 + ref.Fraction(1, 2 ** 24) + ref.Fraction(1, 2 ** 60)) == one + np.float32(2.0 ** -23)
    assert np.float32(np.float64(1 + 2.0 ** -24 + 2.0 ** -60)) == one


def test_fuse_cases_reach_every_branch(oracle_mod):
    targets = cases.fuse_targets()
    assert [(len(kf["kps"]), len(p["u"])) for kf, p in targets] == [(300, 37), (450, 130), (600, 201), (300, 0), (0, 20)]
    for k in range(3):
        kf, pts = targets[k]
        wc = cases.window_counts(oracle_mod, kf, pts)
        assert 0 in wc and 1 in wc and 5 in wc and max(wc) > 64, sorted(set(wc))
        ur = kf["uright"]
        assert (ur == -1).sum() > 5 and (ur == 0).sum() > 5 and (ur > 0).sum() > 5
        for chi2 in (True, False):
            bi, bd, c = cases.expected_fuse(oracle_mod, k, chi2)
            assert c["level_skips"] >= 5 and c["ties_first_kept"] >= 5, c
            if chi2:
                assert c["chi2_stereo_rejections"] >= 5 and c["chi2_mono_rejections"] >= 5, c
            assert int(((bi >= 0) & (bd <= ref.TH_LOW)).sum()) >= 30
    # the gate's boundary points: one float32 below the constant the train is kept, one above it is skipped
    edges = cases.edge_points()
    kf, pts = targets[1]
    bi, _, _ = cases.expected_fuse(oracle_mod, 1, True)
    assert bi[:len(edges)].tolist() == [e[4] for e in edges]
    assert cases.expected_fuse(oracle_mod, 1, False)[0][:len(edges)].tolist() == [e[3] for e in edges]
    for (u, v, urr, j, want) in edges:
        kpx, kpy, kpr = cases.EDGE_TRAINS[j]
        e2, stereo = ref.fuse_e2(u, v, urr, kpx, kpy, kpr)
        const = 7.8 if stereo else 5.99
        assert stereo == (kpr >= 0)
        if want < 0:
            assert float(e2) > const and float(np.nextafter(e2, np.float32(0))) <= const
        else:
            assert float(e2) <= const and float(np.nextafter(e2, np.float32(np.inf))) > const


def test_sequential_and_sim3_cases_reach_every_branch(oracle_mod):
    nfound, vn, c = cases.expected(oracle_mod, "sim3")
    assert c["sim3_disagreements"] >= 5 and c["level_skips"] >= 5 and c["ties_first_kept"] >= 5 and nfound >= 50
    match, n, c = cases.expected(oracle_mod, "loop")
    assert n >= 50 and c["taken_skips"] >= 5 and c["level_skips"] >= 5
    assert n == int((match >= 0).sum())
    match, n, c = cases.expected(oracle_mod, "reloc")
    assert n >= 50 and c["taken_skips"] >= 5 and c["rotation_culls"] >= 5
    assert int((match == -2).sum()) >= 5


@pytest.mark.parametrize("gate", [0, 1])
def test_project_best_host_equals_restatement(orbgpu_mod, oracle_mod, gate):
    for k, (kf, pts) in enumerate(cases.fuse_targets()):
        bi, bd, _ = cases.expected_fuse(oracle_mod, k, gate == 1)
        hi, hd = _host_all(orbgpu_mod, gate, kf, pts)
        assert hi.tolist() == bi.tolist() and hd.tolist() == bd.tolist(), k
    kf1, kf2, p12, p21 = cases.sim3_case()
    for kf, pts in ((kf2, p12), (kf1, p21)):
        want = dict(pts, ur=np.zeros(len(pts["u"]), np.float32))
        bi, bd, _ = ref.fuse_search(oracle_mod, kf, want, gate == 1)
        hi, hd = _host_all(orbgpu_mod, gate, kf, want)
        assert hi.tolist() == bi.tolist() and hd.tolist() == bd.tolist()


def test_project_best_batch_rejects_malformed_targets(orbgpu_mod):
    """Every check of orb_project_best_batch runs before the context is looked at (it is NULL here: no GPU), each with
    its own message; a well-formed call gets as far as the NULL-context error."""
    from orbgpu import _lib, _ProjTargets
    L = _lib.lib()
    kf, pts = cases.fuse_targets()[0]

    def call(gate, mutate=None, ntargets=None, targets=None):
        ts = [_target(orbgpu_mod, kf, pts), _target(orbgpu_mod, kf, pts)] if targets is None else targets
        if mutate:
            mutate(ts[1])
        T = _ProjTargets(ts)
        post = getattr(mutate, "post", None)
        if post:
            post(T.arr[1])
        st = L.orb_project_best_batch(None, gate, len(ts) if ntargets is None else ntargets, ctypes.addressof(T.arr))
        return st, L.orb_last_error().decode()

    def q_field(name, i, value):
        def m(t):
            t["q"] = t["q"].copy()
            t["q"][name][i] = value
        return m

    def grid(f):
        def m(t):
            inv_w, inv_h, off, idx = t["grid"]
            off, idx = off.copy(), idx.copy()
            f(off, idx)
            t["grid"] = (inv_w, inv_h, off, idx)
        return m

    def post(f):
        def m(t):
            pass
        m.post = f
        return m

    def octave(t):
        t["kps_t"] = t["kps_t"].copy()
        t["kps_t"]["octave"][7] = 8

    P = "orb_project_best_batch: target 1: "
    for gate in (0, 1):
        assert call(gate) == (-1, "NULL context")
        assert call(gate, targets=[]) == (-1, "NULL context")
    assert call(2) == (-1, "orb_project_best_batch: unknown gate")
    assert call(-1) == (-1, "orb_project_best_batch: unknown gate")
    assert call(0, ntargets=-1) == (-1, "orb_project_best_batch: ntargets < 0 or targets NULL")
    assert call(0, post(lambda s: setattr(s, "best_idx", None))) == (-1, P + "NULL outputs")
    assert call(1, post(lambda s: setattr(s, "best_dist", None))) == (-1, P + "NULL outputs")
    for name, value in (("u", np.nan), ("v", np.inf), ("r", np.nan), ("r", -1.0)):
        assert call(0, q_field(name, 5, value)) == (-1, P + "query window not finite or radius negative")
    assert call(1, q_field("ur", 3, np.nan)) == (-1, P + "query ur not finite")
    assert call(0, q_field("ur", 3, np.nan)) == (-1, "NULL context")        # ur is not read without the gate

    def first(off, idx):
        off[0] = 1

    def dec(off, idx):
        j = int(np.flatnonzero(off[:3000] >= 1)[0])
        off[j + 1] = off[j] - 1

    def oob(off, idx):
        idx[7] = len(kf["kps"])
    assert call(0, grid(first)) == (-1, P + "grid cell_off[0] != 0")
    assert call(0, grid(dec)) == (-1, P + "grid cell_off decreases")
    assert call(1, grid(oob)) == (-1, P + "grid index out of range")

    def dec_and_nan(t):   # two faults: the grid is checked with the other pointers, ahead of the query values
        grid(dec)(t)
        q_field("u", 5, np.nan)(t)
    assert call(0, dec_and_nan) == (-1, P + "grid cell_off decreases")
    assert call(1, post(lambda s: setattr(s, "inv_sigma2", None))) == (-1, P + "inv_sigma2 NULL")
    assert call(0, post(lambda s: setattr(s, "inv_sigma2", None))) == (-1, "NULL context")
    for n in (0, 17):
        assert call(1, post(lambda s, n=n: setattr(s, "nlevels", n))) == (-1, P + "nlevels outside [1, ORBGPU_MAX_LEVELS]")
    assert call(1, octave) == (-1, P + "train octave outside [0, nlevels)")
    assert call(0, octave) == (-1, "NULL context")                          # the octave indexes nothing without the gate
    # the host helper refuses the same things
    t = _target(orbgpu_mod, kf, pts)
    octave(t)
    with pytest.raises(orbgpu_mod.OrbError, match="train octave outside"):
        orbgpu_mod.project_best_host(1, t, 0)
    with pytest.raises(orbgpu_mod.OrbError, match="bad arguments"):
        orbgpu_mod.project_best_host(0, _target(orbgpu_mod, kf, pts), len(pts["u"]))
    assert call(1) == (-1, "NULL context")


def _host_search(orbgpu, gate):
    def single(target, i, desc):
        kf, pts, _ = target
        t = _target(orbgpu, kf, pts)
        t["qdesc"] = t["qdesc"].copy()
        t["qdesc"][i] = desc
        return orbgpu.project_best_host(gate, t, i)
    return single


def check_replay(batch_search, single, scw):
    want_state, want_nfused, log, asked = toy.sequential(single, scw)
    # Replace events that change a descriptor which is queried afterwards
    changed = {mid for mid, ch in log if ch}
    later = {i for k, i, version in asked if version > 0 and i in changed}
    assert len(later) >= 3, (log, later)
    assert sum(want_nfused) >= 20
    got_state, got_nfused, _, _ = toy.replay(batch_search, single, scw)
    assert got_nfused == want_nfused and got_state == want_state
    off_state, off_nfused, _, _ = toy.replay(batch_search, single, scw, dirty_rule=False)
    assert off_state != want_state, "the case does not need the dirty rule"


@pytest.mark.parametrize("scw", [False, True])
def test_replay_rule_on_the_host(orbgpu_mod, scw):
    gate = 0 if scw else 1
    single = _host_search(orbgpu_mod, gate)

    def batch(targets):
        out = []
        for kf, pts, _ in targets:
            out.append(_host_all(orbgpu_mod, gate, kf, pts))
        return out
    check_replay(batch, single, scw)
