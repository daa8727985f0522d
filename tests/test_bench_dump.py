"""bench.py's plain run and `--dump-outputs DIR`: the layout and size cap of the dump (CPU, over a stand-in
extractor), and on the GPU a plain C5 run -- no leg beside the timed steps on the line, `ms_per_step` the timed
steps' wall time, and a dump equal to what BatchExtractor returns in this process for the same frames (so it is
the same from run to run).  The bench runs as a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("counts", "frames", "keypoints", "descriptors")
LEGS = ("kernels_ms_per_step", "roofline", "cpu_baseline", "hamming", "stereo", "bird", "c4_frame", "host_path",
        "matcher", "matcher_c2")


class _FakeExtractor:
    """counts() / results(frame) of BatchExtractor over seeded random keypoints."""

    def __init__(self, counts):
        from orbgpu import KP_DTYPE
        rng = np.random.RandomState(7)
        self._counts = np.asarray(counts, np.int32)
        self._k, self._d = [], []
        for n in self._counts:
            k = np.zeros(n, KP_DTYPE)
            for f in ("x", "y", "size", "angle", "response"):
                k[f] = rng.rand(n).astype(np.float32) * 700
            k["octave"] = rng.randint(0, 8, n)
            k["class_id"] = -1
            self._k.append(k)
            self._d.append(rng.randint(0, 256, (n, 32)).astype(np.uint8))

    def counts(self):
        return self._counts.copy()

    def results(self, frame):
        return self._k[frame], self._d[frame]


def _load(path):
    out = {n: np.load(os.path.join(path, n + ".npy")) for n in NAMES}
    assert sorted(os.listdir(path)) == sorted(n + ".npy" for n in NAMES)
    assert all(a.dtype == np.float32 for a in out.values())
    return out


def _check_layout(d, ex):
    counts = ex.counts()
    assert np.array_equal(d["counts"], counts)
    sel = d["frames"].astype(int)
    assert np.all(np.diff(sel) > 0) and (len(sel) == 0 or (sel[0] >= 0 and sel[-1] < len(counts)))
    assert d["keypoints"].shape == (counts[sel].sum(), 7) and d["descriptors"].shape == (counts[sel].sum(), 32)
    at = 0
    for f in sel:
        k, de = ex.results(int(f))
        got = d["keypoints"][at:at + len(k)]
        for c, name in enumerate(("x", "y", "size", "angle", "response", "octave", "class_id")):
            assert np.array_equal(got[:, c], k[name].astype(np.float32)), (f, name)
        assert np.array_equal(d["descriptors"][at:at + len(k)], de)
        at += len(k)
    return sel


def test_dump_whole_batch(tmp_path):
    import bench
    ex = _FakeExtractor([5, 0, 17, 3])
    bench.dump_outputs(str(tmp_path / "a"), ex)
    sel = _check_layout(_load(str(tmp_path / "a")), ex)
    assert list(sel) == [0, 1, 2, 3]


def test_dump_sample_is_capped_and_fixed(tmp_path, monkeypatch):
    import bench
    ex = _FakeExtractor([40 + 3 * i for i in range(32)])
    cap = 100 * 1000   # the 32 frames hold 2,808 keypoints of 156 bytes each: about a fifth of them fit
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", cap)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), ex)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert all(np.array_equal(a[n], b[n]) for n in NAMES)
    sel = _check_layout(a, ex)
    assert 0 < len(sel) < 32
    size = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), n + ".npy")) for n in NAMES)
    assert size <= cap
    # no frame left out that would still have fitted whole after the sample's smallest possible next one
    assert cap - size < 156 * int(ex.counts().max()) + 4 * 256


def test_dump_size_limit_is_64_mb():
    import bench
    assert bench.DUMP_MAX_BYTES <= 64 * 1000 * 1000


def _plain_run(out_dir):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "c5", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, orbgpu_mod):
    from orbgpu.synth import bench_frames
    d = _plain_run(str(tmp_path / "a"))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "features/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8" and d["n_gpus"] == 1
    assert all(d[k] is None for k in LEGS), [k for k in LEGS if d[k] is not None]
    # ms_per_step is the timed loop's wall time per step (the line rounds seconds to 1 us, ms to 1e-4)
    assert abs(d["ms_per_step"] - d["ranks"][0]["seconds"] / 3 * 1e3) <= 1e-3 / 3 + 1e-4
    # value = keypoints per step / seconds per step, within the rounding of ms_per_step (half of 1e-4 ms)
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - d["ranks"][0]["keypoints_per_step"]) \
        <= (5e-5 / d["ms_per_step"] + 1e-6) * d["ranks"][0]["keypoints_per_step"]
    a = _load(str(tmp_path / "a"))
    assert a["counts"].sum() == d["ranks"][0]["keypoints_per_step"]
    # the same batch through BatchExtractor here: the dump is what a caller of the timed path reads back
    ex = orbgpu_mod.BatchExtractor(4000, 1280, 720, 8)
    try:
        ex.upload(bench_frames(1280, 720, 8, first=0))
        ex.launch()
        ex.sync()
        sel = _check_layout(a, ex)
        assert list(sel) == list(range(8))
    finally:
        ex.close()
