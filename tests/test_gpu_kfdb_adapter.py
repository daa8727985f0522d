"""GPU: the drop-in KeyFrameDatabase adapter (adapter/KeyFrameDatabase_gpu.cc, the reference's member signatures) over
the models in tests/cpp_kfdb/slam_api/, and the host mirror's ORBVocabulary::score.  tests/cpp_kfdb/test_kfdb_adapter
runs the planted scripts of tests/kfdb_cases.py (add, erase, clear, both Detect* calls, score); the returned keyframe
id vectors and the scores' bits must equal the restatement's."""
import os
import struct
import subprocess

import pytest

import kfdb_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_kfdb")


@pytest.fixture(scope="module")
def adapter_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP, "test_kfdb_adapter"])
    return os.path.join(CPP, "test_kfdb_adapter")


@pytest.mark.gpu
def test_adapter_equals_the_restatement(adapter_bin, orbgpu_mod, tmp_path):
    lds = orbgpu_mod._lib.lib().orb_kfdb_query_lds_words()
    ndetect = 0
    for name, script in kc.all_scripts(lds).items():
        if name == "lengths":
            continue    # (its long queries are the kernel's business: tests/test_gpu_kfdb.py)
        src, dst = tmp_path / (name + ".txt"), tmp_path / (name + ".out")
        src.write_text(kc.to_text(script))
        p = subprocess.run([adapter_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (name, p.stderr[-2000:])
        want = []
        for op, r in zip(script, kc.run_ref(script)):
            if op[0] in ("reloc", "loop"):
                want.append(" ".join([op[0]] + [str(i) for i in r["ids"]]))
                ndetect += 1
            elif op[0] == "score":
                want.append("score %016x" % struct.unpack("<Q", struct.pack("<d", r))[0])
        assert dst.read_text().splitlines() == want, name
    assert ndetect >= 12
