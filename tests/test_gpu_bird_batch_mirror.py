"""GPU: the C++ host mirror's BirdviewORB::extractBirdviewBatch (host/BirdviewORB.{h,cc}) against the oracle.
tests/cpp_bird_batch/test_bird_batch_mirror reads the frames and masks this test writes, calls
extractBirdviewBatch with 0, 1 and N masks and writes the results back."""
import os
import subprocess

import numpy as np
import pytest

import bird_batch_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-birdview_amd")
CPP = os.path.join(ROOT, "tests", "cpp_bird_batch")
NF = 500


@pytest.fixture(scope="module")
def mirror_bin():
    subprocess.check_call(["make", "-s", "-C", PKG, "liborbslam_host.so"])
    subprocess.check_call(["make", "-s", "-C", CPP])
    return os.path.join(CPP, "test_bird_batch_mirror")


@pytest.mark.gpu
def test_mirror_extract_birdview_batch_matches_oracle(mirror_bin, oracle_mod, orbgpu_mod, tmp_path):
    from orbgpu import KP_DTYPE
    frames = bc.FIVE
    ids = [fr[2] for fr in frames]
    w, h = frames[0][:2]
    src, dst = tmp_path / "frames.bin", tmp_path / "results.bin"
    src.write_bytes(np.array([NF, w, h, len(frames), len(ids)], np.int32).tobytes() +
                    b"".join(bc.frame(*fr).tobytes() for fr in frames) +
                    b"".join(bc.mask(w, h, i).tobytes() for i in ids))
    p = subprocess.run([mirror_bin, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = dst.read_bytes()
    o = 0
    for call, mask_ids in enumerate(([None] * 5, [ids[0]] * 5, ids)):
        for f, (fr, mi) in enumerate(zip(frames, mask_ids)):
            n = int(np.frombuffer(res, np.int32, 1, o)[0])
            o += 4
            k = np.frombuffer(res, KP_DTYPE, n, o)
            o += n * KP_DTYPE.itemsize
            d = np.frombuffer(res, np.uint8, n * 32, o).reshape(n, 32)
            o += n * 32
            bc.assert_frame((k, d), NF, fr, mi, f"call {call} ({'no' if call == 0 else 'shared' if call == 1 else 'N'} "
                                                f"masks): frame {f}")
    assert o == len(res)
