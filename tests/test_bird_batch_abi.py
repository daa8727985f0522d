"""No GPU: the batched birdview entry points are exported, bound and versioned."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("orb_bird_extract_batch_device", "orb_bird_extract_batch", "orb_bird_batch_group")


def test_library_exports_the_batch_symbols(orbgpu_mod):
    from orbgpu import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in SYMBOLS:
        assert s in exported, s


def test_ctypes_binds_the_batch_symbols(orbgpu_mod):
    from orbgpu import _lib
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
        fn = getattr(L, s)
        assert fn.argtypes == _lib.SIGNATURES[s][1] and fn.restype is _lib.SIGNATURES[s][0]
    assert len(_lib.SIGNATURES["orb_bird_extract_batch_device"][1]) == 14
    assert len(_lib.SIGNATURES["orb_bird_extract_batch"][1]) == 13
    assert hasattr(orbgpu_mod.BirdORB, "extract_batch") and hasattr(orbgpu_mod.BirdORB, "extract_batch_device")


def test_header_declares_them_and_its_version_is_the_library_s(orbgpu_mod):
    from orbgpu import _lib
    hdr = open(_lib.HEADER).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert re.search(r"#define\s+ORB_BIRD_MAX_BATCH\s+64\b", hdr)
    ver = int(re.search(r"#define\s+ORBGPU_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert _lib.lib().orb_abi_version() == ver


def test_batch_argument_errors_need_no_device(orbgpu_mod):
    """NULL object: ORB_ERR_ARG before any GPU work."""
    from orbgpu import _lib
    L = _lib.lib()
    assert L.orb_bird_extract_batch_device(None, 1, None, 8, 8, 8, 64, None, 0, 0, None, None, 0, None) == -1
    assert L.orb_bird_extract_batch(None, 1, None, 8, 8, 8, None, 0, 0, None, None, 0, None) == -1
    assert L.orb_bird_batch_group(None, 0) == -1
