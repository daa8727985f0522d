"""CPU: the owning buffer behind every device and pinned allocation of the library (csrc/buf.h), without a GPU.

tests/cpp_buf/buf_model.cc instantiates Buf with a policy over malloc that counts allocations, frees and live blocks and
can fail the next allocation, and checks reuse without reallocation (the pointer stays), growth (one free, one
allocation, the floor), the empty state after a failed allocation, moves, swap, reset and the destructor, and that no
block is left.  It is a plain executable built with AddressSanitizer and UBSan and run directly, so a double free or a
touch of a freed block ends it with a report; leaks are caught by the policy's own live count."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp_buf", "buf_model.cc")


def test_buf_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "buf_model")
    # plain g++: the template names no HIP symbol
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-self-move",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")   # (the model counts live blocks itself)
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("\nok") and "violation" not in out.stdout, (
        out.stdout[-800:], out.stderr[-2000:])
    allocs, frees, live = (int(v) for v in out.stdout.splitlines()[-2].split()[1::2])
    assert allocs == frees > 10 and live == 0
