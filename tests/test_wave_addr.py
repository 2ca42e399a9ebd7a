"""The address split of k1's and kr's LDS-DMA pieces and slab stores (loma-nerf_amd/csrc/
lnerf_wave_addr.h: wave-uniform base + per-lane constant + immediate), checked on the host before
any kernel uses it: tests/native/wave_addr_check.cpp compares the split with the pointer expressions
it replaced for every lane (4- and 8-wave rings, whole and partial chunks, all 8 k-steps, both
halves, every block up to a layer's last), and checks every address against its chunk, ring slot or
slab and every byte for being moved exactly once. Built with the host compiler under
AddressSanitizer + UBSan as a stand-alone program. No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "wave_addr_check.cpp")
CSRC = os.path.join(ROOT, "loma-nerf_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host toolchain")
def test_wave_address_split_matches_pointer_expressions(tmp_path):
    exe = str(tmp_path / "wave_addr_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", exe], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "verify_asan_link_order=0:detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "all wave address checks passed" in out, out
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out
