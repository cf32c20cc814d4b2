"""CPU check of the train-triple membership probes (csrc/kge_sampler_device.h): tests/set_probe_host.cpp, a stand-alone program,
fills tables by k_set_insert's rule on the host -- 16 slots with 8 keys, 1 024 slots with 512 keys, tables whose keys all share one
home slot near the end so that the run wraps -- and compares set_contains_wide<4 / 8 / 16> with set_contains for every present key
and for absent keys.  Its host side is built with AddressSanitizer and UBSan and every table is a heap block of exactly its size,
so a group load that leaves the table fails the run.  Skips where hipcc is not installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    return p if os.access(p, os.X_OK) else shutil.which("hipcc")


def test_wide_probe_equals_one_slot_probe_on_host(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not installed")
    exe = str(tmp_path / "set_probe_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "pykg2vec_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "set_probe_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr, (r.stdout, r.stderr[-4000:])
