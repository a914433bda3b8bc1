"""The owners of device and pinned memory (csrc/orbx_mem.h) where no allocation succeeds.

tests/cpp/test_mem.cpp holds every owner to its failure contract -- a failed ensure leaves it empty, and a
second ensure, a release, a move, a swap and the destructor are safe afterwards -- and the sites' growth
policies to the expressions they replaced.  Built here with the address and undefined-behaviour sanitizers
and run as a child process, only where no GPU is visible: that is the case it exists for (the GPU suite holds
the success paths), and a sanitized program does not open a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "orb_slam2_commit_amd", "csrc")


def test_mem_owners_sanitized(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = str(tmp_path / "test_mem")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall",
                           "-Werror"] + san + ["-x", "hip", os.path.join(ROOT, "tests", "cpp", "test_mem.cpp"),
                                               os.path.join(CSRC, "scratch.hip"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert "mem owners ok" in r.stdout, r.stdout
