"""The extraction plan (csrc/plan.hip): pure host arithmetic that decides every LDS size, table index and
launch group of the extraction kernels, and the block-layout cursor of the extractor's host paths
(csrc/orbx_extractor.h).

CPU only: tests/cpp/test_plan.cpp builds plans over a set of geometries and walks them, asserting what the
kernels rely on unguarded; it is built here under the address and undefined-behaviour sanitizers, with
bounds-checked standard containers, and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "orb_slam2_commit_amd", "csrc")


def test_plan_sanitized(tmp_path):
    exe = str(tmp_path / "test_plan")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall",
                           "-Werror", "-D_GLIBCXX_ASSERTIONS"] + san +
                          ["-x", "hip", os.path.join(ROOT, "tests", "cpp", "test_plan.cpp"),
                           os.path.join(CSRC, "plan.hip"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "plan ok" in r.stdout, r.stdout
