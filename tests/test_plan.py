"""The device-memory plan's arithmetic lives in a host-only header (poreseq_amd/csrc/ps_plan.h) that the library and this check both
compile: the shares, slabs and cache limit DESIGN.md section 3 promises for a 309 GB device, the bytes of a skewed score matrix, and
what the cut of a lock-step call into sub-batches guarantees (it advances, a chunk of several regions fits the cap, a list that fits
is one chunk, every region is covered once and in order).  The GPU tests of the plan at work: the slab tests of test_hip_variant.py,
the cache / small-budget / split tests of test_hip_regime.py."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_plan_numbers_matrix_bytes_and_share_cut():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "plan_check")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(HERE, "native", "plan_check.cpp"), "-o", exe])
        out = subprocess.check_output([exe, "20000"], timeout=300).decode()
    assert out.strip().endswith("failures=0"), out
