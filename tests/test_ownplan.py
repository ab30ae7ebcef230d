"""Where the outputs of the own-sequence statistics calls (AlignStats, KmerStats, MoveStats, PosteriorStats) lie in their device
buffer is stated once, in a host-only header (poreseq_amd/csrc/ps_ownplan.h) that the library and this check both compile: the
descriptors of the kernels, the one copy back and the scatter into the callers' arrays all take their addresses from it.  The check
runs it under AddressSanitizer and UBSan on a few thousand seeded calls — every kind, with and without a realignment, regions
without events, events without levels, random wants and group counts — and holds every segment to its bounds, its alignment and a
naive restatement of the three layouts the header replaced.  The GPU tests of the plan at work: test_hip_own_plan.py."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_plan_equals_a_naive_restatement_under_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ownplan_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               os.path.join(HERE, "native", "ownplan_check.cpp"), "-o", exe])
        run = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    assert run.returncode == 0 and out.strip().endswith("failures=0"), out
