"""ViterbiMutate's walk over the reference positions — which positions are kept and the mean level per (position, event) — lives
in a host-only header (poreseq_amd/csrc/ps_vitgather.h) that the library and this check both compile.  It is index arithmetic on
ref_index values a caller may have written: a table indexed by position + 1, (int) conversions, follow-on levels.  The check runs
it under AddressSanitizer and UBSan on heap arrays of exactly their own size and compares T and every record with a naive
restatement (a linear search per position): reads without an aligned level, -1 markers in ref_index, whole values past the largest
refend, the skip and the stop rule, events of 0 levels, E = 1, an event without a ref_index, fractional / NaN / huge values, and a
few hundred seeded compositions.  The GPU tests of the walk at work: test_hip_ref_tables.py."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_walk_equals_a_naive_restatement_under_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "vitgather_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               os.path.join(HERE, "native", "vitgather_check.cpp"), "-o", exe])
        run = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    assert run.returncode == 0 and out.strip().endswith("failures=0"), out
