"""The deterministic back-trace of ViterbiMutate (nkeep == 0) lives in a host-only header (poreseq_amd/csrc/ps_vitpath.h) that the
library and this check both compile.  A back-pointer of -1 on the path (a dead max-plus row) must end the walk
with the row to name instead of indexing the table with -1: the check runs the walk under AddressSanitizer and UBSan on heap tables
of exactly their own size (live, dead from row 0 / from a middle row / in the last row only, T = 1, a -1 off the path, regions at
t_off > 0 of a concatenated table).  The GPU tests of the rule at work: the dead-row cases of test_hip_viterbi_tables.py and tier E
of test_hip_edge_values.py."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_back_trace_stops_at_a_missing_back_pointer():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "vitpath_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               os.path.join(HERE, "native", "vitpath_check.cpp"), "-o", exe])
        run = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    assert run.returncode == 0 and out.strip().endswith("failures=0"), out
