"""The band mode of the Smith-Waterman fill (poreseq_amd/csrc/ps_sw.hip) takes a banded result only under an exactness certificate.
Host check of that certificate (tests/native/sw_band_check.cpp): on random pairs (identities 60-100 %, length differences up to 2 wb,
tandem and interspersed repeats off the diagonal) every certified result equals the full-matrix SW's, and every banded cell that
passes Hb >= B equals the full value.  The GPU tests compare the kernels themselves (test_hip_sw_band.py)."""
import os
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_band_certificate_is_exact():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sw_band_check")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(HERE, "native", "sw_band_check.cpp"), "-o", exe])
        out = subprocess.check_output([exe, "2000"], timeout=600).decode()
    assert out.strip().endswith("mismatches=0"), out
    m = re.search(r"certified=(\d+) .* near_edge=(\d+)", out)
    assert m and int(m.group(1)) > 200 and int(m.group(2)) > 10, out   # both outcomes and maxima near the band edge are exercised
