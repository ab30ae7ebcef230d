"""The checkpoint layout of the Smith-Waterman module has one home, a host-compilable header (poreseq_amd/csrc/ps_swplan.h) that the
fills, the traceback, sw_launch and this check all compile.  The check (tests/native/sw_layout_check.cpp) lays out batches of pairs
as sw_launch does, on heap pools of exactly their size under AddressSanitizer and UBSan, walks every rowsave / colsave / blkmax entry
the fills store and every one the traceback can load (lengths around the 64-row blocks, the 512-column band strips and the
super-strips, band widths 0 / 64 / 128 / 1024, every fill form, all three traceback forms) and asserts that each index stays inside
its own pair's part, that no two entries share an int and that every rowsave / colsave entry loaded is one the fill stored: those
pools are never cleared.  It also pins sw_pair_bytes, which cuts the chunks.  The kernels themselves: test_hip_sw_band.py."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fills_traceback_and_allocation_agree_on_the_layout():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sw_layout_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               os.path.join(HERE, "native", "sw_layout_check.cpp"), "-o", exe])
        run = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    assert run.returncode == 0 and out.strip().endswith("failures=0"), out
