"""The host arithmetic of an edit-scoring call lives in a host-only header (poreseq_amd/csrc/ps_editplan.h) that the library and this
check both compile: which states the kernel sees for an edit's new columns (edited_window's 12-base look-back against the states of the
whole edited sequence), how many columns an edit adds, which matrix columns a list keeps, its distinct old-score columns, its size
classes, and the per-position layout of FindPointMutations' list — each against a naive restatement, on random sequences with non-ACGT
characters and edits at and past both ends (tests/native/editplan_check.cpp).  The same text runs once more under the address and
undefined-behaviour sanitizers, as a program of its own with the runtimes linked statically."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "editplan_check.cpp")


def test_edit_plan_tables_against_brute_force():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "editplan_check")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", SRC, "-o", exe])
        out = subprocess.check_output([exe, "6000"], timeout=300).decode()
    assert out.strip().endswith("failures=0"), out


def _static_runtime(name):
    """path of g++'s static sanitizer runtime `name`, or None when it is not installed (g++ then echoes the bare name)"""
    path = subprocess.check_output(["g++", "-print-file-name=" + name]).decode().strip()
    return path if os.path.isabs(path) and os.path.exists(path) else None


def test_edit_plan_check_is_clean_under_host_sanitizers():
    """the runtimes are linked statically: a program of its own that runs in whatever environment the suite runs in, as it is"""
    import pytest
    missing = [n for n in ("libasan.a", "libubsan.a") if _static_runtime(n) is None]
    if missing:
        print("static sanitizer runtime not installed (%s): the sanitizer half of the edit plan check is skipped" % ", ".join(missing))
        pytest.skip("no static sanitizer runtime for g++ on this machine: " + ", ".join(missing))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "editplan_check_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-static-libubsan", SRC, "-o", exe])
        p = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("failures=0"), p.stdout + p.stderr[-2000:]
