"""CPU test: INTEGRATION.md's "Environment knobs" table names exactly the PORESEQ_* variables the package reads — every
getenv("PORESEQ_...") of the native library and every os.environ / os.getenv access of the Python package — each one once."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"(PORESEQ_[A-Z0-9_]+)"


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _names_in_code():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "poreseq_amd", "csrc", "*.*")):
        if path.endswith((".cpp", ".hip", ".h")):
            names.update(re.findall(r'getenv\(\s*"' + NAME + '"', _read(path)))
    for path in glob.glob(os.path.join(ROOT, "poreseq_amd", "*.py")) + [os.path.join(ROOT, "__graft_entry__.py")]:
        names.update(re.findall(r'(?:environ(?:\.\w+)?\s*[\[(]|getenv\()\s*["\']' + NAME + r'["\']', _read(path)))
    return names


def _names_in_table():
    """PORESEQ_* names of the first column of every row of the table under "## Environment knobs"."""
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    section = text.split("## Environment knobs", 1)[1]
    rows = []
    for line in section.splitlines()[1:]:
        if line.startswith("|"):
            rows.append(line)
        elif rows:
            break   # the table has ended
    names = []
    for row in rows[2:]:   # (header, rule)
        names += re.findall(NAME, row.split("|")[1])
    return names


def test_knob_table_lists_every_variable_the_package_reads_once():
    code, table = _names_in_code(), _names_in_table()
    assert len(code) > 20 and len(table) > 20   # the scans found their sources
    assert sorted(set(table)) == sorted(code), "only in the table: %s; only in the code: %s" % (sorted(set(table) - code), sorted(code - set(table)))
    assert len(table) == len(set(table)), "listed more than once: %s" % sorted(n for n in set(table) if table.count(n) > 1)
