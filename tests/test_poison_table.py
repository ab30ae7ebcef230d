"""Every named pool of the library has a poison class (poreseq_amd/csrc/ps_poison.h): the names csrc passes to Runtime::buf() and
Runtime::hbuf() are exactly the table's.  A pool added without a class — or fetched under a name the scan cannot see — fails here,
without a GPU.  VALUE is the class that needs an argument, so every VALUE entry must carry one."""
import glob
import os
import re

import backends as B

CSRC = os.path.join(B.ROOT, "poreseq_amd", "csrc")
CLASSES = ("INDEX", "VALUE", "EXEMPT")
VALUE_CANDIDATES = {"cmax", "pm", "best", "mutdbl", "like_out", "vit_lik"}


def sources():
    return sorted(p for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".cpp", ".hip", ".h")))


def table():
    """name -> (class, reason) from POISON_TABLE"""
    text = open(os.path.join(CSRC, "ps_poison.h")).read()
    body = text[text.index("POISON_TABLE[] = {"):]
    body = body[:body.index("\n};")]
    rows = re.findall(r'^\s*\{"(\w+)",\s*PoisonClass::(\w+),\s*"([^"]*)"\},?\s*$', body, flags=re.M)
    lines = [ln for ln in body.splitlines()[1:] if ln.strip() and not ln.strip().startswith("//")]
    assert len(rows) == len(lines), "a line of POISON_TABLE is not of the form {\"name\", PoisonClass::X, \"reason\"},"
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return {n: (c, why) for n, c, why in rows}


def used():
    """(names passed to buf(), names passed to hbuf(), every other call of either) over csrc"""
    dev, host, opaque = set(), set(), []
    for path in sources():
        text = open(path).read()
        dev |= set(re.findall(r'\bbuf\("(\w+)"\)', text))
        host |= set(re.findall(r'\bhbuf\("(\w+)"\)', text))
        for m in re.finditer(r'(?:->|\.)h?buf\(([^)]*)\)', text):
            if not re.fullmatch(r'"\w+"', m.group(1).strip()):
                opaque.append("%s: %s" % (os.path.basename(path), m.group(0)))
    return dev, host, opaque


def test_every_pool_name_has_a_class_and_the_table_names_no_other():
    t = table()
    dev, host, opaque = used()
    assert not opaque, "pools fetched under a name that is not a string literal: %s" % opaque
    assert len(dev) >= 40 and host, (len(dev), host)      # the scan found the pools (about 50 today)
    assert dev | host == set(t), sorted((dev | host) ^ set(t))
    assert all(c in CLASSES for c, _ in t.values())


def test_value_entries_are_the_argued_ones():
    t = table()
    value = {n for n, (c, _) in t.items() if c == "VALUE"}
    assert value <= VALUE_CANDIDATES, sorted(value - VALUE_CANDIDATES)
    assert "rec" not in value and "flg" not in value       # the Viterbi arena's back-pointers and the step words are followed
    for n in value | {n for n, (c, _) in t.items() if c == "EXEMPT"}:
        assert len(t[n][1]) >= 20, (n, t[n][1])


def test_python_names_the_classes_as_the_header_does():
    from poreseq_amd import _capi
    text = open(os.path.join(CSRC, "ps_poison.h")).read()
    enum = re.search(r"enum class PoisonClass \{([^}]*)\}", text).group(1)
    assert [(k.strip(), int(v)) for k, v in (kv.split("=") for kv in enum.split(","))] == list(zip(_capi.POISON_CLASSES, range(3)))
    assert "ps_debug_poison" in _capi.OPTIONAL and "ps_debug_poison" in B.oracle_api().missing
