"""How the runtimes' streams get hardware queues when HIP runs on its default of four pooled queues per priority level
(ps_runtime.cpp: hwq_mode, private_stream): a CU-masked stream with a queue of its own per runtime while the process-wide budget lasts
(PORESEQ_PRIVATE_QUEUES, default 16, times the device fraction), priority dealing beyond it; plain streams when GPU_MAX_HW_QUEUES >= 8
was in the start-up environment.  The mode is latched per process, so every case runs in a fresh child process under a time limit.
Whatever the arrangement, the lock-step results of several slot threads equal the same regions refined one by one in a single thread
(sequence, accuracy and every event's ref_align, bit for bit): the reference is computed once, with private queues switched off."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NREG = 12   # synth.make_region(300, 5, 7300 + k): five events is the schedule's minimum

CHILD = r"""
import copy, hashlib, json, sys, threading
sys.path[:0] = [%r, %r]
import numpy as np
from poreseq_amd import _capi, synth
from poreseq_amd.consensus import consensus_region, consensus_regions
from poreseq_amd.poreseqcpp import PSAlign, swalign
from poreseq_amd.util import DEFAULT_PARAMS
mode, nthreads, per, alive = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
P = dict(DEFAULT_PARAMS, verbose=0)
api = _capi.load_hip()
digests, infos = {}, []
def as_pa(r):
    pa = PSAlign(); pa.sequence, pa.events, pa.params = r[0], copy.deepcopy(r[1]), dict(P); return pa
def digest(pa, res):
    h = hashlib.sha1(repr((res[0], res[1])).encode())
    for ev in pa.events:
        h.update(np.ascontiguousarray(ev.ref_align).tobytes())
    return h.hexdigest()
regs = []
def first():                 # (the main thread never enters the library: it would own a runtime, and a queue, for good)
    regs[:] = [synth.make_region(300, 5, 7300 + k, swalign, P) for k in range(%d)]
    if mode == "alone":      # one by one, this thread only
        for k, r in enumerate(regs):
            api.srand(1)     # a region's random stream is a fresh process's (dist.run_regions does the same; a lock-step batch seeds each region so)
            pa = as_pa(r)
            digests[k] = digest(pa, consensus_region(pa, P))
def main():
    t = threading.Thread(target=first); t.start(); t.join()
    if mode == "alone":
        return
    def work(t, gate):
        ks = list(range(per * t, per * t + per))
        pas = [as_pa(regs[k %% len(regs)]) for k in ks]
        gate.wait()          # every thread of the wave owns its runtime before any of them leaves
        out = consensus_regions(pas, P)
        for k, pa, res in zip(ks, pas, out):
            digests[k] = digest(pa, res)
        infos.append(api.info())
        gate.wait()
    for t0 in range(0, nthreads, alive):
        gate = threading.Barrier(min(alive, nthreads - t0))
        th = [threading.Thread(target=work, args=(t, gate)) for t in range(t0, min(t0 + alive, nthreads))]
        [t.start() for t in th]; [t.join() for t in th]
main()
print("RESULT " + json.dumps({"digests": digests, "infos": infos, "info": api.info()}))
""" % (os.path.dirname(HERE), HERE, NREG)

_DROP = ("GPU_MAX_HW_QUEUES", "PORESEQ_HWQ_SET_BY_PACKAGE", "PORESEQ_ONE_PRIORITY", "PORESEQ_PRIORITY_LEVELS", "PORESEQ_PRIVATE_QUEUES",
         "PORESEQ_DEVICE_FRACTION")


def child(mode, nthreads, per, alive, **env):
    e = {k: v for k, v in os.environ.items() if k not in _DROP}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, mode, str(nthreads), str(per), str(alive)], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    out["digests"] = {int(k): v for k, v in out["digests"].items()}
    print(mode, nthreads, "x", per, env, "->", out["info"].split(";")[1])
    return out


def queues(info):
    """(private, budget, fell back) from ps_info's line; None when the process is not in the private-queue mode"""
    m = re.search(r"(\d+) private \(budget (\d+)\) on one priority level, (none|\d+) fell back", info)
    return None if m is None else (int(m.group(1)), int(m.group(2)), 0 if m.group(3) == "none" else int(m.group(3)))


@pytest.fixture(scope="module")
def alone():
    """every region refined on its own, one after the other, in a single thread; private queues switched off"""
    return child("alone", 1, 1, 1, GPU_MAX_HW_QUEUES="4", PORESEQ_PRIVATE_QUEUES="0")["digests"]


def same(got, alone, n):
    return sorted(got) == list(range(n)) and all(got[k] == alone[k] for k in range(n))


def test_private_queues_under_a_preset_of_four(alone):
    got = child("threads", 6, 2, 6, GPU_MAX_HW_QUEUES="4")
    assert queues(got["info"]) == (6, 16, 0)
    assert "none fell back" in got["info"] and "on one priority level" in got["info"] and "HIP's default" in got["info"]
    assert same(got["digests"], alone, 12)


def test_budget_of_two_four_threads(alone):
    got = child("threads", 4, 2, 4, GPU_MAX_HW_QUEUES="4", PORESEQ_PRIVATE_QUEUES="2")
    assert queues(got["info"]) == (2, 2, 2)
    assert "2 fell back and are dealt over the priority levels" in got["info"]
    assert same(got["digests"], alone, 8)


def test_budget_follows_the_device_fraction(alone):
    """eight ranks on one GPU plan for an eighth of it each: two of sixteen private queues per process"""
    got = child("threads", 3, 2, 3, GPU_MAX_HW_QUEUES="4", PORESEQ_DEVICE_FRACTION="0.125")
    assert queues(got["info"]) == (2, 2, 1)
    assert same(got["digests"], alone, 6)


def test_start_up_value_of_sixteen_keeps_plain_streams(alone):
    got = child("threads", 6, 2, 6, GPU_MAX_HW_QUEUES="16")
    assert queues(got["info"]) is None and "private" not in got["info"]
    assert "streams: one priority level, a hardware queue per stream (GPU_MAX_HW_QUEUES=16 in the process's start-up environment); device fraction" in got["info"]
    assert same(got["digests"], alone, 12)


def test_thread_churn_does_not_grow_the_count(alone):
    """twelve short-lived threads, three alive at a time: a thread that leaves hands its runtime, stream included, to the next"""
    got = child("threads", 12, 1, 3, GPU_MAX_HW_QUEUES="4")
    seen = [queues(i) for i in got["infos"]]
    assert len(seen) == 12 and all(q is not None and q[0] <= 3 and q[2] == 0 for q in seen)
    assert queues(got["info"]) == (3, 16, 0)
    assert same(got["digests"], alone, 12)


def test_budget_zero_is_the_dealing_of_before(alone):
    got = child("threads", 6, 2, 6, GPU_MAX_HW_QUEUES="4", PORESEQ_PRIVATE_QUEUES="0")
    assert queues(got["info"]) is None
    assert "streams dealt over the priority levels (HIP's default of 4 hardware queues per level" in got["info"] and "PORESEQ_PRIVATE_QUEUES=0" in got["info"]
    assert same(got["digests"], alone, 12)
