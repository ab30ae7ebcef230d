"""The calls that align every event to its AlignData's own sequence, forward only — ScoreEvents, AlignStats, KmerStats — through the
cuts of a lock-step call: the share chunks, the halves after a realignment whose bands or step codes came out over the share, and the
k-mer call's halving when its tables exceed the share.  test_batch.py takes ScoreEvents through a tiny budget inside a consensus
run; here the two statistics calls go through every cut as well, with and without a realignment, on the three regions of
test_batch._split_case (an odd count: unequal halves; the middle region without events).  Every cut child returns the bytes of the
child that was not cut, that one the bytes of region-by-region PSAlign calls and of util's definitions, no child leaves anything
behind in the regions, and traces and launch counts say that the cuts happened.  Child processes, as PORESEQ_NO_SWEEP and
PORESEQ_DEBUG_GUESS_P are read once per process."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import backends as B
import kmer_cases as K
from poreseq_amd import util
from poreseq_amd.poreseqcpp import PSAlign
from test_batch import _split_case, P

pytestmark = pytest.mark.gpu

# PORESEQ_MAX_BATCH_GB of the cut children.  A forward-only k_fill job at the 64 slots of the `dense` child's guess takes
# (n0 + C + 1 + 24) * 64 * 18 bytes (matrix_bytes, ps_plan.h): about 2.5 MB for the four events of region 0, 3.6 MB for the five of
# region 2.
# DENSE: 6.1 MB for the three.  The trace at 0.008 and 0.006: no share cut, realign finds the nine jobs over the share at the 320
#   slots of their real footprint and halves (realign lines of 9, 4, 5, 5 jobs).  At 0.005, 0.004 and 0.003: share_cut sends 2 + 1,
#   and the sub-batch of two is halved when realign finds it over 1.2 x the share (4, 4, 5 jobs, one "split" per call): both cuts.
# CODES: with PORESEQ_SWEEP_MIN=0 the nine events take the strip sweep.  share_need guesses their step codes at the strip height of
#   one wavefront per sweep, K = 10 at realign_width 300: 2.01 MB, while the launch runs K = 2 on four wavefronts, 1.88 MB — the real
#   codes are smaller than the guess, so no budget gives the line (the trace from 0.02 down to 0.0021: nine jobs, no split; from
#   0.002 down the share cut sends every region alone, which realign never splits).  As in test_batch, PORESEQ_DEBUG_SWEEP_K=4 makes
#   the guess a wrong one: 1.15 * 256 bytes * 3087 steps = 908.8 kB guessed at K = 4, 384 bytes * 2883 steps = 1107.1 kB at the
#   K = 6 the sweep settles on.  The line appears for 908.8 kB <= budget < 1107.1 / 1.2 = 922.6 kB (the trace at 0.001: nine jobs,
#   no split; at 0.0009: the share cut).
# TABLES: 3 * 1024 * 48 bytes per region, 442 kB for three and 295 kB for two.  The trace at 0.0005 and 0.00045: one k_kmer_stats
#   launch for the call without a realignment; at 0.0004 and 0.0003: two (1 + 2 regions), k_align_stats still one.  (The calls with a
#   realignment are cut into single regions by the share at all four.)
SPLIT_DENSE_GB, SPLIT_CODES_GB, SPLIT_TABLES_GB = "0.004", "0.000915", "0.0004"

_HERE = os.path.dirname(os.path.abspath(__file__))
# the child process: calls 1 to 5 on one RegionBatch, the launch counts after each of calls 2 to 5, the regions after close()
_CHILD = (
    "import copy, pickle, sys\n"
    "sys.path[:0] = [%r, %r]\n"
    "import backends as B\n"
    "from test_batch import _split_case, P\n"
    "from poreseq_amd import _capi\n"
    "from poreseq_amd.batch import RegionBatch\n"
    "from poreseq_amd.poreseqcpp import PSAlign\n"
    "api = _capi.load_hip()\n"
    "regs, _, _, groups = _split_case()\n"
    "pas = [B.make_pa(PSAlign, d, copy.deepcopy(ev), P) for d, ev in regs]\n"
    "rb = RegionBatch(pas)\n"
    "out = {'launches': []}\n"
    "def counted(key, call):\n"
    "    n0 = [api.prof_get(k)[1] for k in ('align_stats', 'kmer_stats')]\n"
    "    out[key] = call()\n"
    "    out['launches'].append(tuple(api.prof_get(k)[1] - n for k, n in zip(('align_stats', 'kmer_stats'), n0)))\n"
    "try:\n"
    "    out['score'] = rb.ScoreEvents()\n"
    "    api.prof_enable(1)\n"
    "    api.prof_reset()\n"
    "    try:\n"
    "        counted('astats_re', lambda: rb.AlignStats(realign=True))\n"
    "        counted('kstats_re', lambda: rb.KmerStats(groups=groups, n_groups=3, realign=True))\n"
    "        counted('astats', lambda: rb.AlignStats(realign=False))\n"
    "        counted('kstats', lambda: rb.KmerStats(groups=groups, n_groups=3, realign=False))\n"
    "    finally:\n"
    "        api.prof_enable(0)\n"
    "finally:\n"
    "    rb.close()\n"
    "out['state'] = [(pa.sequence, [ev.ref_align.tobytes() for ev in pa.events], [ev.ref_like.tobytes() for ev in pa.events]) for pa in pas]\n"
    "pickle.dump(out, open(sys.argv[1], 'wb'))\n"
) % (os.path.dirname(_HERE), _HERE)
STATS = ("astats_re", "kstats_re", "astats", "kstats")     # calls 2 to 5, the order of out["launches"]


def run_child(path, extra):
    """(the child's dict, its stderr) under PORESEQ_TRACE=1 and the knobs `extra`"""
    env = dict(os.environ, PORESEQ_TRACE="1", **extra)
    r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(path, "rb") as f:
        return pickle.load(f), r.stderr


def realign_jobs(err):
    """the job counts of the trace's `[ps] realign ...: N jobs x D` lines"""
    return [int(m.group(1)) for m in re.finditer(r"^\[ps\] realign[^\n]*?: (\d+) jobs x \d", err, re.M)]


def split_lines(err):
    return [l for l in err.splitlines() if l.startswith("[ps] realign") and "over the share: split" in l]


def _bytes(x):
    return None if x is None else np.ascontiguousarray(x).tobytes()


def results(out):
    """every output of the five calls as bytes: [call][region] -> (scores, records or table)"""
    return [[_bytes(np.asarray(s, dtype=np.float64)) for s in out["score"]]] + [[(_bytes(sc), _bytes(rec)) for sc, rec in out[k]] for k in STATS]


def test_score_and_stats_calls_survive_being_cut_into_sub_batches(tmp_path):
    """Four child processes, a few seconds in all on an MI355X."""
    plain, err0 = run_child(str(tmp_path / "plain.pkl"), {})
    dense, err1 = run_child(str(tmp_path / "dense.pkl"), {"PORESEQ_DEBUG_GUESS_P": "64", "PORESEQ_NO_SWEEP": "1", "PORESEQ_MAX_BATCH_GB": SPLIT_DENSE_GB})
    codes, err2 = run_child(str(tmp_path / "codes.pkl"), {"PORESEQ_SWEEP_MIN": "0", "PORESEQ_DEBUG_SWEEP_K": "4", "PORESEQ_MAX_BATCH_GB": SPLIT_CODES_GB})
    tables, err3 = run_child(str(tmp_path / "tables.pkl"), {"PORESEQ_MAX_BATCH_GB": SPLIT_TABLES_GB})
    for name, out, err in (("plain", plain, err0), ("dense", dense, err1), ("codes", codes, err2), ("tables", tables, err3)):
        print("%s: launches (align_stats, kmer_stats) of calls 2 to 5 %s; realign jobs %s" % (name, out["launches"], realign_jobs(err)))
        print("\n".join(l for l in err.splitlines() if "over the share" in l))

    # ---- that the cuts happened, and that the plain child had none
    assert realign_jobs(err0) and set(realign_jobs(err0)) == {9} and "over the share" not in err0
    assert plain["launches"] == [(1, 0), (0, 1), (1, 0), (0, 1)]
    # full matrices: the share cut, and a sub-batch halved when its bands turn out wider than the guess
    assert min(realign_jobs(err1)) < 9 and any("of matrices" in l for l in split_lines(err1))
    assert dense["launches"][0][0] > 1 and dense["launches"][1][1] > 1
    # step codes of a strip sweep over the share
    assert any("of step codes" in l for l in split_lines(err2))
    # tables over the share: the k-mer call alone is halved, with and without a realignment
    assert tables["launches"][2] == (1, 0) and tables["launches"][3] == (0, 2) and tables["launches"][1] == (0, 2)
    assert not split_lines(err3)

    # ---- every cut child: the bytes of the plain one, and the regions as they went in
    regs, _, _, groups = _split_case()
    state = [(d, [ev.ref_align.tobytes() for ev in evs], [ev.ref_like.tobytes() for ev in evs]) for d, evs in regs]
    for name, out in (("plain", plain), ("dense", dense), ("codes", codes), ("tables", tables)):
        assert results(out) == results(plain), name
        assert out["state"] == state, name           # the calls only score

    # ---- the plain child against region-by-region PSAlign calls, and the calls without a realignment against the definitions
    for k, (d, evs) in enumerate(regs):
        pa = B.make_pa(PSAlign, d, evs, P)
        one = [_bytes(np.asarray(pa.ScoreEvents(), dtype=np.float64))]
        one += [(_bytes(sc), _bytes(rec)) for sc, rec in (pa.AlignStats(realign=True), pa.KmerStats(groups[k], 3, realign=True),
                                                          pa.AlignStats(realign=False), pa.KmerStats(groups[k], 3, realign=False))]
        assert [r[k] for r in results(plain)] == one, k
        st = K.states_of(d)
        sc, rec = plain["astats"][k]
        assert sc is None and rec.shape == (len(evs),)
        want = [util.align_stats_from_refs(st, ev.mean, ev.ref_align, ev.model.level_mean, ev.model.level_stdv) for ev in evs]
        assert rec.tobytes() == b"".join(w.tobytes() for w in want), k
        sc, tab = plain["kstats"][k]
        assert sc is None and tab.shape == (3, 1024)
        assert tab.tobytes() == util.kmer_stats_from_refs(st, evs, [ev.ref_align for ev in evs], groups[k], 3).tobytes(), k
        assert len(plain["score"][k]) == len(evs) and plain["astats_re"][k][0].shape == (len(evs),) and plain["kstats_re"][k][0].shape == (len(evs),)
    # the region without events: zero-length scores, zero records, an all-zero table
    assert plain["score"][1] == [] and all(plain[c][1][1].shape == (0,) for c in ("astats_re", "astats"))
    assert all(plain[c][1][1].tobytes() == bytes(3 * 1024 * 48) for c in ("kstats_re", "kstats"))
    assert any(plain["kstats"][k][1]["n"].any() for k in (0, 2))
