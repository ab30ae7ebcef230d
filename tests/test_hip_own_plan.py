"""The two own-sequence statistics that were added after test_hip_own_chain.py — MoveStats and PosteriorStats with their per-level
arrays — through the cuts of a lock-step call, and through calls whose regions want different outputs.  The regions are the three of
test_batch._split_case (4, 0 and 5 events) with one event of zero levels put between the events of region 0, so that two consecutive
jobs share a level offset in the per-level arrays.  Every cut child returns the bytes of the child that was not cut, that one the
bytes of region-by-region PSAlign calls, no child leaves anything behind in the regions, and the launch counts (and the trace of the
strip sweep) say that the cuts happened.  Child processes, as PORESEQ_NO_SWEEP, PORESEQ_DEBUG_GUESS_P and PORESEQ_DEBUG_SWEEP_K are
read once per process; PORESEQ_MAX_BATCH_GB is read at every call, so a child sets it per call."""
import copy
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import backends as B
import ref_cases
from poreseq_amd import _capi
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign
from test_batch import _split_case, P

pytestmark = pytest.mark.gpu

# The regions: C = 254, 213 and 293 states; levels (248, 0, 242, 236, 243), none, (292, 286, 284, 272, 277).  realign_width 300.
#
# POSTERIOR.  The records of a job take (n0 + C + 1 + 24) x P x 16 bytes at P slots per anti-diagonal (post_need in ps_own.cpp,
#   matrix_cells in ps_plan.h).  The sums of n0 + C + 25: 2364 for the five events of region 0, 3001 for the five of region 2, 5365
#   together.  The widest footprint of these bands is 292 rows (realign's trace: "widest footprint"), P = 320 slots.
#   SHARE: without PORESEQ_DEBUG_GUESS_P the guess is guess_slots_w(300) = 384 slots, 6144 bytes per anti-diagonal: 14.52 MB, 0 and
#     18.44 MB, 32.96 MB together.  At 25 MB share_cut sends regions 0 + 1, then region 2 (the largest fits alone: a lone region
#     over its share is refused, not cut); the real tables are smaller than the guess, so nothing is halved: 2 launches of k_post_fwd.
#   HALVING: with PORESEQ_DEBUG_GUESS_P=64 the guess is 1024 bytes per anti-diagonal, 5.49 MB for all: no share cut from there up.
#     The real tables take 5120 bytes per anti-diagonal: 15.37 MB for region 2 and 27.47 MB for all.  post_place answers PS_SPLIT for
#     the three when 27.47 MB > 1.2 B, and places every half when 15.37 MB <= B: 15.37 MB <= B < 22.89 MB.  The halves are region 0
#     alone and regions 1 + 2: 2 launches of k_post_fwd, with no share cut before them.
#   REFUSAL: region 2 alone at 5 MB, below its real tables at either footprint.
# MOVES, step codes of a strip sweep (PORESEQ_SWEEP_MIN=0, PORESEQ_DEBUG_SWEEP_K=4: a wrong guess, as in test_hip_own_chain.py).  A
#   job's codes take C + ceil(n0 / K) + 1 steps of 64 K bytes in share_need's guess and C + ceil(n0 / K) steps in sweep_prepare.
#   Guessed at K = 4: 3087 steps for the nine events with levels + 255 for the one without = 3342, x 256 bytes x 1.15 = 983.9 kB.
#   Real at the K = 6 the sweep settles on: 2883 + 254 = 3137 steps x 384 bytes = 1204.6 kB.  The line "of step codes ... over the
#   share: split" appears for 983.9 kB <= B < 1204.6 / 1.2 = 1003.8 kB; the halves are region 0 alone and regions 1 + 2: 2 launches
#   of k_move_stats.  (The posterior call of that child runs without a budget: at 1 MB every lone region would be refused.)
SHARE_GB, HALVE_GB, CODES_GB, REFUSE_GB = "0.025", "0.017", "0.000994", "0.005"
COUNTED = ("move_stats", "post_fwd", "post_bwd")
_HERE = os.path.dirname(os.path.abspath(__file__))


def regions():
    """_split_case's regions, an event of zero levels behind the first event of region 0"""
    regs = _split_case()[0]
    d, evs = regs[0]
    none = ref_cases.levels_cut([copy.deepcopy(evs[1])], 0)[0]
    regs[0] = (d, [evs[0], none] + list(evs[1:]))
    return regs


def _bytes(x):
    return np.ascontiguousarray(x).tobytes()


def moves_bytes(r):
    """one region's MoveStats(levels=True) as bytes: (scores, records, [step], [col])"""
    return (_bytes(r[0]), _bytes(r[1]), [_bytes(a) for a in r[2]], [_bytes(a) for a in r[3]])


def post_bytes(r):
    """one region's PosteriorStats(levels=True) as bytes: (records, [emit], [col])"""
    return (_bytes(r[0]), [_bytes(a) for a in r[1]], [_bytes(a) for a in r[2]])


def _budget(gb):
    if gb:
        os.environ["PORESEQ_MAX_BATCH_GB"] = gb
    else:
        os.environ.pop("PORESEQ_MAX_BATCH_GB", None)


def _event_ptrs(arrs, ptype):
    """one region's [E] array of pointers, and that array as the pointer the C ABI takes"""
    arr = (ptype * max(len(arrs), 1))(*[a.ctypes.data_as(ptype) for a in arrs])
    return arr, C.cast(arr, C.POINTER(ptype))


def mixed_wants(api, regs):
    """ps_batch_move_stats with step of region 0 and col of region 2 only, ps_batch_posterior_stats with emit + col of region 0
    only, on fresh handles -> what came back, as bytes"""
    nl = [[ev.mean.size for ev in evs] for _, evs in regs]
    R = len(regs)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = {}
    hs = [api.align_create(d, copy.deepcopy(evs), P) for d, evs in regs]
    try:
        recs = [np.zeros(max(len(n), 1), dtype=_capi.EVENT_MOVES) for n in nl]
        scores = [np.zeros(max(len(n), 1)) for n in nl]
        step0 = [np.zeros(max(v, 1), dtype=np.uint8) for v in nl[0]]
        col2 = [np.zeros(max(v, 1), dtype=np.int32) for v in nl[2]]
        keep_s, ps = _event_ptrs(step0, _capi.c_u8p)
        keep_c, pc = _event_ptrs(col2, _capi.c_i32p)
        stp = (C.POINTER(_capi.c_u8p) * R)()
        clp = (C.POINTER(_capi.c_i32p) * R)()
        stp[0], clp[2] = ps, pc
        api.check(api.lib.ps_batch_move_stats(R, api._harr(hs), (_capi.c_dp * R)(*[_capi._dp(a) for a in scores]),
                                              (C.c_void_p * R)(*[vp(r) for r in recs]), stp, clp))
        out["moves"] = [(_bytes(s[:len(n)]), _bytes(r[:len(n)])) for s, r, n in zip(scores, recs, nl)]
        out["step0"] = [_bytes(a[:v]) for a, v in zip(step0, nl[0])]
        out["col2"] = [_bytes(a[:v]) for a, v in zip(col2, nl[2])]
    finally:
        for h in hs:
            api.align_destroy(h)
    hs = [api.align_create(d, copy.deepcopy(evs), P) for d, evs in regs]
    try:
        recs = [np.zeros(max(len(n), 1), dtype=_capi.EVENT_POSTERIOR) for n in nl]
        emit0 = [np.zeros(max(v, 1)) for v in nl[0]]
        pcol0 = [np.full(max(v, 1), np.nan) for v in nl[0]]
        keep_e, pe = _event_ptrs(emit0, _capi.c_dp)
        keep_p, pp = _event_ptrs(pcol0, _capi.c_dp)
        emp = (C.POINTER(_capi.c_dp) * R)()
        plp = (C.POINTER(_capi.c_dp) * R)()
        emp[0], plp[0] = pe, pp
        api.check(api.lib.ps_batch_posterior_stats(R, api._harr(hs), (C.c_void_p * R)(*[vp(r) for r in recs]), emp, plp))
        out["post"] = [_bytes(r[:len(n)]) for r, n in zip(recs, nl)]
        out["emit0"] = [_bytes(a[:v]) for a, v in zip(emit0, nl[0])]
        out["pcol0"] = [_bytes(a[:v]) for a, v in zip(pcol0, nl[0])]
    finally:
        for h in hs:
            api.align_destroy(h)
    del keep_s, keep_c, keep_e, keep_p
    return out


def refusal(api, region):
    """one region under a budget below its real posterior tables -> (the error's text, launches of the refused call, what the
    handle scores afterwards)"""
    d, evs = region
    h = api.align_create(d, copy.deepcopy(evs), P)
    try:
        n0 = [api.prof_get(k)[1] for k in COUNTED]
        _budget(REFUSE_GB)
        try:
            api.posterior_stats(h, [ev.mean.size for ev in evs], True)
            text = None
        except _capi.PoreseqError as err:
            text = str(err)
        finally:
            _budget(None)
        launched = tuple(api.prof_get(k)[1] - n for k, n in zip(COUNTED, n0))
        return text, launched, _bytes(api.score_alignments(h, len(evs)))
    finally:
        api.align_destroy(h)


def child(path, moves_gb, post_gb, extras):
    """the child process: the two calls on one RegionBatch, each under its budget ("" for none), the launch counts of each, the
    regions after close(); extras: the mixed wants and the refusal as well"""
    api = _capi.load_hip()
    regs = regions()
    pas = [B.make_pa(PSAlign, d, copy.deepcopy(evs), P) for d, evs in regs]
    out = {"launches": {}}

    def counted(key, gb, call):
        n0 = [api.prof_get(k)[1] for k in COUNTED]
        _budget(gb)
        try:
            out[key] = call()
        finally:
            _budget(None)
        out["launches"][key] = tuple(api.prof_get(k)[1] - n for k, n in zip(COUNTED, n0))

    api.prof_enable(1)
    api.prof_reset()
    try:
        rb = RegionBatch(pas)
        try:
            counted("moves", moves_gb, lambda: [moves_bytes(r) for r in rb.MoveStats(levels=True)])
            counted("post", post_gb, lambda: [post_bytes(r) for r in rb.PosteriorStats(levels=True)])
        finally:
            rb.close()
        if extras:
            out["mixed"] = mixed_wants(api, regs)
            out["refusal"] = refusal(api, regs[2])
    finally:
        api.prof_enable(0)
    out["state"] = [(pa.sequence, [ev.ref_align.tobytes() for ev in pa.events], [ev.ref_like.tobytes() for ev in pa.events]) for pa in pas]
    with open(path, "wb") as f:
        pickle.dump(out, f)


def run_child(path, env, moves_gb="", post_gb="", extras=False):
    """(the child's dict, its stderr) under PORESEQ_TRACE=1 and the knobs `env`"""
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_hip_own_plan as T\nT.child(%r, %r, %r, %r)\n" % (
        os.path.dirname(_HERE), _HERE, path, moves_gb, post_gb, extras)
    full = dict(os.environ, PORESEQ_TRACE="1", **env)
    full.pop("PORESEQ_MAX_BATCH_GB", None)
    r = subprocess.run([sys.executable, "-c", code], env=full, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(path, "rb") as f:
        return pickle.load(f), r.stderr


def split_lines(err):
    return [l for l in err.splitlines() if l.startswith("[ps] realign") and "over the share: split" in l]


def test_move_and_posterior_calls_survive_cuts_and_mixed_wants(tmp_path):
    """Four child processes, a few seconds in all on an MI355X."""
    plain, err0 = run_child(str(tmp_path / "plain.pkl"), {}, extras=True)
    share, err1 = run_child(str(tmp_path / "share.pkl"), {}, SHARE_GB, SHARE_GB)
    halve, err2 = run_child(str(tmp_path / "halve.pkl"), {"PORESEQ_DEBUG_GUESS_P": "64"}, HALVE_GB, HALVE_GB)
    codes, err3 = run_child(str(tmp_path / "codes.pkl"), {"PORESEQ_SWEEP_MIN": "0", "PORESEQ_DEBUG_SWEEP_K": "4"}, CODES_GB, "")
    children = (("plain", plain, err0), ("share", share, err1), ("halve", halve, err2), ("codes", codes, err3))
    for name, out, err in children:
        print("%s: launches %s of the MoveStats call %s, of the PosteriorStats call %s" % (name, COUNTED, out["launches"]["moves"], out["launches"]["post"]))
        print("\n".join(l for l in err.splitlines() if "over the share" in l or "widest footprint" in l))

    # ---- that the cuts happened, and that the plain child had none
    assert plain["launches"] == {"moves": (1, 0, 0), "post": (0, 1, 1)} and "over the share" not in err0
    assert share["launches"]["post"][0] == 0 and share["launches"]["post"][1] > 1 and share["launches"]["post"][2] > 1
    assert halve["launches"]["post"] == (0, 2, 2)            # post_place's PS_SPLIT alone: region 0 | regions 1 + 2
    assert codes["launches"]["moves"] == (2, 0, 0) and codes["launches"]["post"] == (0, 1, 1)
    assert any("of step codes" in l for l in split_lines(err3))

    # ---- every cut child: the bytes of the plain one, and the regions as they went in
    regs = regions()
    state = [(d, [ev.ref_align.tobytes() for ev in evs], [ev.ref_like.tobytes() for ev in evs]) for d, evs in regs]
    for name, out, _ in children:
        assert out["moves"] == plain["moves"], name
        assert out["post"] == plain["post"], name
        assert out["state"] == state, name                   # the calls only score

    # ---- the plain child against region-by-region PSAlign calls
    assert regs[0][1][1].mean.size == 0 and [len(evs) for _, evs in regs] == [5, 0, 5]
    for k, (d, evs) in enumerate(regs):
        pa = B.make_pa(PSAlign, d, copy.deepcopy(evs), P)
        assert plain["moves"][k] == moves_bytes(pa.MoveStats(levels=True)), k
        assert plain["post"][k] == post_bytes(pa.PosteriorStats(levels=True)), k
        assert len(plain["moves"][k][2]) == len(evs) and len(plain["post"][k][1]) == len(evs)
    assert plain["moves"][0][2][1] == b"" and plain["post"][0][1][1] == b""      # the event without levels
    assert any(plain["moves"][2][2]) and any(np.frombuffer(b).any() for b in plain["post"][2][1])

    # ---- regions that want different outputs: what was asked for is what the call with everything gave
    mixed = plain["mixed"]
    assert mixed["moves"] == [m[:2] for m in plain["moves"]]
    assert mixed["step0"] == plain["moves"][0][2] and mixed["col2"] == plain["moves"][2][3]
    assert mixed["post"] == [p[0] for p in plain["post"]]
    assert mixed["emit0"] == plain["post"][0][1] and mixed["pcol0"] == plain["post"][0][2]

    # ---- a lone region over its share is refused before any fill is launched, and its handle stays usable
    text, launched, after = plain["refusal"]
    assert text is not None and "(-5)" in text and "posterior: the forward tables of this AlignData need" in text, text   # PS_ERR_NOMEM
    assert launched == (0, 0, 0)
    d, evs = regs[2]
    assert after == _bytes(np.asarray(B.make_pa(PSAlign, d, copy.deepcopy(evs), P).ScoreEvents(), dtype=np.float64))
