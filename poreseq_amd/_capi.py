"""ctypes binding of the C ABI declared in include/poreseq_hip.h.

`CApi(path)` binds *a* shared library that exports that ABI; the product only ever
binds `poreseq_amd/csrc/libporeseq_hip.so` (see `load_hip`), and raises if it is
missing — there is no CPU fallback.  (The test-suite binds the oracle / reference
shims through the same class, from tests/, never from here.)
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.path.join(_HERE, "csrc", "libporeseq_hip.so")

c_dp = C.POINTER(C.c_double)
c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_u8p = C.POINTER(C.c_uint8)
c_i16p = C.POINTER(C.c_int16)


class PsParams(C.Structure):
    # AlignParams, cpp/AlignUtil.h:57-66
    _fields_ = [("lik_offset", C.c_double), ("scoring_width", C.c_int32),
                ("realign_width", C.c_int32), ("verbose", C.c_int32)]


class PsSwSummary(C.Structure):
    # ps_sw_summary, include/poreseq_hip.h
    _fields_ = [(k, C.c_int32) for k in ("score", "n_pairs", "n_match", "first1", "first2", "last1", "last2", "gap1", "gap2")] + \
               [("accuracy", C.c_double)]


class PsPointBest(C.Structure):
    # ps_point_best, include/poreseq_hip.h
    _fields_ = [("margin", C.c_double), ("slot", C.c_int32), ("n_positive", C.c_int32)]


# the same record as a numpy dtype (16 bytes, no padding): what point_table / batch_point_table hand out
POINT_BEST = np.dtype([("margin", np.float64), ("slot", np.int32), ("n_positive", np.int32)])
POINT_SLOTS = 9   # deletion, substitution by A / C / G / T, insertion of A / C / G / T


class PsEditSupport(C.Structure):
    # ps_edit_support, include/poreseq_hip.h
    _fields_ = [("sum", C.c_double), ("cover", C.c_int32), ("pos", C.c_int32), ("neg", C.c_int32), ("reserved", C.c_int32)]


# the same record as a numpy dtype (24 bytes, no padding): what score_mutation_support / batch_score_mutation_support hand out
EDIT_SUPPORT = np.dtype([("sum", np.float64), ("cover", np.int32), ("pos", np.int32), ("neg", np.int32), ("reserved", np.int32)])
SUPPORT_MAX_GROUPS = 8
GENO_MAX_FRAC = 8   # alt fractions per ps_score_mutation_genotypes call
# the records of ps_score_mutation_phase as numpy dtypes (32, 16 and 24 bytes, no padding): ps_edit_link per (site, w), ps_edit_phase
# per site, ps_event_hap per (event, phase set)
EDIT_LINK = np.dtype([("cis", np.float64), ("trans", np.float64), ("n_both", np.int32), ("n_cis", np.int32), ("n_trans", np.int32), ("reserved", np.int32)])
EDIT_PHASE = np.dtype([("vote", np.float64), ("hap", np.int32), ("set", np.int32)])
EVENT_HAP = np.dtype([("lik1", np.float64), ("lik2", np.float64), ("n1", np.int32), ("n2", np.int32)])
LINK_MAX_WINDOW = 8
PHASE_MAX_SETS = 8
# ps_event_stats (112 bytes, no padding): one event's alignment census and the sums of its scaling fit, what align_stats /
# batch_align_stats hand out
EVENT_STATS = np.dtype([(k, np.int32) for k in ("n_levels", "n_aligned", "n_insert", "n_unaligned", "n_step", "n_stay", "n_extend", "n_jump",
                                                "n_back", "n_nostate", "n_fit", "first_col", "last_col", "reserved")] +
                       [("n_gap_cols", np.int64)] + [(k, np.float64) for k in ("sw", "swm", "swmm", "swr", "swmr", "swrr")])

# ps_event_moves (64 bytes, no padding): one event's backtrace moves, what move_stats / batch_move_stats hand out
EVENT_MOVES = np.dtype([(k, np.int32) for k in ("n_levels", "inert", "top_level", "top_col", "low_level", "low_col", "end_kind", "n_match", "n_ignore",
                                                "n_insert", "n_stay", "n_extend", "n_skip_runs", "max_skip")] + [("n_skip_cols", np.int64)])
MOVE_NAMES = ("", "MATCH", "INSERT", "IGNORE", "STAY", "EXTEND")   # the step codes of the per-level array (0: not on the path)
# ps_event_posterior (80 bytes, no padding): one event's sum over all alignments in its band and the expected moves under it, what
# posterior_stats / batch_posterior_stats hand out
EVENT_POSTERIOR = np.dtype([(k, np.int32) for k in ("n_levels", "inert", "n_cols", "pad")] + [("n_cells", np.int64)] +
                           [(k, np.float64) for k in ("logz", "e_skip", "e_match", "e_ignore", "e_insert", "e_stay", "e_extend")])
POSTERIOR_COUNTS = ("e_skip", "e_match", "e_ignore", "e_insert", "e_stay", "e_extend")

# ps_kmer_cell (48 bytes, no padding): one (event group, 5-mer state) of the tables kmer_stats / batch_kmer_stats hand out
KMER_STATS = np.dtype([("n", np.int64)] + [(k, np.float64) for k in ("sz", "szz", "sp", "spu", "spv")])
KMER_MAX_GROUPS = 256
KMER_TILE = 512      # levels k_kmer_stats stages per step (csrc/ps_internal.h); the tests put events on both sides of its edges


class PsPoisonReport(C.Structure):
    # ps_poison_report, include/poreseq_hip.h
    _fields_ = [("name", C.c_char * 32), ("bytes", C.c_int64), ("cls", C.c_int32), ("skipped", C.c_int32)]


PoisonReport = collections.namedtuple("PoisonReport", "bytes cls skipped")
POISON_CLASSES = ("INDEX", "VALUE", "EXEMPT")   # PoisonClass, csrc/ps_poison.h
POISON_1E300 = int(np.float64(1e300).view(np.uint64))   # the bits of +1e300: finite, wins every max, wrecks every sum


class PoreseqError(Exception):
    pass


# every exported symbol with (restype, argtypes); tests check the library exports all of them
SYMBOLS = {
    "ps_last_error": (C.c_char_p, []),
    "ps_backend_name": (C.c_char_p, []),
    "ps_info": (C.c_int, [C.c_char_p, C.c_int64]),
    "ps_align_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_char_p, C.c_int64, C.c_int32, c_i64p,
                                  c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, C.c_char_p, c_i64p,
                                  C.POINTER(PsParams)]),
    "ps_align_destroy": (None, [C.c_void_p]),
    "ps_align_set_scoring_width": (C.c_int, [C.c_void_p, C.c_int32]),
    "ps_align_new_call": (C.c_int, [C.c_void_p, C.c_int32]),
    "ps_align_keep_refs": (C.c_int, [C.c_void_p]),
    "ps_align_n_events": (C.c_int32, [C.c_void_p]),
    "ps_align_n_levels": (C.c_int64, [C.c_void_p, C.c_int32]),
    "ps_align_sequence_length": (C.c_int64, [C.c_void_p]),
    "ps_align_get_sequence": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "ps_align_get_event_refs": (C.c_int, [C.c_void_p, C.c_int32, c_dp, c_dp]),
    "ps_muts_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int64, c_i32p, c_i64p, C.c_char_p,
                                 c_i64p, C.c_char_p, c_dp]),
    "ps_muts_destroy": (None, [C.c_void_p]),
    "ps_muts_count": (C.c_int64, [C.c_void_p]),
    "ps_muts_orig_bytes": (C.c_int64, [C.c_void_p]),
    "ps_muts_mut_bytes": (C.c_int64, [C.c_void_p]),
    "ps_muts_export": (C.c_int, [C.c_void_p, c_i32p, c_i64p, C.c_char_p, c_i64p, C.c_char_p, c_dp]),
    "ps_seqs_destroy": (None, [C.c_void_p]),
    "ps_seqs_count": (C.c_int64, [C.c_void_p]),
    "ps_seqs_bytes": (C.c_int64, [C.c_void_p]),
    "ps_seqs_export": (C.c_int, [C.c_void_p, c_i64p, C.c_char_p]),
    "ps_score_alignments": (C.c_int, [C.c_void_p, c_dp, c_dp]),
    "ps_find_point_mutations": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "ps_find_mutations": (C.c_int, [C.c_void_p, C.c_int32, c_i64p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "ps_score_mutations": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ps_score_sequences": (C.c_int, [C.c_void_p, C.c_int32, c_i64p, C.c_char_p, c_dp, c_dp]),
    "ps_batch_score_sequences": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(c_dp), C.POINTER(c_dp)]),
    "ps_score_mutation_deltas": (C.c_int, [C.c_void_p, C.c_void_p, c_dp]),
    "ps_make_mutations": (C.c_int, [C.c_void_p, C.c_void_p, c_i32p]),
    "ps_point_table": (C.c_int, [C.c_void_p, c_dp, C.POINTER(PsPointBest), C.c_int64]),
    "ps_batch_point_table": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(c_dp), C.POINTER(C.POINTER(PsPointBest)), c_i64p]),
    "ps_score_mutation_support": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, c_i32p, c_dp, C.POINTER(PsEditSupport)]),
    "ps_batch_score_mutation_support": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i32p, C.POINTER(c_i32p), C.POINTER(c_dp),
                                                  C.POINTER(C.POINTER(PsEditSupport))]),
    "ps_score_mutation_genotypes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, c_i32p, C.c_int32, c_dp, c_dp, C.POINTER(PsEditSupport), c_dp, c_i32p]),
    "ps_batch_score_mutation_genotypes": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i32p, C.POINTER(c_i32p), c_i32p, C.POINTER(c_dp),
                                                    C.POINTER(c_dp), C.POINTER(C.POINTER(PsEditSupport)), C.POINTER(c_dp), C.POINTER(c_i32p)]),
    "ps_score_mutation_phase": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, c_dp, C.c_void_p, C.c_void_p, C.c_void_p, c_i32p]),
    "ps_batch_score_mutation_phase": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i32p, c_dp, c_i32p, C.POINTER(c_dp),
                                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(c_i32p)]),
    "ps_align_stats": (C.c_int, [C.c_void_p, C.c_int32, c_dp, C.c_void_p]),
    "ps_batch_align_stats": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(c_dp), C.POINTER(C.c_void_p)]),
    "ps_kmer_stats": (C.c_int, [C.c_void_p, C.c_int32, c_i32p, C.c_int32, c_dp, C.c_void_p]),
    "ps_batch_kmer_stats": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(c_i32p), c_i32p, C.POINTER(c_dp), C.POINTER(C.c_void_p)]),
    "ps_move_stats": (C.c_int, [C.c_void_p, c_dp, C.c_void_p, C.POINTER(c_u8p), C.POINTER(c_i32p)]),
    "ps_batch_move_stats": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(c_dp), C.POINTER(C.c_void_p), C.POINTER(C.POINTER(c_u8p)),
                                      C.POINTER(C.POINTER(c_i32p))]),
    "ps_posterior_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(c_dp), C.POINTER(c_dp)]),
    "ps_batch_posterior_stats": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.POINTER(c_dp)),
                                           C.POINTER(C.POINTER(c_dp))]),
    "ps_debug_posterior": (C.c_int, [C.c_void_p, C.c_int32, c_dp, c_dp]),
    "ps_viterbi_mutate": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double,
                                    C.c_double, C.c_int32, C.POINTER(C.c_void_p)]),
    "ps_srand": (C.c_int, [C.c_uint32]),
    "ps_rand_draw": (C.c_int, [C.c_int64, c_dp]),
    "ps_rng_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32]),
    "ps_rng_destroy": (None, [C.c_void_p]),
    "ps_seqs_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int64, c_i64p, C.c_char_p]),
    "ps_batch_score_alignments": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(c_dp), C.POINTER(c_dp)]),
    "ps_batch_find_mutations": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "ps_batch_score_mutations": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "ps_batch_make_mutations": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i32p]),
    "ps_batch_viterbi_mutate": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32, C.c_double,
                                          C.c_double, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "ps_swfull": (C.c_int, [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, c_i32p, c_dp, c_i32p,
                            c_i32p, C.c_int64, c_i64p]),
    "ps_batch_sw_summary": (C.c_int, [C.c_int64, C.POINTER(C.c_char_p), c_i64p, C.POINTER(C.c_char_p), c_i64p,
                                      C.POINTER(PsSwSummary)]),
    "ps_seq_to_states": (C.c_int, [C.c_char_p, C.c_int64, c_i32p, c_i64p]),
    "ps_debug_fill": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_dp, c_dp, c_u8p, c_u8p]),
    "ps_debug_poison": (C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(PsPoisonReport), C.c_int32, c_i32p]),
    "ps_debug_viterbi": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                   C.c_int64, c_i32p, c_dp, c_i16p, c_dp, c_dp, c_i16p]),
    "ps_debug_viterbi_steps": (C.c_int, [C.c_int32, c_i32p, c_dp, c_dp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                         c_i16p, c_dp, c_dp, c_i16p]),
    "ps_set_sweep_min": (C.c_int, [C.c_int32]),
    "ps_set_sweep2_min": (C.c_int, [C.c_int32]),
    "ps_set_sparse_min": (C.c_int, [C.c_int32]),
    "ps_set_sweep_form": (C.c_int, [C.c_int32, C.c_int32]),
    "ps_set_device_fraction": (C.c_int, [C.c_double]),
    "ps_prof_enable": (C.c_int, [C.c_int32]),
    "ps_prof_reset": (C.c_int, []),
    "ps_prof_get": (C.c_int, [C.c_char_p, c_dp, c_i64p, c_dp]),
    "ps_prof_units": (C.c_int, [C.c_char_p, c_dp]),
}


# entry points of the header that a checker library (the oracle, the reference shim) may lack: CApi serves them from what the
# library does export (sw_summaries from swfull; PSAlign.ScoreSequences runs the reference's loop of Copy / RealignTo / ScoreEvents;
# PSAlign.PointTable builds its arrays from find_point_mutations + score_mutations; PSAlign.ScoreMutationSupport reduces
# score_mutation_deltas and the re-aligned refs on the host, util.support_from_deltas, and PSAlign.ScoreMutationGenotypes does the
# same with util.genotypes_from_deltas on top; PSAlign.ScoreMutationPhase reduces the same two with util.phase_from_deltas;
# PSAlign.AlignStats reduces the refs the library holds with util.align_stats_from_refs, after its score_alignments, and
# PSAlign.KmerStats does the same with util.kmer_stats_from_refs; PSAlign.MoveStats walks the tables of the library's debug_fill
# with util.moves_from_tables; PSAlign.PosteriorStats runs util.posterior_from_emissions — the definition — on the band pattern of
# the library's debug_fill; ps_debug_posterior has no substitute).
# The Viterbi table hooks have no substitute: on a checker built without them the wrappers raise PoreseqError.
OPTIONAL = frozenset(["ps_posterior_stats", "ps_batch_posterior_stats", "ps_debug_posterior", "ps_move_stats", "ps_batch_move_stats", "ps_kmer_stats", "ps_batch_kmer_stats", "ps_align_stats", "ps_batch_align_stats","ps_align_keep_refs", "ps_batch_sw_summary", "ps_score_sequences", "ps_batch_score_sequences", "ps_debug_viterbi", "ps_debug_viterbi_steps", "ps_debug_poison",
                      "ps_point_table", "ps_batch_point_table", "ps_score_mutation_support", "ps_batch_score_mutation_support",
                      "ps_score_mutation_genotypes", "ps_batch_score_mutation_genotypes",
                      "ps_score_mutation_phase", "ps_batch_score_mutation_phase"])

# one pair's Smith-Waterman summary, in terms of swfull's index lists: their length, the matching pairs, entry 0, entry -1, the
# entries with a 0 on either side, and the identity in % (NaN for an empty alignment)
SwSummary = collections.namedtuple("SwSummary", "score n_pairs n_match first1 first2 last1 last2 gap1 gap2 accuracy")


def _dp(a):
    return a.ctypes.data_as(c_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def summary_from_lists(seq1, seq2, score, accuracy, i1, i2):
    """the SwSummary of one swfull result (score, accuracy, inds1, inds2) of seq1 against seq2; n_match counted as the reference
    does (cpp/swlib.cpp:317-319: aligned pairs whose characters are equal)"""
    n = int(len(i1))
    if not n:
        return SwSummary(int(score), 0, 0, 0, 0, 0, 0, 0, 0, float(accuracy))
    i1, i2 = np.asarray(i1), np.asarray(i2)
    both = (i1 > 0) & (i2 > 0)
    c1 = np.frombuffer(seq1.encode("ascii"), dtype=np.uint8)[i1[both] - 1]
    c2 = np.frombuffer(seq2.encode("ascii"), dtype=np.uint8)[i2[both] - 1]
    return SwSummary(int(score), n, int(np.count_nonzero(c1 == c2)), int(i1[0]), int(i2[0]), int(i1[-1]), int(i2[-1]),
                     int(np.count_nonzero(i1 == 0)), int(np.count_nonzero(i2 == 0)), float(accuracy))


class CApi:
    """One loaded library exporting the include/poreseq_hip.h ABI."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise PoreseqError("poreseq_amd: native library not found: %s "
                               "(build it with `python -c 'import __graft_entry__ as g; g.build()'`)" % path)
        self.path = path
        self.lib = C.CDLL(path)
        self.missing = set()
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(self.lib, name)  # AttributeError if the symbol is missing
            except AttributeError:
                if name not in OPTIONAL:
                    raise
                self.missing.add(name)
                continue
            fn.restype = res
            fn.argtypes = args

    # ------------------------------------------------------------------ helpers
    def check(self, rc):
        if rc != 0:
            msg = self.lib.ps_last_error()
            raise PoreseqError("%s failed (%d): %s" % (os.path.basename(self.path), rc,
                                                      msg.decode() if msg else "?"))

    def _need(self, name):
        if name in self.missing:
            raise PoreseqError("%s does not export %s" % (os.path.basename(self.path), name))

    def backend_name(self):
        return self.lib.ps_backend_name().decode()

    def info(self):
        """process-wide state of the library in one line: stream / hardware-queue mode, runtimes, memory plan"""
        buf = C.create_string_buffer(1024)
        self.check(self.lib.ps_info(buf, 1024))
        return buf.value.decode()

    # ------------------------------------------------------------------ AlignData
    def align_create(self, sequence, events, params):
        """Flatten a PSAlign-shaped object (pyx:139-153) and create the native AlignData."""
        E = len(events)
        for ev in events:
            ev.makecontiguous()
        lens = [int(ev.mean.size) for ev in events]
        off = np.zeros(E + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens)
        cat = lambda name: (_f64(np.concatenate([_f64(getattr(ev, name)) for ev in events]))
                            if E else np.zeros(0))
        mean, stdv, ra, rl = cat("mean"), cat("stdv"), cat("ref_align"), cat("ref_like")
        for ev, n in zip(events, lens):
            if not (ev.stdv.size == n and ev.ref_align.size == n and ev.ref_like.size == n):
                raise PoreseqError("event arrays differ in length")
        model = np.zeros((E, 4, 1024), dtype=np.float64)
        trans = np.zeros((E, 4), dtype=np.float64)
        for e, ev in enumerate(events):
            m = ev.model
            model[e, 0], model[e, 1] = _f64(m.level_mean), _f64(m.level_stdv)
            model[e, 2], model[e, 3] = _f64(m.sd_mean), _f64(m.sd_stdv)
            trans[e] = (m.prob_skip, m.prob_stay, m.prob_extend, m.prob_insert)
        evseqs = [(getattr(ev, "sequence", "") or "").encode("ascii") for ev in events]
        eoff = np.zeros(E + 1, dtype=np.int64)
        eoff[1:] = np.cumsum([len(s) for s in evseqs])
        epool = b"".join(evseqs)
        pp = PsParams(4.5, 150, 300, 0)  # AlignParams defaults, cpp/AlignUtil.h:64
        if "verbose" in params:
            pp.verbose = int(params["verbose"])
        if "lik_offset" in params:
            pp.lik_offset = float(params["lik_offset"])
        if "realign_width" in params:
            pp.realign_width = int(params["realign_width"])  # Python float -> C int truncation (pyx:148-151)
        if "scoring_width" in params:
            pp.scoring_width = int(params["scoring_width"])
        seq = sequence.encode("ascii")
        h = C.c_void_p()
        self.check(self.lib.ps_align_create(C.byref(h), seq, len(seq), E, off.ctypes.data_as(c_i64p),
                                            _dp(mean), _dp(stdv), _dp(ra), _dp(rl), _dp(model),
                                            _dp(trans), epool, eoff.ctypes.data_as(c_i64p), C.byref(pp)))
        return h

    def align_destroy(self, h):
        self.lib.ps_align_destroy(h)

    def align_sequence(self, h):
        n = self.lib.ps_align_sequence_length(h)
        buf = C.create_string_buffer(max(int(n), 1))
        self.check(self.lib.ps_align_get_sequence(h, buf, n))
        return buf.raw[:n].decode("ascii")

    def align_update_events(self, h, events):
        """UpdatePythonEvents (pyx:131-137)."""
        for e, ev in enumerate(events):
            n = int(self.lib.ps_align_n_levels(h, e))
            ra = np.empty(n, dtype=np.float64)
            rl = np.empty(n, dtype=np.float64)
            self.check(self.lib.ps_align_get_event_refs(h, e, _dp(ra), _dp(rl)))
            ev.ref_align[:] = ra
            ev.ref_like[:] = rl

    def align_event_refs(self, h, n_events):
        """[ref_align float64 [n]] of every event of the AlignData, as they are now (after a scoring call: re-aligned)"""
        out = []
        for e in range(int(n_events)):
            n = int(self.lib.ps_align_n_levels(h, e))
            ra = np.empty(n, dtype=np.float64)
            rl = np.empty(n, dtype=np.float64)
            self.check(self.lib.ps_align_get_event_refs(h, e, _dp(ra), _dp(rl)))
            out.append(ra)
        return out

    # ------------------------------------------------------------------ mutation lists
    def muts_create(self, muts, with_scores=False):
        n = len(muts)
        start = np.array([int(m.start) for m in muts], dtype=np.int32)
        origs = [m.orig.encode("ascii") for m in muts]
        mutsb = [m.mut.encode("ascii") for m in muts]
        oo = np.zeros(n + 1, dtype=np.int64)
        oo[1:] = np.cumsum([len(s) for s in origs])
        mo = np.zeros(n + 1, dtype=np.int64)
        mo[1:] = np.cumsum([len(s) for s in mutsb])
        score = np.array([float(m.score) for m in muts], dtype=np.float64) if with_scores else None
        h = C.c_void_p()
        self.check(self.lib.ps_muts_create(C.byref(h), n, start.ctypes.data_as(c_i32p),
                                           oo.ctypes.data_as(c_i64p), b"".join(origs),
                                           mo.ctypes.data_as(c_i64p), b"".join(mutsb),
                                           _dp(score) if score is not None else None))
        return h

    def muts_export(self, h):
        """-> (start int32[n], orig list[str], mut list[str], score float64[n])"""
        n = int(self.lib.ps_muts_count(h))
        ob, mb = int(self.lib.ps_muts_orig_bytes(h)), int(self.lib.ps_muts_mut_bytes(h))
        start = np.zeros(n, dtype=np.int32)
        oo = np.zeros(n + 1, dtype=np.int64)
        mo = np.zeros(n + 1, dtype=np.int64)
        score = np.zeros(n, dtype=np.float64)
        op = C.create_string_buffer(max(ob, 1))
        mp = C.create_string_buffer(max(mb, 1))
        self.check(self.lib.ps_muts_export(h, start.ctypes.data_as(c_i32p), oo.ctypes.data_as(c_i64p), op,
                                           mo.ctypes.data_as(c_i64p), mp, _dp(score)))
        ops, mps = op.raw[:ob].decode("ascii"), mp.raw[:mb].decode("ascii")
        orig = [ops[oo[i]:oo[i + 1]] for i in range(n)]
        mut = [mps[mo[i]:mo[i + 1]] for i in range(n)]
        return start, orig, mut, score

    def muts_destroy(self, h):
        self.lib.ps_muts_destroy(h)

    def seqs_export(self, h):
        n = int(self.lib.ps_seqs_count(h))
        nb = int(self.lib.ps_seqs_bytes(h))
        off = np.zeros(n + 1, dtype=np.int64)
        pool = C.create_string_buffer(max(nb, 1))
        self.check(self.lib.ps_seqs_export(h, off.ctypes.data_as(c_i64p), pool))
        s = pool.raw[:nb].decode("ascii")
        return [s[off[i]:off[i + 1]] for i in range(n)]

    # ------------------------------------------------------------------ free functions
    def score_alignments(self, h, n_events, likes_len=None, likes=None):
        """-> scores float64 [n_events]; with likes_len, or a caller's `likes` (contiguous float64 of at least len(sequence) entries,
        accumulated into in place), -> (scores, likes): the per-base cumulative likelihoods of cpp/MakeMutations.cpp:168-189"""
        scores = np.zeros(n_events, dtype=np.float64)
        if likes is not None:
            if not (isinstance(likes, np.ndarray) and likes.dtype == np.float64 and likes.flags.c_contiguous and likes.flags.writeable):
                raise PoreseqError("score_alignments: likes must be a writeable contiguous float64 array")
        elif likes_len is not None:
            likes = np.zeros(likes_len, dtype=np.float64)
        if likes is not None and likes.size < int(self.lib.ps_align_sequence_length(h)):      # (the library writes len(sequence) entries)
            raise PoreseqError("score_alignments: likes has %d entries, the sequence %d bases" % (likes.size, int(self.lib.ps_align_sequence_length(h))))
        self.check(self.lib.ps_score_alignments(h, _dp(scores), _dp(likes) if likes is not None else None))
        return (scores, likes) if likes is not None else scores

    def find_point_mutations(self, h):
        out = C.c_void_p()
        self.check(self.lib.ps_find_point_mutations(h, C.byref(out)))
        return out

    def find_mutations(self, h, seqs):
        bs = [s.encode("ascii") for s in seqs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(b) for b in bs])
        out = C.c_void_p()
        self.check(self.lib.ps_find_mutations(h, len(bs), off.ctypes.data_as(c_i64p), b"".join(bs), C.byref(out)))
        return out

    def score_mutations(self, h, hm):
        out = C.c_void_p()
        self.check(self.lib.ps_score_mutations(h, hm, C.byref(out)))
        return out

    def score_sequences(self, h, seqs, n_events):
        """-> (scores float64 [len(seqs)][n_events], accuracy float64 [len(seqs)]): ScoreEvents of the AlignData realigned to each
        sequence, and swalign's identity in %; the AlignData is not modified"""
        bs = [s.encode("ascii") for s in seqs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(b) for b in bs])
        scores = np.zeros((len(bs), int(n_events)), dtype=np.float64)
        acc = np.zeros(len(bs), dtype=np.float64)
        if bs:
            self.check(self.lib.ps_score_sequences(h, len(bs), off.ctypes.data_as(c_i64p), b"".join(bs), _dp(scores), _dp(acc)))
        return scores, acc

    def score_mutation_deltas(self, h, hm, n_events, n_muts):
        """[n_events][n_muts] float64: every event's term of every edit's score (their sum in event order + -1e-6 is the score)"""
        out = np.zeros((int(n_events), int(n_muts)), dtype=np.float64)
        if out.size:
            self.check(self.lib.ps_score_mutation_deltas(h, hm, _dp(out)))
        return out

    def point_table(self, h, n, want_table=True):
        """-> (table float64 [n, 9] or None, best POINT_BEST [n]): ps_point_table of one AlignData with n positions"""
        return self.batch_point_table([h], [n], want_table)[0]

    def batch_point_table(self, hs, ns, want_table=True):
        """ps_batch_point_table over the AlignData `hs` with ns[i] positions each, one launch chain and one copy back ->
        [(table float64 [n, 9] or None, best POINT_BEST [n])]: slot 0 the deletion, 1-4 substitution by A / C / G / T (NaN for the
        base itself), 5-8 insertion; best['margin'] the row's largest entry, ['slot'] the first slot holding it, ['n_positive']
        the entries > 0."""
        self._need("ps_batch_point_table")
        R = len(hs)
        ns = np.array([int(n) for n in ns] + [0], dtype=np.int64)
        tables = [np.empty((int(n), POINT_SLOTS), dtype=np.float64) if want_table else None for n in ns[:R]]
        bests = [np.empty(int(n), dtype=POINT_BEST) for n in ns[:R]]
        tp = (c_dp * max(R, 1))(*[_dp(t) for t in tables]) if want_table else None
        bp = (C.POINTER(PsPointBest) * max(R, 1))(*[b.ctypes.data_as(C.POINTER(PsPointBest)) for b in bests])
        self.check(self.lib.ps_batch_point_table(R, self._harr(hs), tp, bp, ns.ctypes.data_as(c_i64p)))
        return list(zip(tables, bests))

    def score_mutation_support(self, h, hm, n_muts, groups, n_groups):
        """-> (scores float64 [M], support EDIT_SUPPORT [M, n_groups]): ps_score_mutation_support of one AlignData"""
        return self.batch_score_mutation_support([h], [hm], [n_muts], [groups], [n_groups])[0]

    def batch_score_mutation_support(self, hs, hms, n_muts, groups, n_groups):
        """ps_batch_score_mutation_support over the AlignData `hs` with the edit lists `hms` of n_muts[i] edits, groups[i] the group
        id of every event of AlignData i (0 .. n_groups[i] - 1): one launch chain, reduced on the device, one copy back ->
        [(scores float64 [M], support EDIT_SUPPORT [M, n_groups[i]])].  support['sum'] is the group's events' terms added in event
        order, ['cover'] the events of the group whose re-aligned span holds the edit, ['pos'] / ['neg'] those of them with a
        positive / negative term."""
        self._need("ps_batch_score_mutation_support")
        R = len(hs)
        ng = np.array([int(g) for g in n_groups] + [0], dtype=np.int32)
        grp = [np.ascontiguousarray(list(g) + [0], dtype=np.int32) for g in groups]   # (one spare entry: never a null pointer)
        scores = [np.empty(int(m), dtype=np.float64) for m in n_muts]
        recs = [np.empty((int(m), max(int(g), 0)), dtype=EDIT_SUPPORT) for m, g in zip(n_muts, ng[:R])]
        gp = (c_i32p * max(R, 1))(*[g.ctypes.data_as(c_i32p) for g in grp])
        sp = (c_dp * max(R, 1))(*[_dp(a) for a in scores])
        rp = (C.POINTER(PsEditSupport) * max(R, 1))(*[r.ctypes.data_as(C.POINTER(PsEditSupport)) for r in recs])
        self.check(self.lib.ps_batch_score_mutation_support(R, self._harr(hs), self._harr(hms), ng.ctypes.data_as(c_i32p), gp, sp, rp))
        return list(zip(scores, recs))

    def score_mutation_genotypes(self, h, hm, n_muts, groups, n_groups, alt_frac, want_support=True):
        """-> (scores [M], support [M, n_groups] or None, lik float64 [M, K + 1], n_cover int32 [M]): ps_score_mutation_genotypes
        of one AlignData"""
        return self.batch_score_mutation_genotypes([h], [hm], [n_muts], [groups], [n_groups], [alt_frac], want_support)[0]

    def batch_score_mutation_genotypes(self, hs, hms, n_muts, groups, n_groups, alt_frac, want_support=True):
        """ps_batch_score_mutation_genotypes over the AlignData `hs`: batch_score_mutation_support's arguments plus alt_frac[i], the
        K_i alt-allele fractions of AlignData i (0 .. 8 of them, each 1e-6 .. 1 - 1e-6).  One launch chain, reduced on the device,
        one copy back -> [(scores float64 [M], support EDIT_SUPPORT [M, n_groups[i]] — None with want_support=False, the records
        are then neither produced nor copied —, lik float64 [M, K_i + 1], n_cover int32 [M])].  lik[:, k] is the log-likelihood of
        alt fraction alt_frac[i][k] over the events that span the edit, relative to hom-ref (0); lik[:, K_i] is hom-alt, the
        covering events' terms added in event order; n_cover counts those events."""
        self._need("ps_batch_score_mutation_genotypes")
        R = len(hs)
        ng = np.array([int(g) for g in n_groups] + [0], dtype=np.int32)
        grp = [np.ascontiguousarray(list(g) + [0], dtype=np.int32) for g in groups]   # (one spare entry: never a null pointer)
        frs = [np.ascontiguousarray(list(f) + [0.0], dtype=np.float64) for f in alt_frac]
        nf = np.array([len(f) - 1 for f in frs] + [0], dtype=np.int32)
        scores = [np.empty(int(m), dtype=np.float64) for m in n_muts]
        recs = [np.empty((int(m), max(int(g), 0)), dtype=EDIT_SUPPORT) if want_support else None for m, g in zip(n_muts, ng[:R])]
        liks = [np.empty((int(m), max(int(k), 0) + 1), dtype=np.float64) for m, k in zip(n_muts, nf[:R])]
        ncov = [np.empty(int(m), dtype=np.int32) for m in n_muts]
        gp = (c_i32p * max(R, 1))(*[g.ctypes.data_as(c_i32p) for g in grp])
        fp = (c_dp * max(R, 1))(*[_dp(f) for f in frs])
        sp = (c_dp * max(R, 1))(*[_dp(a) for a in scores])
        rp = (C.POINTER(PsEditSupport) * max(R, 1))(*[r.ctypes.data_as(C.POINTER(PsEditSupport)) for r in recs]) if want_support else None
        lp = (c_dp * max(R, 1))(*[_dp(a) for a in liks])
        cp = (c_i32p * max(R, 1))(*[a.ctypes.data_as(c_i32p) for a in ncov])
        self.check(self.lib.ps_batch_score_mutation_genotypes(R, self._harr(hs), self._harr(hms), ng.ctypes.data_as(c_i32p), gp,
                                                              nf.ctypes.data_as(c_i32p), fp, sp, rp, lp, cp))
        return list(zip(scores, recs, liks, ncov))

    def score_mutation_phase(self, h, hm, n_muts, n_events, window=2, min_link=0.0, max_sets=4, want_hap=True):
        """-> (scores [M], link EDIT_LINK [M, W], phase EDIT_PHASE [M], hap EVENT_HAP [E, S] or None, n_sets): ps_score_mutation_phase
        of one AlignData"""
        return self.batch_score_mutation_phase([h], [hm], [n_muts], [n_events], [window], [min_link], [max_sets], want_hap)[0]

    def batch_score_mutation_phase(self, hs, hms, n_muts, n_events, window, min_link, max_sets, want_hap=True):
        """ps_batch_score_mutation_phase over the AlignData `hs`: per AlignData the list hms[i] of n_muts[i] candidate sites, its
        event count, the window W_i (1 .. 8), the vote threshold (finite, >= 0) and the number of tagged phase sets S_i (1 .. 8).
        One launch chain, three reductions on the device (k_link, k_phase, k_haptag), one copy back -> [(scores float64 [M],
        link EDIT_LINK [M, W_i], phase EDIT_PHASE [M], hap EVENT_HAP [E, S_i] — None with want_hap=False, the records are then
        neither produced nor copied —, n_sets int)]."""
        self._need("ps_batch_score_mutation_phase")
        R = len(hs)
        win = np.array([int(w) for w in window] + [0], dtype=np.int32)
        mlk = np.array([float(v) for v in min_link] + [0.0], dtype=np.float64)
        mxs = np.array([int(v) for v in max_sets] + [0], dtype=np.int32)
        scores = [np.empty(int(m), dtype=np.float64) for m in n_muts]
        links = [np.zeros((int(m), max(int(w), 0)), dtype=EDIT_LINK) for m, w in zip(n_muts, win[:R])]
        phases = [np.zeros(int(m), dtype=EDIT_PHASE) for m in n_muts]
        haps = [np.zeros((int(e), max(int(v), 0)), dtype=EVENT_HAP) if want_hap else None for e, v in zip(n_events, mxs[:R])]
        nsets = np.zeros(R + 1, dtype=np.int32)
        vp = lambda arrs: (C.c_void_p * max(R, 1))(*[a.ctypes.data_as(C.c_void_p) for a in arrs])
        sp = (c_dp * max(R, 1))(*[_dp(a) for a in scores])
        np_ = (c_i32p * max(R, 1))(*[nsets[i:].ctypes.data_as(c_i32p) for i in range(R)])
        self.check(self.lib.ps_batch_score_mutation_phase(R, self._harr(hs), self._harr(hms), win.ctypes.data_as(c_i32p), _dp(mlk),
                                                          mxs.ctypes.data_as(c_i32p), sp, vp(links), vp(phases),
                                                          vp(haps) if want_hap else None, np_))
        return [(scores[i], links[i], phases[i], haps[i], int(nsets[i])) for i in range(R)]

    def align_stats(self, h, n_events, realign=True):
        """-> (scores float64 [E] or None, stats EVENT_STATS [E]): ps_align_stats of one AlignData"""
        return self.batch_align_stats([h], [n_events], realign)[0]

    def batch_align_stats(self, hs, n_events, realign=True):
        """ps_batch_align_stats over the AlignData `hs` with n_events[i] events: per event the census of its ref_align array and
        the sums of the shift / scale fit of its model (include/poreseq_hip.h has the definition), one launch of k_align_stats and
        one copy back -> [(scores float64 [E] or None, stats EVENT_STATS [E])].  realign=True runs ScoreAlignments' chain first
        (scores are score_alignments' bits and the realignment stays in the handle); realign=False reduces the refs the handle
        holds, launches no DP and returns None for the scores."""
        self._need("ps_batch_align_stats")
        R = len(hs)
        recs = [np.zeros(max(int(e), 1), dtype=EVENT_STATS) for e in n_events]      # (one spare record: never a null pointer)
        scores = [np.zeros(max(int(e), 1), dtype=np.float64) for e in n_events] if realign else None
        rp = (C.c_void_p * max(R, 1))(*[r.ctypes.data_as(C.c_void_p) for r in recs])
        sp = (c_dp * max(R, 1))(*[_dp(a) for a in scores]) if realign else None
        self.check(self.lib.ps_batch_align_stats(R, self._harr(hs), 1 if realign else 0, sp, rp))
        return [(scores[i][:int(e)] if realign else None, recs[i][:int(e)]) for i, e in enumerate(n_events)]

    def kmer_stats(self, h, n_events, groups, n_groups, realign=True):
        """-> (scores float64 [E] or None, table KMER_STATS [G, 1024]): ps_kmer_stats of one AlignData"""
        return self.batch_kmer_stats([h], [n_events], [groups], [n_groups], realign)[0]

    def batch_kmer_stats(self, hs, n_events, groups, n_groups, realign=True):
        """ps_batch_kmer_stats over the AlignData `hs` with n_events[i] events: groups[i] gives every event of AlignData i a group id
        0 .. n_groups[i] - 1 (1 .. 256 groups); per group and 5-mer state the sums of a re-estimation of that state's model rows
        (include/poreseq_hip.h has the definition), one launch of k_kmer_stats and one copy back -> [(scores float64 [E] or None,
        table KMER_STATS [G_i, 1024])].  realign as in batch_align_stats."""
        self._need("ps_batch_kmer_stats")
        R = len(hs)
        grp = [np.ascontiguousarray(np.append(np.asarray(g, dtype=np.int32).reshape(-1), np.int32(0))) for g in groups]   # (one spare id: never a null pointer)
        for g, e in zip(grp, n_events):
            if g.size != int(e) + 1:
                raise ValueError("kmer_stats: %d group ids for %d events" % (g.size - 1, int(e)))
        ng = np.array([int(g) for g in n_groups] + [0], dtype=np.int32)
        tabs = [np.zeros((min(max(int(g), 1), KMER_MAX_GROUPS), 1024), dtype=KMER_STATS) for g in n_groups]
        scores = [np.zeros(max(int(e), 1), dtype=np.float64) for e in n_events] if realign else None
        gp = (c_i32p * max(R, 1))(*[g.ctypes.data_as(c_i32p) for g in grp])
        tp = (C.c_void_p * max(R, 1))(*[t.ctypes.data_as(C.c_void_p) for t in tabs])
        sp = (c_dp * max(R, 1))(*[_dp(a) for a in scores]) if realign else None
        self.check(self.lib.ps_batch_kmer_stats(R, self._harr(hs), 1 if realign else 0, gp, ng.ctypes.data_as(c_i32p), sp, tp))
        return [(scores[i][:int(e)] if realign else None, tabs[i]) for i, e in enumerate(n_events)]

    def move_stats(self, h, n_levels, levels=False):
        """-> (scores float64 [E], records EVENT_MOVES [E][, step, col]): ps_move_stats of one AlignData whose events have
        n_levels[e] levels"""
        return self.batch_move_stats([h], [n_levels], levels)[0]

    def batch_move_stats(self, hs, n_levels, levels=False):
        """ps_batch_move_stats over the AlignData `hs`, n_levels[i][e] the levels of event e of AlignData i: ScoreAlignments' chain
        with one launch of k_move_stats between the backtrace walk and the kernel that overwrites its records, one copy back ->
        [(scores float64 [E] — score_alignments' bits —, records EVENT_MOVES [E])], with levels=True [(scores, records, step, col)]:
        per event a uint8 array of move codes (MOVE_NAMES; 0 off the path) and an int32 array of the columns the levels were
        recorded from (include/poreseq_hip.h has the definition).  The realignment stays in the handles."""
        self._need("ps_batch_move_stats")
        R = len(hs)
        nl = [[int(v) for v in np.asarray(n, dtype=np.int64).reshape(-1)] for n in n_levels]
        recs = [np.zeros(max(len(n), 1), dtype=EVENT_MOVES) for n in nl]      # (one spare record: never a null pointer)
        scores = [np.zeros(max(len(n), 1), dtype=np.float64) for n in nl]
        rp = (C.c_void_p * max(R, 1))(*[r.ctypes.data_as(C.c_void_p) for r in recs])
        sp = (c_dp * max(R, 1))(*[_dp(a) for a in scores])
        stp = clp = None
        if levels:
            step = [[np.zeros(max(v, 1), dtype=np.uint8) for v in n] for n in nl]
            col = [[np.zeros(max(v, 1), dtype=np.int32) for v in n] for n in nl]
            se = [(c_u8p * max(len(n), 1))(*[a.ctypes.data_as(c_u8p) for a in st]) for n, st in zip(nl, step)]
            ce = [(c_i32p * max(len(n), 1))(*[a.ctypes.data_as(c_i32p) for a in cl]) for n, cl in zip(nl, col)]
            stp = (C.POINTER(c_u8p) * max(R, 1))(*[C.cast(x, C.POINTER(c_u8p)) for x in se])
            clp = (C.POINTER(c_i32p) * max(R, 1))(*[C.cast(x, C.POINTER(c_i32p)) for x in ce])
        self.check(self.lib.ps_batch_move_stats(R, self._harr(hs), sp, rp, stp, clp))
        out = []
        for i, n in enumerate(nl):
            E = len(n)
            if levels:
                out.append((scores[i][:E], recs[i][:E], [a[:v] for a, v in zip(step[i], n)], [a[:v] for a, v in zip(col[i], n)]))
            else:
                out.append((scores[i][:E], recs[i][:E]))
        return out

    def posterior_stats(self, h, n_levels, levels=False):
        """-> records EVENT_POSTERIOR [E] (levels=True: (records, emit, col)): ps_posterior_stats of one AlignData whose events
        have n_levels[e] levels"""
        return self.batch_posterior_stats([h], [n_levels], levels)[0]

    def batch_posterior_stats(self, hs, n_levels, levels=False):
        """ps_batch_posterior_stats over the AlignData `hs`, n_levels[i][e] the levels of event e of AlignData i: the band stage of
        the fills, k_post_fwd and k_post_bwd over all events, one copy back -> [records EVENT_POSTERIOR [E]], with levels=True
        [(records, emit, col)]: per event two float64 arrays, the expected number of emitting arrivals at every level and their
        posterior mean column (NaN where there is none; an inert event keeps zeros and NaN).  include/poreseq_hip.h has the
        definition.  Nothing of the handles changes."""
        self._need("ps_batch_posterior_stats")
        R = len(hs)
        nl = [[int(v) for v in np.asarray(n, dtype=np.int64).reshape(-1)] for n in n_levels]
        recs = [np.zeros(max(len(n), 1), dtype=EVENT_POSTERIOR) for n in nl]      # (one spare record: never a null pointer)
        rp = (C.c_void_p * max(R, 1))(*[r.ctypes.data_as(C.c_void_p) for r in recs])
        emp = clp = None
        if levels:
            emit = [[np.zeros(max(v, 1)) for v in n] for n in nl]
            col = [[np.full(max(v, 1), np.nan) for v in n] for n in nl]
            ee = [(c_dp * max(len(n), 1))(*[_dp(a) for a in em]) for n, em in zip(nl, emit)]
            ce = [(c_dp * max(len(n), 1))(*[_dp(a) for a in cl]) for n, cl in zip(nl, col)]
            emp = (C.POINTER(c_dp) * max(R, 1))(*[C.cast(x, C.POINTER(c_dp)) for x in ee])
            clp = (C.POINTER(c_dp) * max(R, 1))(*[C.cast(x, C.POINTER(c_dp)) for x in ce])
        self.check(self.lib.ps_batch_posterior_stats(R, self._harr(hs), rp, emp, clp))
        out = []
        for i, n in enumerate(nl):
            E = len(n)
            if levels:
                out.append((recs[i][:E], [a[:v] for a, v in zip(emit[i], n)], [a[:v] for a, v in zip(col[i], n)]))
            else:
                out.append(recs[i][:E])
        return out

    def debug_posterior(self, h, ev, n_levels, n_states):
        """the forward log tables of ps_posterior_stats for one event (ps_debug_posterior): (main, stay), [n_levels + 1][n_states + 1],
        NaN outside the band"""
        self._need("ps_debug_posterior")
        shape = (n_levels + 1, n_states + 1)
        main, stay = np.zeros(shape), np.zeros(shape)
        self.check(self.lib.ps_debug_posterior(h, ev, _dp(main), _dp(stay)))
        return main, stay

    def make_mutations(self, h, hm):
        nb = C.c_int32(0)
        self.check(self.lib.ps_make_mutations(h, hm, C.byref(nb)))
        return int(nb.value)

    def viterbi_mutate(self, h, nkeep, skip, stay, mmin, mmax, verbose):
        out = C.c_void_p()
        self.check(self.lib.ps_viterbi_mutate(h, nkeep, skip, stay, mmin, mmax, int(bool(verbose)), C.byref(out)))
        try:
            return self.seqs_export(out)
        finally:
            self.lib.ps_seqs_destroy(out)

    # ------------------------------------------------------------------ lock-step batches (several AlignData per call)
    @staticmethod
    def _harr(handles):
        arr = (C.c_void_p * len(handles))()
        for i, h in enumerate(handles):
            arr[i] = h.value if isinstance(h, C.c_void_p) else h
        return arr

    def rng_create(self, seed=1):
        h = C.c_void_p()
        self.check(self.lib.ps_rng_create(C.byref(h), int(seed)))
        return h

    def rng_destroy(self, h):
        self.lib.ps_rng_destroy(h)

    def seqs_create(self, seqs):
        bs = [s.encode("ascii") for s in seqs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(b) for b in bs])
        h = C.c_void_p()
        self.check(self.lib.ps_seqs_create(C.byref(h), len(bs), off.ctypes.data_as(c_i64p), b"".join(bs)))
        return h

    def seqs_destroy(self, h):
        self.lib.ps_seqs_destroy(h)

    def batch_score_alignments(self, handles, n_events):
        n = len(handles)
        scores = [np.zeros(max(int(e), 1), dtype=np.float64) for e in n_events]
        sp = (c_dp * n)(*[_dp(a) for a in scores])
        self.check(self.lib.ps_batch_score_alignments(n, self._harr(handles), sp, None))
        return [a[:int(e)] for a, e in zip(scores, n_events)]

    def batch_find_mutations(self, handles, seqs_handles):
        n = len(handles)
        out = (C.c_void_p * n)()
        self.check(self.lib.ps_batch_find_mutations(n, self._harr(handles), self._harr(seqs_handles), out))
        return [C.c_void_p(out[i]) for i in range(n)]

    def batch_score_mutations(self, handles, muts_handles):
        n = len(handles)
        out = (C.c_void_p * n)()
        self.check(self.lib.ps_batch_score_mutations(n, self._harr(handles), self._harr(muts_handles), out))
        return [C.c_void_p(out[i]) for i in range(n)]

    def batch_score_sequences(self, handles, seqs, n_events):
        """score_sequences for several AlignData in one chain; seqs[i]: the sequences of handles[i] -> [(scores, accuracy)]"""
        n = len(handles)
        hs = [self.seqs_create(list(sv)) for sv in seqs]
        try:
            scores = [np.zeros((len(sv), int(e)), dtype=np.float64) for sv, e in zip(seqs, n_events)]
            acc = [np.zeros(len(sv), dtype=np.float64) for sv in seqs]
            sp = (c_dp * n)(*[_dp(a) for a in scores])
            ap = (c_dp * n)(*[_dp(a) for a in acc])
            self.check(self.lib.ps_batch_score_sequences(n, self._harr(handles), self._harr(hs), sp, ap))
        finally:
            for h in hs:
                self.seqs_destroy(h)
        return list(zip(scores, acc))

    def batch_make_mutations(self, handles, muts_handles):
        n = len(handles)
        nb = np.zeros(max(n, 1), dtype=np.int32)
        self.check(self.lib.ps_batch_make_mutations(n, self._harr(handles), self._harr(muts_handles), nb.ctypes.data_as(c_i32p)))
        return [int(x) for x in nb[:n]]

    def batch_viterbi_mutate(self, handles, rngs, nkeep, skip, stay, mmin, mmax):
        n = len(handles)
        out = (C.c_void_p * n)()
        self.check(self.lib.ps_batch_viterbi_mutate(n, self._harr(handles), self._harr(rngs), nkeep, skip, stay, mmin, mmax, out))
        res = []
        for i in range(n):
            h = C.c_void_p(out[i])
            try:
                res.append(self.seqs_export(h))
            finally:
                self.lib.ps_seqs_destroy(h)
        return res

    def srand(self, seed):
        self.check(self.lib.ps_srand(int(seed)))

    def rand_draw(self, n):
        out = np.zeros(int(n), dtype=np.float64)
        self.check(self.lib.ps_rand_draw(int(n), _dp(out)))
        return out

    def swfull(self, s1, s2):
        b1, b2 = s1.encode("ascii"), s2.encode("ascii")
        cap = len(b1) + len(b2) + 1
        i1 = np.zeros(cap, dtype=np.int32)
        i2 = np.zeros(cap, dtype=np.int32)
        score = C.c_int32(0)
        acc = C.c_double(0)
        n = C.c_int64(0)
        self.check(self.lib.ps_swfull(b1, len(b1), b2, len(b2), C.byref(score), C.byref(acc),
                                      i1.ctypes.data_as(c_i32p), i2.ctypes.data_as(c_i32p), cap, C.byref(n)))
        return int(score.value), float(acc.value), i1[:n.value].copy(), i2[:n.value].copy()

    def sw_summaries(self, pairs):
        """[SwSummary] of the (seq1, seq2) pairs: ONE ps_batch_sw_summary call where the library has it, otherwise the same
        records derived from swfull's index lists pair by pair (the checkers)."""
        pairs = list(pairs)
        if "ps_batch_sw_summary" in self.missing:
            return [summary_from_lists(a, b, *self.swfull(a, b)) for a, b in pairs]
        n = len(pairs)
        if not n:
            return []
        b1 = [a.encode("ascii") for a, _ in pairs]
        b2 = [b.encode("ascii") for _, b in pairs]
        p1, p2 = (C.c_char_p * n)(*b1), (C.c_char_p * n)(*b2)
        n1 = np.array([len(x) for x in b1], dtype=np.int64)
        n2 = np.array([len(x) for x in b2], dtype=np.int64)
        out = (PsSwSummary * n)()
        self.check(self.lib.ps_batch_sw_summary(n, p1, n1.ctypes.data_as(c_i64p), p2, n2.ctypes.data_as(c_i64p), out))
        return [SwSummary(*(int(getattr(r, k)) for k in SwSummary._fields[:-1]), float(r.accuracy)) for r in out]

    def debug_sw_band(self):
        """cumulative Smith-Waterman band counters: banded, fell_back, edge, band_cells, full_cells"""
        fn = self.lib.ps_debug_sw_band   # (the HIP library only: not part of the ABI the checkers export)
        fn.restype, fn.argtypes = C.c_int, [c_i64p]
        out = np.zeros(5, dtype=np.int64)
        self.check(fn(out.ctypes.data_as(c_i64p)))
        return dict(zip(("banded", "fell_back", "edge", "band_cells", "full_cells"), (int(v) for v in out)))

    def seq_to_states(self, s):
        b = s.encode("ascii")
        st = np.zeros(max(len(b), 1), dtype=np.int32)
        n = C.c_int64(0)
        self.check(self.lib.ps_seq_to_states(b, len(b), st.ctypes.data_as(c_i32p), C.byref(n)))
        return st[:n.value].copy()

    def debug_fill(self, h, ev, direction, n_levels, n_states):
        shape = (n_levels + 1, n_states + 1)
        main = np.zeros(shape)
        stay = np.zeros(shape)
        sm = np.zeros(shape, dtype=np.uint8)
        ss = np.zeros(shape, dtype=np.uint8)
        self.check(self.lib.ps_debug_fill(h, ev, direction, _dp(main), _dp(stay),
                                          sm.ctypes.data_as(c_u8p), ss.ctypes.data_as(c_u8p)))
        return main, stay, sm, ss

    def debug_poison(self, index_word=1, value_word=POISON_1E300):
        """overwrite the scratch memory the calling thread's next call could find left over (ps_debug_poison): the index word
        into every 32-bit word of the pools that may hold indices, counts or flags, the value word into every double of the
        value-only pools -> {buffer name: PoisonReport(bytes, cls, skipped)}"""
        self._need("ps_debug_poison")
        cap = 128
        rep = (PsPoisonReport * cap)()
        n = C.c_int32(0)
        self.check(self.lib.ps_debug_poison(int(index_word) & 0xffffffff, int(value_word) & 0xffffffffffffffff, rep, cap, C.byref(n)))
        if n.value > cap:
            raise PoreseqError("ps_debug_poison: %d report records, room for %d" % (n.value, cap))
        return {rep[k].name.decode(): PoisonReport(int(rep[k].bytes), POISON_CLASSES[rep[k].cls], int(rep[k].skipped)) for k in range(n.value)}

    def debug_viterbi(self, handles, cap_T, nkeep, skip, stay, mmin, mmax, obs_build=0):
        """the tables of ViterbiMutate for a batch of AlignData (ps_debug_viterbi) -> per region a dict: T, obs [T][1024],
        bp int16 [T][1024], lik_final [1024], fwd [T][1024] (None when nkeep == 0; rows up to their own scale), paths int16
        [max(nkeep, 1)][T] (states)"""
        self._need("ps_debug_viterbi")
        n, cap, np_ = len(handles), int(cap_T), max(int(nkeep), 1)
        T = np.zeros(max(n, 1), dtype=np.int32)
        obs = np.zeros((n, cap, 1024))
        bp = np.zeros((n, cap, 1024), dtype=np.int16)
        lik = np.zeros((n, 1024))
        fwd = np.zeros((n, cap, 1024)) if nkeep else None
        paths = np.zeros((n, np_, cap), dtype=np.int16)
        self.check(self.lib.ps_debug_viterbi(n, self._harr(handles), int(obs_build), int(nkeep), skip, stay, mmin, mmax, cap,
                                             T.ctypes.data_as(c_i32p), _dp(obs), bp.ctypes.data_as(c_i16p), _dp(lik),
                                             _dp(fwd) if nkeep else None, paths.ctypes.data_as(c_i16p)))
        return [dict(T=int(T[r]), obs=obs[r, :T[r]].copy(), bp=bp[r, :T[r]].copy(), lik_final=lik[r].copy(),
                     fwd=fwd[r, :T[r]].copy() if nkeep else None, paths=paths[r, :, :T[r]].copy()) for r in range(n)]

    def debug_viterbi_steps(self, obs_rows, deviates, nkeep, skip, stay, mmin, mmax):
        """the recursion and back-traces on given emission rows (ps_debug_viterbi_steps): obs_rows[r] is [T_r][1024], deviates[r]
        [nkeep][T_r] (ignored when nkeep == 0) -> per region a dict as debug_viterbi's, without obs"""
        self._need("ps_debug_viterbi_steps")
        R, np_ = len(obs_rows), max(int(nkeep), 1)
        rows = [_f64(o).reshape(-1, 1024) for o in obs_rows]
        T = np.array([o.shape[0] for o in rows] + [0], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(T[:R])]).astype(np.int64)
        tt = int(off[R])
        obs = _f64(np.concatenate(rows)) if R else np.zeros((0, 1024))
        rnd = None
        if nkeep:
            rnd = _f64(np.concatenate([_f64(deviates[r]).reshape(nkeep, int(T[r])).ravel() for r in range(R)] + [np.zeros(1)]))
        bp = np.zeros((max(tt, 1), 1024), dtype=np.int16)
        lik = np.zeros((max(R, 1), 1024))
        fwd = np.zeros((max(tt, 1), 1024)) if nkeep else None
        paths = np.zeros(max(np_ * tt, 1), dtype=np.int16)
        self.check(self.lib.ps_debug_viterbi_steps(R, T.ctypes.data_as(c_i32p), _dp(obs), _dp(rnd) if nkeep else None, int(nkeep),
                                                   skip, stay, mmin, mmax, bp.ctypes.data_as(c_i16p), _dp(lik),
                                                   _dp(fwd) if nkeep else None, paths.ctypes.data_as(c_i16p)))
        return [dict(T=int(T[r]), bp=bp[off[r]:off[r + 1]].copy(), lik_final=lik[r].copy(),
                     fwd=fwd[off[r]:off[r + 1]].copy() if nkeep else None,
                     paths=paths[np_ * off[r]:np_ * off[r + 1]].reshape(np_, int(T[r])).copy()) for r in range(R)]

    def set_sweep_min(self, n):
        """forward-only batches of at least n alignments run one wavefront per alignment (negative: the default)"""
        self.check(self.lib.ps_set_sweep_min(int(n)))

    def set_sweep2_min(self, n):
        """Alignment::update batches (forward + backward sweep per alignment) of at least n sweeps run one wavefront per sweep"""
        self.check(self.lib.ps_set_sweep2_min(int(n)))

    def set_sparse_min(self, n):
        """Alignment::update batches whose edit lists read few matrix columns: strip sweeps with kept columns from n sweeps on"""
        self.check(self.lib.ps_set_sparse_min(int(n)))

    def set_sweep_form(self, rows_per_lane, wavefronts=1):
        """the form strip sweeps try first: rows of the band per lane, wavefronts per (alignment, direction); <= 0: the library's choice"""
        self.check(self.lib.ps_set_sweep_form(int(rows_per_lane), int(wavefronts)))

    def set_device_fraction(self, fraction):
        """the part of the device's memory this process plans for (ranks sharing a GPU: 1 / ranks on it); <= 0: the default"""
        self.check(self.lib.ps_set_device_fraction(float(fraction)))

    def prof_enable(self, on):
        self.check(self.lib.ps_prof_enable(int(on)))   # 1: synchronous per launch, 2: event pairs queued and read by prof_get

    def prof_reset(self):
        self.check(self.lib.ps_prof_reset())

    def prof_units(self, name):
        u = C.c_double(0)
        self.check(self.lib.ps_prof_units(name.encode(), C.byref(u)))
        return float(u.value)

    def prof_get(self, name):
        ms, n, b = C.c_double(0), C.c_int64(0), C.c_double(0)
        self.check(self.lib.ps_prof_get(name.encode(), C.byref(ms), C.byref(n), C.byref(b)))
        return float(ms.value), int(n.value), float(b.value)


_hip = None


def load_hip():
    """The product's one and only native backend.  Fails loudly when it is not built."""
    global _hip
    if _hip is None:
        _hip = CApi(HIP_LIB)
    return _hip
