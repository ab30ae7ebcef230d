"""The oracle's Viterbi table hooks (ps_debug_viterbi, ps_debug_viterbi_steps) against the plain numpy reference of viterbi_ref,
and the preconditions of the crafted inputs that tests/test_hip_viterbi_tables.py feeds to the HIP kernels.  No GPU needed.

The oracle's forward vectors (serial float64 sums, libm exp, normalised every step) measured against the long-double recursion,
in units of 2^-53 (viterbi_ref.fwd_error): 2.1 at T = 1, 27 at T = 9, 42 at T = 33, 27 .. 33 over the trough cases.

Rows that kill the max-plus vector (viterbi_cases.DEAD_CASES) are pinned here first: how many back-pointers of -1 each row gets
under the ordered scan, where the reference's forward vector dies, that the oracle refuses the deterministic back-trace there
 and what it names, and that the deviates of the partly dead cases keep clear of every boundary."""
import numpy as np
import pytest

import backends as B
import viterbi_cases as K
import viterbi_ref as V

need_ld = pytest.mark.skipif(not V.HAVE_LD, reason="np.longdouble has no 64-bit mantissa on this machine")
ARGS = (K.SKIP, K.STAY, K.MMIN, K.MMAX)


def steps(rows, rnd=None, nkeep=0):
    return B.oracle_api().debug_viterbi_steps([rows], [rnd] if nkeep else None, nkeep, *ARGS)[0]


@pytest.mark.parametrize("T", K.LENGTHS)
def test_oracle_steps_equal_the_ordered_scan(T):
    rows = K.random_rows(T, 100 + T)
    bp, lik = V.run64(rows, K.SKIP, K.STAY)
    got = steps(rows)
    assert got["T"] == T
    assert np.array_equal(got["bp"], bp) and np.array_equal(got["lik_final"], lik)
    # the deterministic back-trace follows the back-pointers from the first maximum
    c, want = int(np.argmax(lik)), []
    for i in range(T - 1, -1, -1):
        want.append(c)
        c = int(bp[i][c])
    assert got["paths"][0].tolist() == want[::-1]


@need_ld
@pytest.mark.parametrize("T", (1, 9, 33))
def test_oracle_forward_vectors_against_long_double(T):
    rows = K.random_rows(T, 100 + T)
    got = steps(rows, K.deviates(1, T, T), 1)
    err = V.fwd_error(got["fwd"], V.run_ld(rows, K.SKIP, K.STAY))
    print("oracle forward error, T = %d: %.1f units of 2^-53" % (T, err))
    assert err < 250.0      # three steps' worth of the worst case of a serial sum of 85 terms; the mixing of each step damps older error


def test_rounding_tie_rows_reach_the_fallback():
    """the precondition of the rounding-tie test: a rule without the ordered-scan fallback gets at least 100 back-pointers of row 1
    wrong on these rows (and none of row 0, where all previous scores are equal)"""
    rows = K.tie_rows()
    lik0, _ = V.step64(V.start()[0], rows[0], K.SKIP, K.STAY)
    g = np.arange(256)
    assert np.array_equal(lik0[g + 256], np.nextafter(lik0[g], np.inf))
    assert np.all(lik0[g + 512] < lik0[g] - 0.5) and np.all(lik0[g + 768] < lik0[g + 512] - 0.5)
    bp, _ = V.run64(rows, K.SKIP, K.STAY)
    bp_nf, _ = V.run64(rows, K.SKIP, K.STAY, V.step64_family_argmax)
    assert int(np.count_nonzero(bp[1] != bp_nf[1])) >= 100
    assert np.array_equal(steps(rows)["bp"], bp)


def test_exact_ties_take_the_smallest_index():
    rows = K.equal_rows()
    bp, lik = V.run64(rows, K.SKIP, K.STAY)
    assert np.all(bp == (np.arange(V.NS) >> 2)[None, :])      # first predecessor of the 1-base scan; stay never wins
    got = steps(rows)
    assert np.array_equal(got["bp"], bp) and np.array_equal(got["lik_final"], lik)


@need_ld
@pytest.mark.parametrize("case", K.TROUGHS)
def test_reference_stays_normal_through_the_troughs(case):
    """the precondition of the trough tests: the float64 reference itself survives these rows"""
    rows = K.trough_rows(case)
    assert rows.min() > -400.0
    got = steps(rows, K.deviates(1, K.TROUGH_T, 1), 1)
    bp, lik = V.run64(rows, K.SKIP, K.STAY)
    assert np.array_equal(got["bp"], bp) and np.array_equal(got["lik_final"], lik)
    tot = got["fwd"].sum(axis=1)
    assert np.all(np.abs(tot - 1.0) < 1e-12)
    err = V.fwd_error(got["fwd"], V.run_ld(rows, K.SKIP, K.STAY))
    print("oracle forward error, trough %s: %.1f" % (case, err))
    assert err < 250.0


@need_ld
@pytest.mark.parametrize("nkeep,T,seed", K.TRACE_CASES)
def test_oracle_back_steps_and_deviate_margins(nkeep, T, seed):
    """every back-step of the oracle is the long-double pick, and no deviate of these seeds lies within 2^-40 of a boundary (the
    GPU test excuses no step on the strength of this)"""
    rows, rnd = K.random_rows(T, seed), K.deviates(nkeep, T, seed)
    got = steps(rows, rnd, nkeep)
    assert got["paths"].shape == (nkeep, T)
    assert not K.check_back_steps(got["paths"], V.run_ld(rows, K.SKIP, K.STAY), rnd, nkeep, min_margin=2.0 ** -40)


def test_steps_batch_equals_regions_alone():
    rows = [K.random_rows(9, 31), K.random_rows(0, 32), K.random_rows(17, 33)]
    rnd = [K.deviates(4, 9, 31), np.zeros((4, 0)), K.deviates(4, 17, 33)]
    got = B.oracle_api().debug_viterbi_steps(rows, rnd, 4, *ARGS)
    assert [g["T"] for g in got] == [9, 0, 17]
    for r in (0, 2):
        alone = steps(rows[r], rnd[r], 4)
        for k in ("bp", "lik_final", "fwd", "paths"):
            assert np.array_equal(got[r][k], alone[k]), (r, k)


# ---- rows that kill the max-plus vector (viterbi_cases.DEAD_CASES) -----------------------------------------------------------------
def walk(bp, lik):
    """the deterministic path by the rule of DESIGN.md section 2; bp[0] is not followed"""
    c, out = int(np.argmax(lik)), []
    for i in range(len(bp) - 1, -1, -1):
        out.append(c)
        assert i == 0 or bp[i][c] >= 0
        c = int(bp[i][c])
    return out[::-1]


@pytest.mark.parametrize("name", tuple(K.DEAD_CASES))
def test_dead_rows_are_what_their_names_say(name):
    """the preconditions of the dead-row tests: back-pointers of -1 per row as listed, by the ordered scan and by the oracle; final
    scores of the fully dead cases all -1e300 (of `straddle` all -9.9e299: the live states tie exactly); the deterministic decode
    refused where the last row is dead and T > 1, the ordered scan's own path otherwise"""
    T, _, counts = K.DEAD_CASES[name]
    rows = K.dead_rows(name)
    assert rows.shape == (T, V.NS) and not np.any(np.isnan(rows))
    bp, lik = V.run64(rows, K.SKIP, K.STAY)
    assert K.dead_counts(bp) == counts
    got = steps(rows, K.deviates(16, T, 5), 16)
    assert np.array_equal(got["bp"], bp) and np.array_equal(got["lik_final"], lik)
    if name == "accum":
        assert rows.min() > -1e300
    if name == "below_big":
        assert np.all(np.isfinite(rows))
    if name in K.FULLY_DEAD or name == "T1_neginf":
        assert np.all(lik == -1e300)
    if name == "straddle":
        assert np.all(lik == -9.9e299)
    if name in K.FULLY_DEAD:
        assert counts[K.FIRST_DEAD[name]] == 1024 and (K.FIRST_DEAD[name] == 0 or counts[K.FIRST_DEAD[name] - 1] == 0)
        K.refused_steps(B.oracle_api(), [rows], 0, K.FIRST_DEAD[name])
    else:
        path = steps(rows)["paths"][0].tolist()
        assert path == walk(bp, lik) and min(path) >= 0
        if name == "T1_neginf":
            assert path == [0]


@pytest.mark.parametrize("at", range(K.SWEEP_T))
def test_a_dead_row_at_every_index(at):
    rows = K.sweep_rows(at)
    bp, lik = V.run64(rows, K.SKIP, K.STAY)
    assert K.dead_counts(bp) == (0,) * at + (1024,) * (K.SWEEP_T - at) and np.all(lik == -1e300)
    got = steps(rows, K.deviates(16, K.SWEEP_T, at), 16)
    assert np.array_equal(got["bp"], bp) and np.array_equal(got["lik_final"], lik)
    assert np.all(np.isnan(got["fwd"][at:])) and np.all(np.isfinite(got["fwd"][:at]))
    # a back-step from position i weighs with the forward row of position i: over a dead row it falls through to the last state
    assert np.all(got["paths"][:, max(at - 1, 0):K.SWEEP_T - 1] == V.NS - 1)
    K.refused_steps(B.oracle_api(), [rows], 0, at)


@need_ld
@pytest.mark.parametrize("name", tuple(K.DEAD_CASES))
def test_dead_rows_forward_vectors(name):
    """the reference's forward vector dies (0 / 0, NaN to the end) at the first row whose exp(obs) is 0 for every state that has
    weight — row 4, row 2 of `accum`, never for the two cases that keep live states with ordinary emissions; the oracle's rows before
    that stand against the long-double recursion as everywhere else"""
    T = K.DEAD_CASES[name][0]
    rows = K.dead_rows(name)
    ref, alive = K.run_ld_until_dead(rows, K.SKIP, K.STAY)
    want = {"neginf_mid": 4, "neginf_first": 0, "neginf_last": 8, "below_big": 4, "accum": 2, "half_neginf": 9, "one_alive": 9, "straddle": 4,
            "T1_neginf": 0}[name]
    assert alive == want
    got = steps(rows, K.deviates(16, T, 5), 16)
    assert np.all(np.isnan(got["fwd"][alive:])) and np.all(np.isfinite(got["fwd"][:alive]))
    if alive:
        err = V.fwd_error(got["fwd"][:alive], ref)
        print("oracle forward error, %s: %.1f units of 2^-53" % (name, err))
        assert err < 250.0


@need_ld
@pytest.mark.parametrize("name", tuple(K.DEAD_SEED))
def test_partly_dead_back_steps_and_deviate_margins(name):
    """every stochastic back-step of the oracle over the partly dead rows is the long-double pick, and no deviate of the chosen seed
    lies within 2^-40 of a boundary (the GPU test excuses no step on the strength of this)"""
    rows = K.dead_rows(name)
    rnd = K.deviates(16, len(rows), K.DEAD_SEED[name])
    got = steps(rows, rnd, 16)
    assert not K.check_back_steps(got["paths"], V.run_ld(rows, K.SKIP, K.STAY), rnd, 16, min_margin=2.0 ** -40)


def test_steps_batch_with_a_dead_region():
    """a dead region beside a live one: both equal their runs alone under stochastic back-traces, and the deterministic decode of the
    batch is refused as a whole, naming region 0"""
    rows, rnd = K.dead_batch()
    got = B.oracle_api().debug_viterbi_steps(rows, rnd, 16, *ARGS)
    for r in (0, 2):
        alone = steps(rows[r], rnd[r], 16)
        for k in ("bp", "lik_final", "fwd", "paths"):
            assert np.array_equal(got[r][k], alone[k], equal_nan=k == "fwd"), (r, k)
    K.refused_steps(B.oracle_api(), rows, 0, 4)
    rows[0], rows[2] = rows[2], rows[0]
    K.refused_steps(B.oracle_api(), rows, 2, 4)


@pytest.mark.parametrize("key", K.REGIONS[2:4])
def test_oracle_handle_hook_is_its_viterbi_mutate(key):
    """the handle hook walks the region as ps_viterbi_mutate does: its state paths give ps_viterbi_mutate's sequences, its
    back-pointers are the ordered scan of its own emission rows"""
    orc = B.oracle_api()
    draft, events = K.region(*key)
    for nkeep in (0, 16):
        tab = K.oracle_region_tables(key, nkeep)
        B.reset_rand()
        h = orc.align_create(draft, events, K.P0)
        try:
            seqs = orc.viterbi_mutate(h, nkeep, *ARGS, 0)
        finally:
            orc.align_destroy(h)
        assert tab["T"] > len(draft) // 2
        assert [V.path_to_bases(p) for p in tab["paths"]] == seqs
    bp, lik = V.run64(tab["obs"], K.SKIP, K.STAY)
    assert np.array_equal(tab["bp"], bp) and np.array_equal(tab["lik_final"], lik)


def test_region_holes_span_the_trimmed_mean_branches():
    """the precondition of the emission tests: over the regions, positions see 1 .. 8 contributing events — a single event
    (nl == 1), nothing dropped (nl = 2, 3) and a dropped quarter (nl >= 4)"""
    seen = set()
    for L, E, seed in K.REGIONS:
        draft, events = K.region(L, E, seed)
        n = K.contributing(events, len(draft))
        seen |= set(int(x) for x in n[10:len(draft) - 10])
    assert set(range(1, 9)) <= seen


def test_reference_shim_has_no_table_view():
    if not B.have_ref():
        pytest.skip("reference build not present")
    from poreseq_amd._capi import PoreseqError
    with pytest.raises(PoreseqError):
        B.ref_api().debug_viterbi_steps([K.random_rows(1, 1)], None, 0, *ARGS)
