"""The tables of the ViterbiMutate kernels (ps_viterbi.hip), step by step: the trimmed-mean emissions of the three emission builds,
the back-pointers and final scores of k_vit_steps, its forward vectors, and every back-step of k_vit_trace — against the oracle and
against the plain reference of viterbi_ref (ordered scan in float64, forward recursion in long double).

Max-plus tables must be equal bit for bit.  A forward table is normalised per row in long double and compared with the long-double
recursion (viterbi_ref.fwd_error, units of 2^-53); the device must stay within 4x the figure the oracle's own serial float64 sums
reach on the same rows (device exp / log are 1-2 ulp where libm is under 1, and the sums associate differently).

Measured maxima of the oracle, units of 2^-53: 2.1 at T = 1, 27 at T = 9, 42 at T = 33, 27 .. 33 over the trough cases, 16 .. 38 over
the regions.  The device on an MI355X (every test prints both figures before it asserts): 1.7 at T = 1, 7.4 at T = 9, 8.8 at
T = 33, 8.6 .. 12.2 over the trough cases, 8.7 .. 12.5 over the regions; a float64 restatement of the device's scheme on the CPU
(family sums, one power-of-two scale per step) reaches 1.7 / 6.8 / 9.3 and 8.1 .. 10.5 on the same rows, and with the earlier
every-8-steps scale its totals reach 0 in the -150 and -300 troughs.

Rows that kill the max-plus vector (viterbi_cases.DEAD_CASES: -inf rows, rows below -1e300, running scores that pass -1e300, half
dead rows, one live state, live scores that absorb every addend): back-pointers of -1 and scores of exactly -1e300 must come out of
the family reduction bit for bit; the forward rule holds on the rows before the reference's own vector dies (device 3.4 .. 8.0
against the oracle's 12.1 .. 25.5 there) and a dead vector is required after; the deterministic back-trace is refused where it
would follow a -1.
"""

import numpy as np
import pytest

import backends as B
import viterbi_cases as K
import viterbi_ref as V
from poreseq_amd import _capi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not V.HAVE_LD, reason="np.longdouble has no 64-bit mantissa on this machine")]
ARGS = (K.SKIP, K.STAY, K.MMIN, K.MMAX)
TABLES = ("bp", "lik_final", "fwd", "paths")


def run_steps(rows, rnd, nkeep):
    """(device, oracle) tables of one region through the steps hook"""
    dv = rnd if nkeep else None
    return tuple(api.debug_viterbi_steps([rows], [dv] if nkeep else None, nkeep, *ARGS)[0] for api in (_capi.load_hip(), B.oracle_api()))


def check_exact(hip, orc, rows):
    bp, lik = V.run64(rows, K.SKIP, K.STAY)
    assert hip["T"] == orc["T"] == len(rows)
    assert np.array_equal(hip["bp"], bp) and np.array_equal(orc["bp"], bp)
    assert np.array_equal(hip["lik_final"], lik) and np.array_equal(orc["lik_final"], lik)


def check_forward(hip, orc, rows, what):
    """the device's forward table within 4x the oracle's own error against the long-double recursion; no raw row total 0 or subnormal"""
    tot = hip["fwd"].sum(axis=1)
    assert np.all(np.isfinite(tot)) and np.all(tot >= np.finfo(np.float64).tiny), "raw row totals: %s" % tot
    ref = V.run_ld(rows, K.SKIP, K.STAY)
    e_orc, e_hip = V.fwd_error(orc["fwd"], ref), V.fwd_error(hip["fwd"], ref)
    print("forward error %s: oracle %.1f, device %.1f units of 2^-53" % (what, e_orc, e_hip))
    assert e_hip <= 4.0 * e_orc, (what, e_hip, e_orc)


@pytest.mark.parametrize("T", K.LENGTHS)
def test_steps_every_length(T):
    """every phase of the unrolled 4 + 4 loop and of its prefetch clamp"""
    rows = K.random_rows(T, 100 + T)
    hip, orc = run_steps(rows, K.deviates(1, T, T), 1)
    check_exact(hip, orc, rows)
    check_forward(hip, orc, rows, "T = %d" % T)


def test_rounding_ties_take_the_ordered_scan():
    """a family member one ulp below the maximum, at a smaller state index, rounds to the same sum for about half of the destinations:
    k_vit_steps must fall back to the reference's ordered scan there (tests/test_viterbi_tables.py proves the rows reach that case)"""
    rows = K.tie_rows()
    bp_nf, _ = V.run64(rows, K.SKIP, K.STAY, V.step64_family_argmax)
    bp, _ = V.run64(rows, K.SKIP, K.STAY)
    assert int(np.count_nonzero(bp[1] != bp_nf[1])) >= 100
    hip, orc = run_steps(rows, None, 0)
    check_exact(hip, orc, rows)
    assert np.array_equal(hip["paths"], orc["paths"])


def test_exact_ties_take_the_smallest_index():
    rows = K.equal_rows()
    hip, orc = run_steps(rows, K.deviates(1, len(rows), 5), 1)
    check_exact(hip, orc, rows)
    assert np.all(hip["bp"] == (np.arange(V.NS) >> 2)[None, :])
    check_forward(hip, orc, rows, "equal rows")


@pytest.mark.parametrize("case", K.TROUGHS)
def test_troughs_keep_the_forward_vector_alive(case):
    """a stretch of rows 20 .. 300 nats down (levels outside the model's range, near-zero stdv terms): the reference renormalises
    every step and survives; so must the device's power-of-two scaling"""
    rows = K.trough_rows(case)
    rnd = K.deviates(1, K.TROUGH_T, 1)
    hip, orc = run_steps(rows, rnd, 1)
    check_exact(hip, orc, rows)
    check_forward(hip, orc, rows, "trough %s" % (case,))
    assert not K.check_back_steps(hip["paths"], V.run_ld(rows, K.SKIP, K.STAY), rnd, 1, min_margin=2.0 ** -40)


def test_batch_offsets():
    """R = 3 with T = (9, 0, 17): each region's tables equal a run of it alone (t_off, pos_reg, the gridDim.x * t_off offsets of
    deviates and paths)"""
    hip = _capi.load_hip()
    rows = [K.random_rows(9, 31), K.random_rows(0, 32), K.random_rows(17, 33)]
    rnd = [K.deviates(16, 9, 31), np.zeros((16, 0)), K.deviates(16, 17, 33)]
    got = hip.debug_viterbi_steps(rows, rnd, 16, *ARGS)
    assert [g["T"] for g in got] == [9, 0, 17]
    for r in (0, 2):
        alone = hip.debug_viterbi_steps([rows[r]], [rnd[r]], 16, *ARGS)[0]
        for k in TABLES:
            assert np.array_equal(got[r][k], alone[k]), (r, k)
        check_exact(got[r], alone, rows[r])
    got0 = hip.debug_viterbi_steps(rows, None, 0, *ARGS)       # the deterministic back-trace of a batch
    for r in (0, 2):
        assert np.array_equal(got0[r]["paths"], B.oracle_api().debug_viterbi_steps([rows[r]], None, 0, *ARGS)[0]["paths"])


@pytest.mark.parametrize("nkeep,T,seed", K.TRACE_CASES)
def test_back_steps_one_by_one(nkeep, T, seed):
    """every back-step of k_vit_trace judged on its own: from the device's own state at position i, its state at i - 1 must be the
    long-double pick for that deviate.  No step is excused: tests/test_viterbi_tables.py asserts that no deviate of these seeds
    lies within 2^-40 of a boundary."""
    rows, rnd = K.random_rows(T, seed), K.deviates(nkeep, T, seed)
    hip, orc = run_steps(rows, rnd, nkeep)
    check_exact(hip, orc, rows)
    assert hip["paths"].shape == (nkeep, T)
    start = int(np.argmax(hip["lik_final"]))
    assert np.all(hip["paths"][:, T - 1] == start)
    assert not K.check_back_steps(hip["paths"], V.run_ld(rows, K.SKIP, K.STAY), rnd, nkeep, min_margin=2.0 ** -40)
    assert np.array_equal(hip["paths"], orc["paths"])


# ---- rows that kill the max-plus vector, wholly or partly (viterbi_cases.DEAD_CASES; tests/test_viterbi_tables.py pins what each
# case does to the ordered scan and to the reference's forward vector) -----------------------------------------------------------
def check_forward_until_dead(hip, orc, rows, what):
    """check_forward on the rows before the first whose long-double total is 0; from that row on the reference carries NaN and the
    device's vector must be dead as well: every row total 0 or NaN, which makes k_vit_trace fall through to the last state as the
    reference does (the paths, compared exactly, say that it did)"""
    _, alive = K.run_ld_until_dead(rows, K.SKIP, K.STAY)
    assert np.all(np.isnan(orc["fwd"][alive:])) and np.all(np.isfinite(orc["fwd"][:alive]))
    if alive:
        check_forward({"fwd": hip["fwd"][:alive]}, {"fwd": orc["fwd"][:alive]}, rows[:alive], what)
    tot = hip["fwd"][alive:].sum(axis=1)
    assert np.all((tot == 0) | np.isnan(tot)), (what, tot)


@pytest.mark.parametrize("name", tuple(K.DEAD_CASES))
def test_dead_rows_tables_and_stochastic_paths(name):
    """back-pointers (-1 where no candidate is above -1e300) and final scores exact through the family reduction: members at exactly
    -1e300, `second` on the sentinel, live scores that absorb every addend; 16 stochastic paths the oracle's"""
    T = K.DEAD_CASES[name][0]
    rows = K.dead_rows(name)
    rnd = K.deviates(16, T, K.DEAD_SEED.get(name, 5))
    hip, orc = run_steps(rows, rnd, 16)
    check_exact(hip, orc, rows)
    assert K.dead_counts(hip["bp"]) == K.DEAD_CASES[name][2]
    assert np.array_equal(hip["paths"], orc["paths"])
    check_forward_until_dead(hip, orc, rows, name)
    if name in K.DEAD_SEED:
        assert not K.check_back_steps(hip["paths"], V.run_ld(rows, K.SKIP, K.STAY), rnd, 16, min_margin=2.0 ** -40)


@pytest.mark.parametrize("name", tuple(K.DEAD_CASES))
def test_dead_rows_deterministic_decode(name):
    """nkeep = 0: a path that meets a back-pointer of -1 is refused by both backends, naming the first dead position; the partly dead
    cases and T = 1 return the oracle's path, which holds no -1"""
    rows = K.dead_rows(name)
    if name in K.FULLY_DEAD:
        for api in (_capi.load_hip(), B.oracle_api()):
            K.refused_steps(api, [rows], 0, K.FIRST_DEAD[name])
        # the library is as usable as before
        live = K.random_rows(9, 31)
        hip, orc = run_steps(live, None, 0)
        check_exact(hip, orc, live)
        assert np.array_equal(hip["paths"], orc["paths"])
    else:
        hip, orc = run_steps(rows, None, 0)
        check_exact(hip, orc, rows)
        assert np.array_equal(hip["paths"], orc["paths"]) and hip["paths"].min() >= 0
        if name == "T1_neginf":
            assert hip["paths"].tolist() == [[0]]


@pytest.mark.parametrize("at", range(K.SWEEP_T))
def test_a_dead_row_at_every_index(at):
    """an all -inf row in each phase of the unrolled 4 + 4 loop and of its prefetch clamp"""
    rows = K.sweep_rows(at)
    hip, orc = run_steps(rows, K.deviates(16, K.SWEEP_T, at), 16)
    check_exact(hip, orc, rows)
    assert K.dead_counts(hip["bp"]) == (0,) * at + (1024,) * (K.SWEEP_T - at)
    assert np.array_equal(hip["paths"], orc["paths"])
    check_forward_until_dead(hip, orc, rows, "dead row %d of %d" % (at, K.SWEEP_T))
    K.refused_steps(_capi.load_hip(), [rows], 0, at)


def test_batch_with_a_dead_region():
    """R = 3 of (dead from row 4, T = 0, live): under stochastic back-traces each region's tables equal its run alone by bytes; the
    deterministic decode of the batch is refused as a whole and names region 0"""
    hip = _capi.load_hip()
    rows, rnd = K.dead_batch()
    got = hip.debug_viterbi_steps(rows, rnd, 16, *ARGS)
    assert [g["T"] for g in got] == [9, 0, 17]
    for r in (0, 2):
        alone = hip.debug_viterbi_steps([rows[r]], [rnd[r]], 16, *ARGS)[0]
        for k in TABLES:
            assert got[r][k].tobytes() == alone[k].tobytes(), (r, k)
        check_exact(got[r], alone, rows[r])
    K.refused_steps(hip, rows, 0, 4)
    K.refused_steps(hip, rows[::-1], 2, 4)
    assert np.array_equal(hip.debug_viterbi_steps(rows[1:], None, 0, *ARGS)[1]["paths"], B.oracle_api().debug_viterbi_steps(rows[2:], None, 0, *ARGS)[0]["paths"])


# ---- the handle hook: vit_gather, the emission kernel, steps, log, trace on real AlignData -----------------------------------
def hip_region_tables(keys, nkeep, build=0):
    hip = _capi.load_hip()
    hs = []
    try:
        for key in keys:
            draft, events = K.region(*key)
            hs.append(hip.align_create(draft, events, K.P0))
        return hip.debug_viterbi(hs, max(k[0] for k in keys) + 64, nkeep, *ARGS, obs_build=build)
    finally:
        for h in hs:
            hip.align_destroy(h)


def check_region(got, want, what, forward=True):
    assert got["T"] == want["T"] and got["T"] > 0
    assert np.array_equal(got["obs"], want["obs"]), what
    bp, lik = V.run64(want["obs"], K.SKIP, K.STAY)
    assert np.array_equal(got["bp"], bp) and np.array_equal(want["bp"], bp), what
    assert np.array_equal(got["lik_final"], lik) and np.array_equal(want["lik_final"], lik), what
    assert np.array_equal(got["paths"], want["paths"]), what
    if forward:
        check_forward(got, want, want["obs"], what)


@pytest.mark.parametrize("key", K.REGIONS + (K.DEEP_REGION,))
def test_region_tables_under_every_emission_build(key):
    """T and the trimmed-mean emissions bit-equal to the oracle under every emission build that admits the region's events
    (k_vit_obs_lds, k_vit_obs<64>, k_vit_obs<256>); back-pointers and final scores exact, forward vectors within the bound, state
    paths the oracle's (deviates from the per-thread generator)"""
    E = key[1]
    want = K.oracle_region_tables(key, 16)
    builds = K.admitted_builds(E)
    for b in [0] + builds:
        B.reset_rand()
        got = hip_region_tables([key], 16, b)[0]
        check_region(got, want, "region %s, build %d" % (key, b), forward=b in (0, builds[-1]))
    for b in sorted(set((1, 2, 3)) - set(builds)):
        with pytest.raises(_capi.PoreseqError):
            hip_region_tables([key], 16, b)
    B.reset_rand()
    got = hip_region_tables([key], 0)[0]
    want0 = K.oracle_region_tables(key, 0)
    assert got["fwd"] is None and np.array_equal(got["paths"], want0["paths"]) and np.array_equal(got["bp"], want0["bp"])


def test_region_batch_equals_regions_alone():
    """three handles with E = (3, 8, 1) and unequal L in one call equal the three run alone (in_off, t_off on the real path); the
    deviates come from one generator in region order either way"""
    B.reset_rand()
    got = hip_region_tables(list(K.BATCH), 16)
    B.reset_rand()
    alone = [hip_region_tables([key], 16)[0] for key in K.BATCH]
    assert len(set(g["T"] for g in got)) == 3
    for r, (g, a) in enumerate(zip(got, alone)):
        for k in ("obs",) + TABLES:
            assert np.array_equal(g[k], a[k]), (r, k)
        assert np.array_equal(g["obs"], K.oracle_region_tables(K.BATCH[r], 16)["obs"])
