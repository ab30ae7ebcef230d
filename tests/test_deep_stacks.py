"""Deep event stacks on the CPU (tests/deep_cases.py): the rule that combines the events of a position restated in numpy
(deep_cases.trimmed_row) against the oracle's emission rows, bit for bit, at every contributor count from 1 to 256; the oracle's
back-pointers and final scores against viterbi_ref on those rows; the oracle against the live reference build through
Mutate('viterbi'); and the preconditions that keep the stacks from going stale (every count and every value of `drop` occurs,
the duplicate pairs meet, no emission is non-finite).  The HIP path is held to the same rows in test_hip_deep_stacks.py.

Checked against the checker: with the kept values of a state summed by np.sum (pairwise from eight values on) in place of the
serial sum, test_restatement_by_hand fails and test_oracle_rows_equal_the_restatement fails on every stack but E9, first at 10
contributors.  (np.sum along the event axis of the [nl][1024] array adds the rows in order and gives the serial sum's bits.)
`drop >= nl - 2` in place of `drop > nl - 2` is the same function: floor(nl / 4) reaches nl - 2 only at nl = 2, where it is 0
already, so nothing can tell the two apart; test_restatement_by_hand pins drop at nl = 1 .. 5 instead."""
import numpy as np
import pytest

import backends as B
import deep_cases as D
import ref_cases as RC
import viterbi_cases as K

need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (the reference sources are not here)")
stacks = pytest.mark.parametrize("name", D.NAMES)


# ---- the restatement on rows small enough to do by hand --------------------------------------------------------------------------
def test_restatement_by_hand():
    col = lambda *v: np.array(v, dtype=np.float64)[:, None]
    one = lambda *v: float(D.trimmed_row(col(*v))[0])
    assert [D.drop_of(n) for n in (1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 72, 73, 255, 256)] == [0, 0, 0, 1, 1, 1, 2, 2, 16, 16, 18, 18, 63, 64]
    assert all(D.drop_of(n) == n // 4 <= n - 2 for n in range(2, 258))
    assert one(-7.0) == -7.0
    assert one(-1.0, -3.0) == -2.0 and one(-1.0, -3.0, -8.0) == -4.0                 # nl = 2, 3: nothing dropped
    assert one(-1.0, -100.0, -3.0, -2.0) == -2.0                                    # nl = 4: the lowest goes
    assert one(-5.0, -1.0, -100.0, -3.0, -2.0, -4.0, -200.0, -6.0) == -3.5          # nl = 8: the two lowest go
    # the order of the additions: ascending, from the lowest kept row.  (1 + 2^-53) + 2^-53 rounds back to 1 twice; 2^-53 + 2^-53
    # first and then + 1 does not
    t = 2.0 ** -53
    assert one(1.0, t, t) == (t + t + 1.0) / 3.0 != ((1.0 + t) + t) / 3.0
    # sixteen kept rows, fifteen of 2^-53 below one of 1 (the five lowest of the twenty-one go): the serial sum reaches 15 * 2^-53
    # before it meets the 1 and rounds to 1 + 8 * 2^-52; numpy's pairwise sum of the sixteen (eight strided partial sums) puts
    # the 1 on one 2^-53 first, loses it, and ends on 1 + 7 * 2^-52
    rows = [1.0] + [-9.0] * 5 + [t] * 15
    assert D.drop_of(21) == 5 and one(*rows) == (1.0 + 8 * 2.0 ** -52) / 16.0
    assert float(np.sum(np.array(sorted(rows)[5:]))) == 1.0 + 7 * 2.0 ** -52
    # equal rows sum to the same bits wherever the sort puts them
    assert one(-2.5, -2.5, -1.0, -2.5) == (-2.5 + -2.5 + -1.0) / 3.0
    two = D.trimmed_row(np.array([[-1.0, -8.0], [-3.0, -2.0], [-9.0, -4.0], [-5.0, -6.0]]))      # each state sorts on its own
    assert two.tolist() == [-3.0, -4.0]


# ---- preconditions -------------------------------------------------------------------------------------------------------------------
def test_stack_sizes():
    assert D.DEEP_E == (9, 30, 63, 64, 65, 71, 72, 73, 255, 256)
    for name in D.NAMES:
        draft, events = D.stack(name)
        assert len(events) == D.STACKS[name][0] and len(draft) <= 700, name
        assert all(ev.mean.size == ev.stdv.size == ev.ref_align.size == ev.ref_like.size for ev in events), name
    assert len(D.stack257()[1]) == 257
    assert [len(ev) for _, ev in D.mixed_batch()] == list(D.MIXED_E) == [1, 73, 0, 9, 72]
    assert [len(ev) for _, ev in D.mixed_batch(with73=False)] == [1, 0, 9, 72]
    assert RC.viterbi_positions(D.no_positions_region()[1]) == []


@stacks
def test_every_count_and_every_drop_occur(name):
    """every number of contributors from 1 to E among the kept positions (flat73: 73 and nothing else), and so every `drop` from
    0 to floor(E / 4); several positions at the deepest count"""
    walk, _ = D.restated(name)
    E = D.STACKS[name][0]
    counts = [len(here) for _, here in walk]
    if name == "flat73":
        assert set(counts) == {73} and len(counts) > 100
        return
    assert set(counts) == set(range(1, E + 1)), sorted(set(range(1, E + 1)) - set(counts))
    assert set(D.drop_of(n) for n in counts) == set(range(E // 4 + 1))
    assert counts.count(E) >= 2
    assert len(walk) <= 700


def test_no_two_copies_are_equal_but_the_twins():
    for name in D.NAMES:
        events = D.stack(name)[1]
        twins = set(D.duplicate_pairs()) if name == "dup65" else set()
        keys = {}
        for k, ev in enumerate(events):
            keys.setdefault((ev.mean[:8].tobytes(), ev.stdv[:8].tobytes()), []).append(k)
        assert set(tuple(v) for v in keys.values() if len(v) > 1) == twins, name


def test_twins_meet():
    """dup65: for every pair, positions where both copies contribute (equal keys in the sort) and positions where one does"""
    walk, _ = D.restated("dup65")
    events = D.stack("dup65")[1]
    for a, b in D.duplicate_pairs():
        assert np.array_equal(events[a].mean[:4], events[b].mean[:4]) and np.array_equal(events[a].stdv[:4], events[b].stdv[:4])
        both = sum(1 for _, here in walk if {a, b} <= set(e for e, _, _, _ in here))
        one = sum(1 for _, here in walk if len({a, b} & set(e for e, _, _, _ in here)) == 1)
        assert both >= 2 and one >= 1, (a, b, both, one)
    # equal keys: the two rows are the same bits
    _, here = next(w for w in walk if {0, 1} <= set(e for e, _, _, _ in w[1]))
    r = {e: RC.emission_row(events[e].model, lvl, sd) for e, lvl, sd, _ in here if e in (0, 1)}
    assert r[0].tobytes() == r[1].tobytes()


@stacks
def test_emissions_are_finite_and_distinct(name):
    walk, obs = D.restated(name)
    events = D.stack(name)[1]
    assert np.all(np.isfinite(obs))
    _, here = max(walk, key=lambda w: len(w[1]))
    rows = np.array([RC.emission_row(events[e].model, lvl, sd) for e, lvl, sd, _ in here])
    assert np.all(np.isfinite(rows))
    same = len(here) - len(set(r.tobytes() for r in rows))
    assert same == (sum(1 for a, b in D.duplicate_pairs() if {a, b} <= set(e for e, _, _, _ in here)) if name == "dup65" else 0)


def test_a_cut_read_does_not_come_back():
    """what cut_behind's dropped levels are for: with ref_align zeroed alone, the reference's extrapolated ref_index brings an
    early-cut read back at later positions, next to a read that keeps the walk going (oracle and restatement agree on that,
    too: the cases of viterbi_cases.region are cut that way)"""
    draft, base, full = D.base_region(*D.SMALL)
    p = full[D.LEAD + 4]
    behind = lambda ev: [r for r, here in RC.viterbi_positions([D.twin(base[0]), ev]) if r > p and any(e == 1 for e, _, _, _ in here)]
    came_back = 0
    for b in range(1, D.BASE_E):
        ev = D.twin(base[b])
        ev.ref_align[ev.ref_align > p] = 0
        assert bool(behind(ev)) == D.comes_back(ev.ref_align, p), b
        came_back += bool(behind(ev))
        D.cut_behind(ev, p)
        assert not D.comes_back(ev.ref_align, p) and not behind(ev), b
        assert ev.mean.size == ev.ref_align.size <= int(np.flatnonzero(ev.ref_align > 0)[-1]) + 1 + D.TAIL
    assert came_back >= 1


# ---- the oracle against the restatement and viterbi_ref --------------------------------------------------------------------------------
@stacks
def test_oracle_rows_equal_the_restatement(name):
    walk, obs = D.restated(name)
    got = D.oracle_tables(name, 16)
    assert got["T"] == len(walk)
    if not np.array_equal(got["obs"], obs):
        t = int(np.flatnonzero((got["obs"] != obs).any(axis=1))[0])
        raise AssertionError("%s: first differing position %d (%d contributors)" % (name, t, len(walk[t][1])))


@stacks
def test_oracle_steps_equal_the_ordered_scan(name):
    bp, lik = D.steps_ref(name)
    for nkeep in (16, 0):
        got = D.oracle_tables(name, nkeep)
        assert np.array_equal(got["bp"], bp) and np.array_equal(got["lik_final"], lik), (name, nkeep)
    assert D.oracle_tables(name, 0)["fwd"] is None


def test_oracle_takes_257_events():
    draft, events = D.stack257()
    walk, obs = D.restated_obs(events)
    got = RC.viterbi_tables(B.oracle_api(), draft, events, K.P0, 0, len(draft) + 64)
    assert max(len(here) for _, here in walk) == 257
    assert got["T"] == len(walk) and np.array_equal(got["obs"], obs)


def test_viterbi_calls_refuse_a_region_without_events():
    """alone or in a batch: this is why the batches of handles carry a region without positions in the middle"""
    from poreseq_amd._capi import PoreseqError
    api = B.oracle_api()
    draft, events = D.empty_region()
    h = api.align_create(draft, events, K.P0)
    try:
        with pytest.raises(PoreseqError) as err:
            api.debug_viterbi([h], 64, 0, *RC.VIT)
        assert "no events" in str(err.value)
    finally:
        api.align_destroy(h)
    pa = B.make_pa(B.OraclePSAlign, draft, [], K.P0)
    assert pa.ScoreEvents() == []


# ---- the oracle against the live reference ---------------------------------------------------------------------------------------------
def mutate_log(cls, name):
    draft, events = D.stack(name)
    B.reset_rand()
    pa = B.make_pa(cls, draft, events, K.P0)
    return [pa.Mutate(seqs="viterbi", reps=1), pa.sequence], RC.refs(pa)


@need_ref
@pytest.mark.parametrize("name", D.REF_STACKS)
def test_oracle_equals_the_reference_build(name):
    got, want = mutate_log(B.OraclePSAlign, name), mutate_log(B.RefPSAlign, name)
    assert got[0] == want[0] and got[0][0] > 0
    assert RC.same_arrays(got[1], want[1])
