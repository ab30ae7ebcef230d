"""A plain numpy reference of ViterbiMutate's recursion and back-traces (cpp/Viterbi.cpp:39-131), for the table-level tests.

step64   the reference's ordered scan in float64 with the reference's association: bit-exact for lik and bp
step_ld  the forward recursion in np.longdouble (64-bit mantissa on x86), normalised every step
pick_ld  the long-double cumulative sums of T[cur][p] * fwd[p]^atten that one stochastic back-step walks
"""
import math

import numpy as np

NS = 1024
LD = np.longdouble
HAVE_LD = np.finfo(np.longdouble).nmant >= 63   # x87 extended or better; the tests that need it skip otherwise
BIG = 1e300
_C = np.arange(NS)


def start():
    """(lik, fwd) before the first position, cpp/Viterbi.cpp:262-268"""
    return np.zeros(NS), np.full(NS, 1.0 / NS)


def preds(j):
    """[4^j][1024]: the predecessors of every state with a j-base advance, in the order the reference scans them (ascending state)"""
    return (_C[None, :] >> (2 * j)) + (np.arange(4 ** j)[:, None] << (10 - 2 * j))


_PREDS = {j: preds(j) for j in (1, 2, 3, 4)}


def _lsp(skip):
    """log weights of the 1 / 2 / 3-base advances as V_LIK accumulates them: lsp = (lsp + log .25) + log skip (libm logs, as the C++)"""
    l25, lskip = math.log(0.25), math.log(skip)
    out = [l25]
    for _ in range(2):
        out.append((out[-1] + l25) + lskip)
    return out


def step64(lik, obs, skip, stay):
    """one max-plus step: (lik', bp int) by the reference's ordered scan (first strict maximum), (obs[c] + lsp) + lik[q], levels
    j = 1, 2, 3, then stay"""
    best = np.full(NS, -BIG)
    bp = np.full(NS, -1, dtype=np.int64)
    for j, lsp in zip((1, 2, 3), _lsp(skip)):
        a = obs + lsp
        for q in _PREDS[j]:
            l = a + lik[q]
            up = l > best
            best = np.where(up, l, best)
            bp = np.where(up, q, bp)
    l = (obs + math.log(stay)) + lik
    up = l > best
    return np.where(up, l, best), np.where(up, _C, bp)


def step64_family_argmax(lik, obs, skip, stay):
    """the same step WITHOUT the ordered-scan fallback: per advance length the smallest index of the family maximum.  Differs from
    step64 exactly where a smaller, earlier member rounds to the same sum; the tests use it to prove their tie inputs reach that case"""
    best = np.full(NS, -BIG)
    bp = np.full(NS, -1, dtype=np.int64)
    for j, lsp in zip((1, 2, 3), _lsp(skip)):
        fam = lik[_PREDS[j]]                       # [4^j][1024]
        k = np.argmax(fam, axis=0)                 # first maximum = smallest state index
        l = (obs + lsp) + fam[k, _C]
        up = l > best
        best = np.where(up, l, best)
        bp = np.where(up, _PREDS[j][k, _C], bp)
    l = (obs + math.log(stay)) + lik
    up = l > best
    return np.where(up, l, best), np.where(up, _C, bp)


def run64(rows, skip, stay, step=step64):
    """(bp [T][1024], lik_final) of the rows through `step`"""
    lik, _ = start()
    bps = []
    for o in rows:
        lik, bp = step(lik, np.asarray(o, dtype=np.float64), skip, stay)
        bps.append(bp)
    return np.array(bps, dtype=np.int64).reshape(len(bps), NS), lik


def step_ld(fwd, obs, skip, stay):
    """one forward step in long double, normalised to sum 1 (V_LIK's fs and normvec, cpp/Viterbi.cpp:76-101)"""
    fwd = np.asarray(fwd, dtype=LD)
    fs = np.zeros(NS, dtype=LD)
    sp = LD(0.25)
    for j in (1, 2, 3):
        fs += sp * fwd.reshape(4 ** j, NS >> (2 * j)).sum(axis=0)[_C >> (2 * j)]
        sp = sp * LD(0.25) * LD(skip)
    fs += LD(stay) * fwd
    fs *= np.exp(np.asarray(obs, dtype=LD))
    return fs / fs.sum()


def run_ld(rows, skip, stay):
    """[T][1024] long double: the normalised forward vector after every row"""
    f = np.asarray(start()[1], dtype=LD)
    out = []
    for o in rows:
        f = step_ld(f, o, skip, stay)
        out.append(f)
    return np.array(out, dtype=LD).reshape(len(out), NS)


def trans_row(cur, skip, stay):
    """T[cur][:] of buildT (cpp/Viterbi.cpp:134-168): 1..4-base advances add up, the diagonal is the stay probability"""
    t = np.zeros(NS, dtype=LD)
    sp = LD(0.25)
    for j in (1, 2, 3, 4):
        t[_PREDS[j][:, cur]] += sp
        sp = sp * LD(0.25) * LD(skip)
    t[cur] = LD(stay)
    return t


def pick_ld(fwd_row, cur, atten, skip, stay):
    """long-double cumulative sums of T[cur][p] * fwd[p]^atten over p (randbp, cpp/Viterbi.cpp:105-131): a deviate r picks the first
    p with r * cum[-1] < cum[p]"""
    w = trans_row(cur, skip, stay) * np.power(np.asarray(fwd_row, dtype=LD), LD(atten))
    return np.cumsum(w)


def pick(cum, r):
    """(state, margin): the state the deviate picks and its distance to the nearest interior boundary relative to the total"""
    tot = cum[-1]
    x = LD(r) * tot
    hit = np.nonzero(x < cum)[0]
    state = int(hit[0]) if hit.size else NS - 1
    inner = cum[(cum > 0) & (cum < tot)]
    margin = float(np.min(np.abs(inner - x)) / tot) if inner.size else 1.0
    return state, margin


def fwd_error(rows, ref):
    """the forward metric: rows (any scale per row) normalised to sum 1 in long double against ref [T][1024] long double; the maximum
    over states with p_ref >= 2^-200 of |p - p_ref| / p_ref in units of 2^-53.  States below the floor must have p <= 2^-199."""
    rows = np.asarray(rows, dtype=LD)
    worst = 0.0
    for t in range(rows.shape[0]):
        tot = rows[t].sum()
        assert np.isfinite(tot) and tot > 0, "row %d of the forward table has total %r" % (t, tot)
        p = rows[t] / tot
        big = ref[t] >= LD(2.0) ** -200
        assert np.all(p[~big] <= LD(2.0) ** -199), "row %d: a state below the floor in the reference is not small" % t
        worst = max(worst, float(np.max(np.abs(p[big] - ref[t][big]) / ref[t][big]) * LD(2.0) ** 53))
    return worst


def path_to_bases(path):
    """StatesToSequence (cpp/Viterbi.cpp:171-237)"""
    base = lambda st, k: "ACGT"[3 & (st >> (2 * (4 - k)))]
    cur = int(path[0])
    s = [base(cur, 0)]
    for nxt in path[1:]:
        nxt = int(nxt)
        if nxt == cur:
            continue
        for n in (1, 2, 3, 4):
            if (nxt >> (2 * n)) == (cur & ((NS >> (2 * n)) - 1)):      # nxt = ((cur << 2n) & 1023) + k
                s += [base(cur, b) for b in range(1, n + 1)]
                break
        else:
            s.append(base(nxt, 0))
        cur = nxt
    s += [base(cur, b) for b in range(1, 5)]
    return "".join(s)
