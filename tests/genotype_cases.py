"""The yardstick of the per-edit genotype likelihoods (ps_score_mutation_genotypes), shared by test_genotypes.py (the fallback path on
the CPU checkers) and test_hip_genotypes.py (k_genotype on the GPU): the definition restated as plain loops over (edit, fraction,
event), run over the ORACLE's score_mutation_deltas and the ref_align the oracle's AlignData holds after that call
(support_cases.oracle_terms).

  cover(e, m)       support_cases.covers: the edit is not skipped, e has a span and refstart <= start + 1 <= refend
  n_cover[m]        the covering events
  lik[m][k], k < K  acc = 0.0; for e ascending with cover:  d = delta[e][m], u = exp(-|d|),
                    x = g_k u + f_k if d > 0 else g_k + f_k u,  acc += max(d, 0) + log(x);  g_k = 1.0 - f_k
  lik[m][K]         0.0, then += d over the covering events in event order

`loop64` evaluates this in float64 — with numpy's exp and log on scalars, the functions util.genotypes_from_deltas calls — and
`loopld` in numpy.longdouble (80-bit here, asserted).  n_cover and the hom-alt column are compared for equality / by bytes.  The K
mixture columns are compared with `loopld` under a DERIVED bound:

  |got - ref| <= 2^-52 (16 + n_cover[m]) sum over covering e of (1 + |d_e|)

Per term: one ulp each from exp and log, about three ulp relative in x (a product, a sum, u's own error), which is about
3 * 2^-52 absolute in log x, |log x| <= 14 for the allowed fractions, and one add — 16 * 2^-52 (1 + |d|) covers them with room; the
in-order sum adds n_cover roundings of a running total that is at most sum (14 + |d_e|) in size.  A correct evaluation stays more than
an order of magnitude below it; a wrong cover set, a swapped branch or a dropped event does not."""
import numpy as np

import support_cases as S

assert np.finfo(np.longdouble).eps < 2e-19, "numpy.longdouble is not the 80-bit format here: loopld is no better than float64"


def _loop(terms, L, fracs, real):
    starts, delta, spans = terms
    E, M, K = len(delta), len(starts), len(fracs)
    assert np.isfinite(np.array(delta, dtype=np.float64)).all()          # precondition: no case is left out of the comparison
    f = [real(v) for v in np.asarray(fracs, dtype=np.float64).tolist()]
    g = [real(np.float64(1.0) - np.float64(v)) for v in np.asarray(fracs, dtype=np.float64).tolist()]     # formed once, in FP64
    lik = np.zeros((M, K + 1), dtype=real)
    n_cover = np.zeros(M, dtype=np.int32)
    zero = real(0.0)
    for m in range(M):
        acc = [real(0.0) for _ in range(K)]
        hom, nc = real(0.0), 0
        for e in range(E):
            if not S.covers(spans, starts, L, e, m):
                continue
            d = real(delta[e][m])
            nc += 1
            hom = hom + d
            u = np.exp(-np.abs(d))
            for k in range(K):
                x = g[k] * u + f[k] if d > 0 else g[k] + f[k] * u
                acc[k] = acc[k] + ((d if d > 0 else zero) + np.log(x))
        lik[m, :K] = acc
        lik[m, K] = hom
        n_cover[m] = nc
    return lik, n_cover


def loop64(terms, L, fracs):
    """(lik float64 [M, K + 1], n_cover int32 [M]) by the definition, in float64"""
    return _loop(terms, L, fracs, np.float64)


def loopld(terms, L, fracs):
    """the same in numpy.longdouble"""
    return _loop(terms, L, fracs, np.longdouble)


def bound(terms, L):
    """float64 [M]: 2^-52 (16 + n_cover[m]) sum over the covering events of (1 + |d|)"""
    starts, delta, spans = terms
    out = np.zeros(len(starts))
    for m in range(len(starts)):
        ds = [abs(delta[e][m]) for e in range(len(delta)) if S.covers(spans, starts, L, e, m)]
        out[m] = 2.0 ** -52 * (16 + len(ds)) * sum(1.0 + d for d in ds)
    return out


def yardstick(terms, L, fracs):
    """(loop64's lik, n_cover, loopld's lik, bound [M]) of one case"""
    l64, nc = loop64(terms, L, fracs)
    lld, nc2 = loopld(terms, L, fracs)
    assert np.array_equal(nc, nc2)
    return l64, nc, lld, bound(terms, L)


def worst(lik, want):
    """the largest |lik - loopld| / bound over the mixture columns (0.0 without any): printed by the tests before they assert"""
    _l64, _nc, lld, bnd = want
    K = lld.shape[1] - 1
    if not K or not len(bnd):
        return 0.0
    err = np.abs(np.asarray(lik, dtype=np.longdouble)[:, :K] - lld[:, :K]).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0.0, err / bnd[:, None])
    return float(r.max())


def same(lik, n_cover, want):
    """n_cover equal, the hom-alt column byte for byte loop64's, every mixture column within the bound of loopld"""
    l64, nc, lld, bnd = want
    lik = np.asarray(lik)
    K = l64.shape[1] - 1
    if lik.dtype != np.float64 or lik.shape != l64.shape or np.asarray(n_cover).dtype != np.int32 or not np.array_equal(n_cover, nc):
        return False
    if np.ascontiguousarray(lik[:, K]).tobytes() != np.ascontiguousarray(l64[:, K]).tobytes():
        return False
    err = np.abs(lik.astype(np.longdouble)[:, :K] - lld[:, :K])
    return bool(np.all(err <= bnd[:, None]))
