"""Helpers of test_hip_poison.py: the HIP library behind a proxy that poisons the device scratch (ps_debug_poison) before every
native call, PSAlign on that proxy, the two patterns, and a comparison by bytes of arbitrarily nested results.

The proxy is what makes "poison immediately before each call" uniform: every helper of the suite that takes an `api` or a PSAlign
class runs unchanged on it, and a call chain inside one Python method (Mutate: viterbi_mutate, find_mutations, score_mutations,
make_mutations; ScorePoints: find_point_mutations, score_mutations) is poisoned between its C calls as well."""
import numpy as np

from poreseq_amd import _capi
from poreseq_amd.poreseqcpp import PSAlign

# (index word, value word): the value word made of two index words, and the bits of +1e300
PATTERNS = {"ones": (1, (1 << 32) | 1), "1e300": (1, _capi.POISON_1E300)}
PATTERN_IDS = list(PATTERNS)
_PLAIN = frozenset(["check", "_need", "_harr", "backend_name", "info", "debug_poison", "srand", "rand_draw", "prof_enable", "prof_reset", "prof_get",
                    "prof_units", "set_sweep_min", "set_sweep2_min", "set_sparse_min", "set_sweep_form", "debug_sw_band"])


class PoisonApi:
    """_capi.load_hip() with ps_debug_poison in front of every call that can reach the device or an AlignData"""

    def __init__(self, pattern):
        self._api = _capi.load_hip()
        self._words = PATTERNS[pattern]
        self.calls = 0

    def poison(self):
        self.calls += 1
        return self._api.debug_poison(*self._words)

    def __getattr__(self, name):
        v = getattr(self._api, name)
        if not callable(v) or name in _PLAIN or name.startswith("__"):
            return v

        def poisoned(*a, **kw):
            self.poison()
            return v(*a, **kw)
        return poisoned


_apis = {}


def api(pattern):
    if pattern not in _apis:
        _apis[pattern] = PoisonApi(pattern)
    return _apis[pattern]


class _Ones(PSAlign):
    _native = staticmethod(lambda: api("ones"))


class _Big(PSAlign):
    _native = staticmethod(lambda: api("1e300"))


CLASSES = {"ones": _Ones, "1e300": _Big}


def poison(pattern):
    """one explicit poisoning -> the hook's report"""
    return api(pattern).poison()


def flat(x):
    """a nested result as a flat list of hashable leaves: arrays and floats by their bytes, scored edits by their fields"""
    if isinstance(x, np.ndarray):
        return [("nd", x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())]
    if isinstance(x, (float, np.floating)):
        return [("f", np.float64(x).tobytes())]
    if isinstance(x, dict):
        return [("dict", tuple(x))] + [leaf for k in x for leaf in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [("seq", len(x))] + [leaf for y in x for leaf in flat(y)]
    if hasattr(x, "start") and hasattr(x, "mut"):
        return [("edit", int(x.start), x.orig, x.mut)] + flat(float(getattr(x, "score", 0.0)))
    return [x]


def same_bytes(a, b):
    fa, fb = flat(a), flat(b)
    if fa == fb:
        return True
    k = next((i for i, (x, y) in enumerate(zip(fa, fb)) if x != y), min(len(fa), len(fb)))
    raise AssertionError("results differ by bytes from leaf %d of %d / %d" % (k, len(fa), len(fb)))
