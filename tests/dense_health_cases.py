"""Shared by tests/test_dense64_health_host.py (CPU) and tests/test_gpu_dense64_health.py: the op-by-op numpy models of
ekf_dense64_health and ekf_dense64_symmetrize as include/ekfslam.h defines them, and the families of live corners they are
checked on.  Everything is IEEE binary64, one rounding per operation; "bits" means the 64-bit pattern of a double."""
import numpy as np

SIGN_OFF = np.uint64(0x7FFFFFFFFFFFFFFF)
FAMILIES = ("symmetric_integers", "asymmetric_integers", "random_spd", "degenerate")
REPORT_FIELDS = ("n_nonfinite", "n_asym", "n_diag_bad", "n_minor", "max_asym", "min_diag", "asym_i", "asym_j", "min_diag_i")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def same_report(got, want):
    """field for field, doubles as bits (ms, if there, is not a field)"""
    return all(same_bits(got[k], want[k]) if isinstance(want[k], float) else got[k] == want[k] for k in REPORT_FIELDS)


def _pairs(Sigma, Na):
    """the pairs i < j < Na in lexicographic order -> i, j, Sigma[i][j], Sigma[j][i]"""
    C = np.asarray(Sigma, dtype=np.float64)[:Na, :Na]
    i, j = np.triu_indices(Na, 1)
    return i, j, np.ascontiguousarray(C[i, j]), np.ascontiguousarray(C[j, i])


def _max_asym(a, b):
    """-> (the maximum of |fl(a - b)| on its bit pattern as a double, the first position that attains it or -1)"""
    if a.size == 0:
        return 0.0, -1
    with np.errstate(all="ignore"):
        m = bits(a - b) & SIGN_OFF
    k = int(np.argmax(m))   # the first occurrence: the lowest (i, j)
    return float(m[k:k + 1].view(np.float64)[0]), k


def np_health(Sigma, Na):
    """the report of ekf_dense64_health on Sigma[:Na, :Na], a dict of REPORT_FIELDS"""
    C = np.asarray(Sigma, dtype=np.float64)[:Na, :Na]
    i, j, a, b = _pairs(Sigma, Na)
    dg = np.ascontiguousarray(np.diagonal(C))
    most, k = _max_asym(a, b)
    ok = np.flatnonzero(~np.isnan(dg))
    at = int(ok[np.argmin(dg[ok])]) if ok.size else -1   # the first of equal values (-0.0 == +0.0)
    with np.errstate(all="ignore"):
        minor = (a * b) > (dg[i] * dg[j])   # a comparison with a NaN is False
        bad = ~(dg > 0.0)
    return {"n_nonfinite": int((~np.isfinite(C)).sum()), "n_asym": int((bits(a) != bits(b)).sum()),
            "n_diag_bad": int(bad.sum()), "n_minor": int(minor.sum()),
            "max_asym": most, "asym_i": int(i[k]) if k >= 0 else -1, "asym_j": int(j[k]) if k >= 0 else -1,
            "min_diag": float(dg[at]) if at >= 0 else float("inf"), "min_diag_i": at}


def np_symmetrize(Sigma, Na):
    """-> (Sigma after ekf_dense64_symmetrize with live = Na, n_changed, max_asym); Sigma itself is left alone"""
    out = np.array(Sigma, dtype=np.float64, copy=True)
    i, j, a, b = _pairs(out, Na)
    differ = bits(a) != bits(b)
    with np.errstate(all="ignore"):
        v = 0.5 * (a + b)
    out[i[differ], j[differ]] = v[differ]
    out[j[differ], i[differ]] = v[differ]
    return out, int(differ.sum()), _max_asym(a, b)[0]


# ---- the families: corner(family, Na) -> Na x Na ----------------------------------------------------------------------------

def _seed(family, Na):
    return 1000 * FAMILIES.index(family) + Na


def _symmetric_integers(Na, rng):
    U = np.triu(rng.integers(-9, 10, size=(Na, Na)), 1)
    return (U + U.T + np.diag(rng.integers(-2, 10, size=Na))).astype(np.float64)


def _asymmetric_integers(Na, rng):
    return rng.integers(-9, 10, size=(Na, Na)).astype(np.float64)


def _random_spd(Na, rng):
    """A A^T / k + c I with c = (largest |off-diagonal entry|) / 0.85, so every |correlation| <= 0.85 before and <= 0.9
    after each entry has moved by up to three ulps on its own"""
    A = rng.standard_normal((Na, Na + 3))
    S = A @ A.T / (Na + 3)
    S = 0.5 * (S + S.T)
    off = np.abs(S - np.diag(np.diagonal(S))).max() if Na > 1 else 0.0
    S = S + (off / 0.85 if off > 0.0 else 1.0) * np.eye(Na)
    moved = S.view(np.int64) + rng.integers(-3, 4, size=(Na, Na))
    return moved.view(np.float64).copy()


NAN_PAIR = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
NAN_LONE = np.array([0x7FF8000000000456], dtype=np.uint64).view(np.float64)[0]
DBL_MAX = np.finfo(np.float64).max
SUBNORMALS = np.array([3, 7], dtype=np.uint64).view(np.float64)   # odd last bits; their mean is the subnormal of bits 5
DEGENERATE_FULL = 11   # the smallest Na that holds every planted defect
# (i, j, Sigma[i][j], Sigma[j][i]); a defect is planted when j < Na
DEGENERATE_PAIRS = (
    (0, 1, NAN_PAIR, NAN_PAIR),         # a NaN pair with equal payloads: two non-finite entries, NOT asymmetric
    (0, 2, NAN_LONE, 3.0),              # a NaN against a number
    (1, 3, np.inf, -2.0),               # +Inf
    (2, 4, -0.0, 0.0),                  # -0.0 against +0.0: differ in bits, d = -0.0
    (3, 5, SUBNORMALS[0], SUBNORMALS[1]),
    (4, 6, DBL_MAX, 0.75 * DBL_MAX),    # the sum overflows: v = +Inf (and the product does: a minor violation)
    (9, 10, 150.0, 150.0),              # the planted minor violation: 150 * 150 > 100 * 100
)
DEGENERATE_DIAG = ((7, -4.0), (8, 0.0))   # rows and columns 7 and 8 are zero elsewhere


def _degenerate(Na, rng):
    """small symmetric integers under a diagonal of 100 (no minor violation of their own), then the defects above"""
    U = np.triu(rng.integers(-9, 10, size=(Na, Na)), 1)
    S = (U + U.T).astype(np.float64) + 100.0 * np.eye(Na)
    for k, v in DEGENERATE_DIAG:
        if k < Na:
            S[k, :] = 0.0
            S[:, k] = 0.0
            S[k, k] = v
    for i, j, a, b in DEGENERATE_PAIRS:
        if j < Na:
            S[i, j], S[j, i] = a, b
    return S


def degenerate_counts(Na):
    """what the defects of a full degenerate corner add up to, counted by hand (Na >= DEGENERATE_FULL):
    non-finite: the NaN pair (2), the lone NaN, +Inf; asymmetric: every planted pair but the NaN pair and the minor;
    diagonal: -4 and 0; minors: the planted one, the pair whose product overflows, and 0 * 0 > -4 * 100 for every partner
    of the negative diagonal entry except the zero one (0 > -0.0 is false)"""
    assert Na >= DEGENERATE_FULL
    return {"n_nonfinite": 4, "n_asym": 5, "n_diag_bad": 2, "n_minor": 2 + (Na - 2),
            "max_asym": NAN_LONE, "asym_i": 0, "asym_j": 2, "min_diag": -4.0, "min_diag_i": 7}


_MAKERS = {"symmetric_integers": _symmetric_integers, "asymmetric_integers": _asymmetric_integers,
           "random_spd": _random_spd, "degenerate": _degenerate}


def corner(family, Na):
    return _MAKERS[family](Na, np.random.default_rng(_seed(family, Na)))


def sizes(T):
    """the live dimensions of the GPU tests for a tile side T"""
    return [1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T + 2]
