"""ekf_dense64_factor / ekf_dense64_get_factor / ekf_dense64_whiten as include/ekfslam.h defines them: an op-by-op float64
numpy model (columns ascending, the lower triangle only, the stop rule, logdet summed on the host with math.log) and the
families of live corners they are tested on.
  integer_factor        L0 lower triangular, integers in [-3, 3], diagonal from {1, 2, 4}; the corner is L0 L0^T.  Every
                        intermediate of a Cholesky factorisation is an integer far below 2^53, every square root is of a
                        perfect square and every quotient an integer: ANY correct factorisation in ANY order of summation
                        returns L0 bit for bit (test_dense64_factor_host.py proves it in Fraction arithmetic).
  integer_indefinite    the same with corner[p][p] -= L0[p][p]^2 + c: the exact pivot at p is -c
  nan_entry             the same with a payload NaN at corner[i][j], j < i: the pivot at i is a NaN
  slam_like             B B^T / 8 + diag(U(1e-3, 1)), B of shape Na x 8, exactly symmetric; slam_like_input() overwrites the
                        strict upper triangle with garbage to show that only the lower triangle is read."""
import math

import numpy as np

REPORT_FIELDS = ("ok", "fail_index", "min_pivot_i", "Na", "fail_pivot", "min_pivot", "max_pivot", "logdet")
BLOCK_SIDES = (16, 32, 64, 128)        # what ekf_dense64_factor_launch_info may report: a divisor of 128, >= 16
U = 2.0 ** -53


def sizes(nb):
    return [1, 2, 3, nb - 1, nb, nb + 1, 2 * nb + 1, 3 * nb + 2]


def fail_columns(nb, Na):
    return sorted({p for p in (0, 1, nb - 1, nb, nb + 1, Na - 1) if 0 <= p < Na})


def gamma(n):
    return n * U / (1.0 - n * U)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def same_report(got, want):
    """bit for bit -- but a pivot that is a NaN only has to be a NaN: it has gone through a division, a product of two
    NaNs and a subtraction, and which payload and sign those hand on is the hardware's business"""
    def same(k):
        if not isinstance(want[k], float):
            return got[k] == want[k]
        if k == "fail_pivot" and math.isnan(want[k]):
            return math.isnan(got[k])
        return same_bits(got[k], want[k])
    return all(same(k) for k in REPORT_FIELDS)


# ---- the families ---------------------------------------------------------------------------------------------------------

def integer_L0(Na, seed=0):
    rng = np.random.default_rng(1000 + 7 * Na + seed)
    L0 = np.tril(rng.integers(-3, 4, size=(Na, Na)).astype(np.float64), -1)
    L0[np.arange(Na), np.arange(Na)] = rng.choice([1.0, 2.0, 4.0], size=Na)
    return L0


def integer_factor(Na, seed=0):
    """-> (corner, L0)"""
    L0 = integer_L0(Na, seed)
    return L0 @ L0.T, L0


def integer_indefinite(Na, p, c, seed=0):
    C, L0 = integer_factor(Na, seed)
    C[p, p] -= L0[p, p] ** 2 + c
    return C, L0


def payload_nan(k):
    return np.array([0x7FF8000000000000 + 0x5A5A00 + k], dtype=np.uint64).view(np.float64)[0]


def nan_entry(Na, i, j, seed=0):
    assert 0 <= j < i < Na
    C, L0 = integer_factor(Na, seed)
    C[i, j] = payload_nan(i)
    return C, L0


def slam_like(Na, seed=0):
    """the symmetric matrix itself"""
    rng = np.random.default_rng(2000 + 11 * Na + seed)
    B = rng.standard_normal((Na, 8))
    S = B @ B.T / 8 + np.diag(rng.uniform(1e-3, 1.0, size=Na))
    return np.tril(S) + np.tril(S, -1).T


def slam_like_input(Na, seed=0):
    """what the handle is given: the lower triangle of slam_like(), garbage above the diagonal"""
    S = slam_like(Na, seed)
    rng = np.random.default_rng(3000 + Na + seed)
    junk = np.where(rng.random((Na, Na)) < 0.5, payload_nan(1), 1e300 * rng.standard_normal((Na, Na)))
    up = np.triu(np.ones((Na, Na), dtype=bool), 1)
    S[up] = junk[up]
    return S


# ---- the model ------------------------------------------------------------------------------------------------------------

def np_factor(C):
    """the definition, one rounded operation at a time, reading C[i][j] with j <= i only -> (report, L); after a failed
    pivot L holds the columns before it"""
    Na = C.shape[0]
    L = np.zeros((Na, Na))
    rep = dict(ok=1, fail_index=-1, min_pivot_i=-1, Na=Na, fail_pivot=0.0, min_pivot=math.inf, max_pivot=0.0, logdet=math.nan)
    for j in range(Na):
        d = C[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if not (d > 0.0 and d < math.inf):
            rep.update(ok=0, fail_index=j, fail_pivot=float(d))
            return rep, L
        if d < rep["min_pivot"]:
            rep.update(min_pivot=float(d), min_pivot_i=j)
        rep["max_pivot"] = max(rep["max_pivot"], float(d))
        L[j, j] = math.sqrt(d)
        col = C[j + 1:, j].copy()
        for k in range(j):
            col = col - L[j + 1:, k] * L[j, k]
        L[j + 1:, j] = col / L[j, j]
    rep["logdet"] = host_logdet(np.diagonal(L))
    return rep, L


def host_logdet(diag):
    """2.0 * (((log l_0) + log l_1) + ...), ascending, the C library's log"""
    s = 0.0
    for l in diag:
        s = s + math.log(float(l))
    return 2.0 * s


def np_whiten(L, B):
    """Y[r] = L^-1 B[r] by ascending forward substitution, d2[r] = sum Y[r]^2 (ascending)"""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    Y = np.zeros_like(B)
    for i in range(L.shape[0]):
        s = B[:, i].copy()
        for k in range(i):
            s = s - L[i, k] * Y[:, k]
        Y[:, i] = s / L[i, i]
    d2 = np.zeros(B.shape[0])
    for i in range(L.shape[0]):
        d2 = d2 + Y[:, i] * Y[:, i]
    return Y, d2


# ---- the derived bounds (Higham, Accuracy and Stability of Numerical Algorithms, Theorems 10.3 and 8.5: componentwise,
# valid for any order of summation and with fused multiply-adds) -------------------------------------------------------------

def factor_residual_ratio(A, L):
    """max over i >= j of |A - L L^T|_ij / (gamma_{Na+1} (|L| |L|^T)_ij), the product formed in extended precision"""
    Na = A.shape[0]
    Lx = np.asarray(L, dtype=np.longdouble)
    res = np.abs(np.asarray(A, dtype=np.longdouble) - Lx @ Lx.T)
    bound = np.longdouble(gamma(Na + 1)) * (np.abs(Lx) @ np.abs(Lx).T)
    low = np.tril(np.ones((Na, Na), dtype=bool))
    return float(np.max(res[low] / bound[low]))


def logdet_bound(A, L):
    """2 Na gamma_{Na+1} || |L| |L|^T ||_2 || A^-1 ||_2: the first-order perturbation of log det under the backward error of
    the factorisation, doubled for the higher orders"""
    Na = A.shape[0]
    absL = np.abs(L)
    return 2.0 * Na * gamma(Na + 1) * np.linalg.norm(absL @ absL.T, 2) * np.linalg.norm(np.linalg.inv(A), 2)


def whiten_residual_ratio(L, y, b):
    """max_i |L y - b|_i / (gamma_Na (|L| |y|)_i) in extended precision"""
    Na = L.shape[0]
    Lx, yx = np.asarray(L, dtype=np.longdouble), np.asarray(y, dtype=np.longdouble)
    res = np.abs(Lx @ yx - np.asarray(b, dtype=np.longdouble))
    bound = np.longdouble(gamma(Na)) * (np.abs(Lx) @ np.abs(yx))
    return float(np.max(res / bound))


def norm_ratio(y, d2):
    """|d2 - y.y| / (gamma_Na d2), y.y in extended precision"""
    yx = np.asarray(y, dtype=np.longdouble)
    return float(abs(np.longdouble(d2) - yx @ yx) / (np.longdouble(gamma(len(y))) * np.longdouble(d2)))
