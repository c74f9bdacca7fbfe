"""ekf_dense64_map_congruence / ekf_dense64_reframe_landmarks as include/ekfslam.h defines them: Sigma <- J Sigma J^T on the
live corner for J = D + [C | 0], D = blockdiag(1, G, ..., G) over the pairs (1, 2), (3, 4), ...; an op-by-op float64 model
(np_congruence: every product and every fused multiply-add rounded as the header says), an exact int64 model of J Sigma J^T,
the two state transforms with their Jacobians, and the corners the calls are tested on.  EVERY CORNER IS DELIBERATELY NOT
SYMMETRIC: the call never symmetrises, and a transposed access must show.
  integer families   Sigma non-zero integers with |.| <= 2^10, C integers with |.| <= 8 and G one of GS (two rotations and a matrix that
                     is none).  Every intermediate is an integer below 2^21, so every operation is exact in any order and
                     the comparison is bit for bit.
  slam_like          B B^T / 8 + diag(U(0.05, 1)) (dense_factor_cases' recipe with a floor that keeps the condition number
                     <= 1e4 at every size used; the host test checks it) plus an antisymmetric part of relative size 1e-6;
                     the state has its landmarks within 10 m of the pose."""
import math
from fractions import Fraction

import numpy as np

from dense_factor_cases import U, bits, gamma, payload_nan, same_bits   # noqa: F401  (shared helpers)

FIXED, ROBOT = 0, 1
GS = {"rot90": np.array([[0.0, -1.0], [1.0, 0.0]]), "rot180": np.array([[-1.0, 0.0], [0.0, -1.0]]),
      "shear": np.array([[2.0, 1.0], [1.0, 1.0]])}
COND_MAX = 1e4


def odd_near(v):
    """the odd number nearest v (v itself when odd, else v + 1), at least 3"""
    return max(3, v if v % 2 else v + 1)


def sizes(tr, tc):
    """Na around both tile sides: the odd numbers nearest {3, 5, 7, T - 1, T, T + 1, 2 T + 1, 3 T + 2}, T in {tr, tc}"""
    out = set()
    for T in (tr, tc):
        out |= {odd_near(v) for v in (3, 5, 7, T - 1, T, T + 1, 2 * T + 1, 3 * T + 2)}
    return sorted(out)


# ---- the families -----------------------------------------------------------------------------------------------------------

def integer_corner(Na, seed=0):
    rng = np.random.default_rng(4000 + 13 * Na + seed)
    S = rng.integers(-1024, 1025, size=(Na, Na)).astype(np.float64)
    S[S == 0.0] = 1.0                        # (fl(-1 * 0) is -0.0, which the int64 model cannot say: no zero entries)
    assert not np.array_equal(S, S.T) or Na == 1
    return S


def integer_C(Na, seed=0):
    return np.random.default_rng(5000 + 17 * Na + seed).integers(-8, 9, size=(Na, 3)).astype(np.float64)


def slam_like(Na, seed=0):
    rng = np.random.default_rng(2000 + 11 * Na + seed)
    B = rng.standard_normal((Na, 8))
    S = B @ B.T / 8 + np.diag(rng.uniform(0.05, 1.0, size=Na))
    S = np.tril(S) + np.tril(S, -1).T
    A = rng.standard_normal((Na, Na))
    return S + 1e-6 * (A - A.T)


def slam_state(Na, seed=0):
    """[theta, x, y, l1x, l1y, ...]: the landmarks within 10 m of the pose"""
    rng = np.random.default_rng(6000 + Na + seed)
    x = np.empty(Na)
    x[:3] = [0.8, 1.5, -2.25]
    r, a = rng.uniform(0.5, 10.0, size=(Na - 3) // 2), rng.uniform(-math.pi, math.pi, size=(Na - 3) // 2)
    x[3::2], x[4::2] = x[1] + r * np.cos(a), x[2] + r * np.sin(a)
    return x


def condition(S):
    sym = 0.5 * (S + S.T)
    w = np.linalg.eigvalsh(sym)
    return float(w[-1] / w[0])


# ---- fl(a b + c), one rounding ----------------------------------------------------------------------------------------------

def _fma1(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    prod = Fraction(a) * Fraction(b)
    v = prod + Fraction(c)
    if v == 0:                               # an exact zero: x + (-x) = +0.0; with a zero product the plain sum has the sign
        return a * b + c if prod == 0 else 0.0
    return float(v)                          # int / int: correctly rounded


_fma = np.vectorize(_fma1, otypes=[np.float64])


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    r = a * b + c
    whole = (a == np.rint(a)) & (b == np.rint(b)) & (c == np.rint(c)) & (np.abs(a * b) < 2.0 ** 52) & (np.abs(c) < 2.0 ** 52)
    if whole.all():
        return r                             # integers far below 2^53: the plain expression is exact
    return _fma(a, b, c)


def one_sided(g0, g1, b0, b1):
    """(b0, b1) against one row of G: fma(g1, b1, fl(g0 b0)) -- from the left and from the right the same expression"""
    return fma(g1, b1, g0 * b0)


# ---- the models -------------------------------------------------------------------------------------------------------------

def is_identity(G):
    return same_bits(np.asarray(G, dtype=np.float64).reshape(4), [1.0, 0.0, 0.0, 1.0])


def np_D_congruence(S, G):
    """step 1: P = D S D^T block by block, row 0 and column 0 one-sided"""
    Na = S.shape[0]
    G = np.asarray(G, dtype=np.float64)
    Y = np.empty_like(S)                     # Y = D S
    Y[0] = S[0]
    for r in range(2):
        Y[1 + r::2] = one_sided(G[r, 0], G[r, 1], S[1::2], S[2::2])
    P = np.empty_like(S)                     # P = Y D^T
    P[:, 0] = Y[:, 0]
    for c in range(2):
        P[:, 1 + c::2] = one_sided(G[c, 0], G[c, 1], Y[:, 1::2], Y[:, 2::2])
    assert P.shape == (Na, Na)
    return P


def np_congruence(S, G, C=None):
    """the header's definition on the Na x Na corner S, one rounded operation at a time -> the new corner"""
    S = np.array(S, dtype=np.float64)
    Na = S.shape[0]
    assert Na >= 3 and Na % 2 == 1
    G = np.asarray(G, dtype=np.float64).reshape(2, 2)
    if C is None:
        return S if is_identity(G) else np_D_congruence(S, G)
    C = np.asarray(C, dtype=np.float64)
    P = np_D_congruence(S, G)
    Sp, Sc, Spp = S[:3, :], S[:, :3], S[:3, :3]
    A = np.empty((3, Na))                    # step 2
    A[:, 0] = Sp[:, 0]
    for c in range(2):
        A[:, 1 + c::2] = one_sided(G[c, 0], G[c, 1], Sp[:, 1::2], Sp[:, 2::2])
    for l in range(3):
        A = fma(Spp[:, l][:, None], C[:, l][None, :], A)
    Bc = np.empty((Na, 3))
    Bc[0] = Sc[0]
    for r in range(2):
        Bc[1 + r::2] = one_sided(G[r, 0], G[r, 1], Sc[1::2], Sc[2::2])
    acc = P                                  # step 3
    for k in range(3):
        acc = fma(C[:, k][:, None], A[k][None, :], acc)
    for k in range(3):
        acc = fma(Bc[:, k][:, None], C[:, k][None, :], acc)
    return acc


def jacobian(Na, G, C=None, dtype=np.float64):
    J = np.zeros((Na, Na), dtype=dtype)
    J[0, 0] = 1
    G = np.asarray(G).reshape(2, 2)
    for j in range(1, Na, 2):
        J[j:j + 2, j:j + 2] = G
    if C is not None:
        J[:, :3] += np.asarray(C).astype(dtype)
    return J


def jacobian_rows(N, rows, G, C=None, dtype=np.float64):
    """the rows `rows` of the N x N Jacobian, without forming it"""
    G = np.asarray(G).reshape(2, 2).astype(dtype)
    out = np.zeros((len(rows), N), dtype=dtype)
    for a, i in enumerate(rows):
        if i == 0:
            out[a, 0] = 1
        else:
            p = i if i % 2 else i - 1
            out[a, p:p + 2] = G[i - p]
        if C is not None:
            out[a, :3] += np.asarray(C[i]).astype(dtype)
    return out


def times_jacobian_T(L, G, C, absolute):
    """L J^T for L of shape (r, N) in L's precision; absolute: L |J|^T (|J| = |D + [C | 0]|, entry by entry)"""
    dt = L.dtype.type
    N = L.shape[1]
    Gm = np.asarray(G).reshape(2, 2).astype(dt)
    Cm = None if C is None else np.asarray(C).astype(dt)
    if absolute:
        Gm, Cm = np.abs(Gm), None if Cm is None else np.abs(Cm)
    out = np.empty_like(L)
    out[:, 0] = L[:, 0]
    out[:, 1::2] = L[:, 1::2] * Gm[0, 0] + L[:, 2::2] * Gm[0, 1]
    out[:, 2::2] = L[:, 1::2] * Gm[1, 0] + L[:, 2::2] * Gm[1, 1]
    if Cm is not None:
        out[:, 3:] += L[:, :3] @ Cm[3:].T
        J3 = jacobian_rows(N, [0, 1, 2], G, C, dt)[:, :3]        # where D and C overlap: the sum first, then | |
        out[:, :3] = L[:, :3] @ (np.abs(J3) if absolute else J3).T
    return out


def exact_congruence(S, G, C=None):
    """J S J^T in int64 for integer operands (every entry of the families is one) -> float64, exact"""
    for a in (S, G) + (() if C is None else (C,)):
        assert np.array_equal(np.asarray(a), np.rint(a))
    J = jacobian(S.shape[0], np.asarray(G, dtype=np.int64), None if C is None else np.asarray(C, dtype=np.int64), np.int64)
    out = J @ np.asarray(S, dtype=np.int64) @ J.T
    assert np.abs(out).max() < 2 ** 53
    return out.astype(np.float64)


def bound_ratio(got, S, G, C=None):
    """max_ij |got - J S J^T|_ij / (gamma_16 (|J| |S| |J|^T)_ij), the products in extended precision"""
    J = jacobian(S.shape[0], G, C, np.longdouble)
    Sx = np.asarray(S, dtype=np.longdouble)
    res = np.abs(np.asarray(got, dtype=np.longdouble) - J @ Sx @ J.T)
    bound = np.longdouble(gamma(16)) * (np.abs(J) @ np.abs(Sx) @ np.abs(J).T)
    return float(np.max(res / bound))


# ---- the state ----------------------------------------------------------------------------------------------------------------

def g_fixed(x, dtheta, tx, ty, dtype=np.float64):
    """theta + dtheta (not wrapped), q -> R(dtheta) q + t"""
    x = np.asarray(x, dtype=dtype)
    c, s = dtype(math.cos(dtheta)), dtype(math.sin(dtheta))
    out = x.copy()
    out[0] = x[0] + dtype(dtheta)
    out[1::2] = c * x[1::2] - s * x[2::2] + dtype(tx)
    out[2::2] = s * x[1::2] + c * x[2::2] + dtype(ty)
    return out


def fixed_state_bound(x, dtheta, tx, ty):
    """gamma_4 (|c| |x| + |s| |y| + |t|) per entry (the heading: gamma_4 (|theta| + |dtheta|))"""
    c, s = abs(math.cos(dtheta)), abs(math.sin(dtheta))
    x = np.abs(np.asarray(x, dtype=np.float64))
    b = np.empty_like(x)
    b[0] = x[0] + abs(dtheta)
    b[1::2] = c * x[1::2] + s * x[2::2] + abs(tx)
    b[2::2] = s * x[1::2] + c * x[2::2] + abs(ty)
    return gamma(4) * b


def fixed_terms(dtheta):
    c, s = math.cos(dtheta), math.sin(dtheta)
    return np.array([[c, -s], [s, c]])


def g_robot(x, dtype=np.float64):
    """the inverse pose composition: theta' = -theta, p' = -M p, l' = M (l - p), M = R(-theta)"""
    x = np.asarray(x, dtype=dtype)
    c, s = np.cos(x[0]), np.sin(x[0])
    out = np.empty_like(x)
    out[0] = -x[0]
    dx, dy = x[3::2] - x[1], x[4::2] - x[2]
    out[1], out[2] = -(c * x[1] + s * x[2]), -(-s * x[1] + c * x[2])
    out[3::2], out[4::2] = c * dx + s * dy, -s * dx + c * dy
    return out


def robot_terms(x):
    """-> G = M (2 x 2), C (Na x 3): theta row [-2, 0, 0], position rows [-M' p | -2 M], landmark i [M' (l_i - p) | -M]"""
    x = np.asarray(x, dtype=np.float64)
    Na = x.shape[0]
    c, s = math.cos(x[0]), math.sin(x[0])
    M, Md = np.array([[c, s], [-s, c]]), np.array([[-s, c], [-c, -s]])
    C = np.zeros((Na, 3))
    C[0] = [-2.0, 0.0, 0.0]
    C[1:3, 0] = -Md @ x[1:3]
    C[1:3, 1:] = -2.0 * M
    d = np.stack([x[3::2] - x[1], x[4::2] - x[2]])          # 2 x n
    md = Md @ d
    C[3::2, 0], C[4::2, 0] = md[0], md[1]
    C[3::2, 1:], C[4::2, 1:] = -M[0], -M[1]
    return M, C


def row_scale_err(got, want):
    """max_i max_j |got - want|_ij / max_j |want|_ij: the error relative to the scale of its row"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    scale = np.maximum(np.abs(want).max(axis=1, keepdims=True), np.finfo(np.float64).tiny)
    return float(np.max(np.abs(got - want) / scale))
