"""ekf_dense64_join_congruence / ekf_dense64_join_map as include/ekfslam.h defines them: the live corner of a source handle
(map B, Nb states, in the frame of A's robot pose and independent of A) joined onto the live corner of a destination (map A,
Na states).  With D = blockdiag(1, G, ..., G) over B's pairs (1, 2), (3, 4), ..., E (Nb x 3) on A's pose and
iota: 0, 1, 2 -> 0, 1, 2, 3 + t -> Na + t:  Y = D Sigma_B D^T + E Sigma_pp E^T at iota x iota, E P and Pc E^T beside it,
Sigma_A[3:Na, 3:Na] untouched.  Here: an op-by-op float64 model (np_join: every product and every fused multiply-add rounded
as the header says), an exact int64 model of J blockdiag(Sigma_A, Sigma_B) J^T, the composition g with its Jacobian terms, a
long-double reference with the header's componentwise bound, and the sizes the GPU test runs.  The families are
dense_frame_cases': EVERY CORNER IS DELIBERATELY NOT SYMMETRIC, so a transposed access shows.
  integer families   Sigma_A, Sigma_B non-zero integers with |.| <= 2^10, E non-zero integers with |.| <= 8 (a zero row of E
                     would give -0.0 where the int64 model says 0), G one of GS.  Every intermediate is an integer below 2^21."""
import math

import numpy as np

from dense_frame_cases import (GS, fma, gamma, integer_corner, jacobian as frame_jacobian, np_D_congruence,   # noqa: F401
                               odd_near, payload_nan, row_scale_err, same_bits, slam_like, slam_state)
from dense_frame_cases import sizes as frame_sizes

OPS = 14   # rounded operations an entry of Y sees: 4 products and 4 fused steps of Z, 3 of W, 3 of W E^T (a cross entry: 3)


def sizes(tr, tc):
    """the distinct odd numbers nearest {3, 5, 7, T - 1, T, T + 1, 2 T + 1, 3 T + 2}, T in {tr, tc}"""
    return frame_sizes(tr, tc)


def integer_E(Nb, seed=0):
    rng = np.random.default_rng(9000 + 19 * Nb + seed)
    return (rng.integers(1, 9, size=(Nb, 3)) * rng.choice([-1, 1], size=(Nb, 3))).astype(np.float64)


def iota(Na, Nb):
    """where B's indices go in the joined map"""
    return np.concatenate([np.arange(3), np.arange(Na, Na + Nb - 3)])


# ---- the models -------------------------------------------------------------------------------------------------------------

def np_join(SA, SB, G, E):
    """the header's definition on the corners SA (Na x Na) and SB (Nb x Nb), one rounded operation at a time -> the joined
    corner (Na + Nb - 3 square)"""
    SA, SB = np.array(SA, dtype=np.float64), np.array(SB, dtype=np.float64)
    Na, Nb = SA.shape[0], SB.shape[0]
    assert Na >= 3 and Na % 2 == 1 and Nb >= 3 and Nb % 2 == 1
    G, E = np.asarray(G, dtype=np.float64).reshape(2, 2), np.asarray(E, dtype=np.float64)
    assert E.shape == (Nb, 3)
    P, Pc, Spp = SA[:3, :], SA[:, :3], SA[:3, :3]
    Z = np_D_congruence(SB, G)                                   # step 1
    W = E[:, [0]] * Spp[0][None, :]                              # step 2
    for t in (1, 2):
        W = fma(E[:, [t]], Spp[t][None, :], W)
    Y = Z                                                        # step 3
    for l in range(3):
        Y = fma(W[:, [l]], E[:, l][None, :], Y)
    Xr = E[:, [0]] * P[0][None, :]                               # step 4
    Xc = Pc[:, [0]] * E[:, 0][None, :]
    for l in (1, 2):
        Xr = fma(E[:, [l]], P[l][None, :], Xr)
        Xc = fma(Pc[:, [l]], E[:, l][None, :], Xc)
    Nj, io, mid = Na + Nb - 3, iota(Na, Nb), np.arange(3, Na)    # step 5
    out = np.empty((Nj, Nj))
    out[3:Na, 3:Na] = SA[3:Na, 3:Na]
    out[np.ix_(io, io)] = Y
    out[np.ix_(io, mid)] = Xr[:, 3:Na]
    out[np.ix_(mid, io)] = Xc[3:Na, :]
    return out


def jacobian(Na, Nb, G, E, dtype=np.float64):
    """the Jacobian of the joined state on (A, B): (Na + Nb - 3) x (Na + Nb)"""
    J = np.zeros((Na + Nb - 3, Na + Nb), dtype=dtype)
    J[np.arange(3, Na), np.arange(3, Na)] = 1
    io = iota(Na, Nb)
    J[io, :3] = np.asarray(E).astype(dtype)
    J[np.ix_(io, np.arange(Na, Na + Nb))] = frame_jacobian(Nb, G, None, dtype)
    return J


def blockdiag(SA, SB, dtype=np.float64):
    Na, Nb = SA.shape[0], SB.shape[0]
    S = np.zeros((Na + Nb, Na + Nb), dtype=dtype)
    S[:Na, :Na], S[Na:, Na:] = SA, SB
    return S


def exact_join(SA, SB, G, E):
    """J blockdiag(SA, SB) J^T in int64 for integer operands -> float64, exact"""
    for a in (SA, SB, G, E):
        assert np.array_equal(np.asarray(a), np.rint(a))
    J = jacobian(SA.shape[0], SB.shape[0], np.asarray(G, dtype=np.int64), np.asarray(E, dtype=np.int64), np.int64)
    out = J @ blockdiag(SA, SB, np.int64) @ J.T
    assert np.abs(out).max() < 2 ** 53
    return out.astype(np.float64)


def reference_full(SA, SB, G, E):
    """(J S J^T, |J| |S| |J|^T) in extended precision, the full products (small sizes)"""
    J = jacobian(SA.shape[0], SB.shape[0], G, E, np.longdouble)
    S = blockdiag(SA, SB, np.longdouble)
    return J @ S @ J.T, np.abs(J) @ np.abs(S) @ np.abs(J).T


def _D_times(X, G):
    Y = X.copy()
    Y[1::2], Y[2::2] = G[0, 0] * X[1::2] + G[0, 1] * X[2::2], G[1, 0] * X[1::2] + G[1, 1] * X[2::2]
    return Y


def reference(SA, SB, G, E):
    """the same two matrices block by block, without a product that is N^3 in long double (the host test holds it against
    reference_full)"""
    Na, Nb = SA.shape[0], SB.shape[0]
    io, mid = iota(Na, Nb), np.arange(3, Na)
    outs = []
    for absolute in (False, True):
        f = (lambda a: np.abs(np.asarray(a, dtype=np.longdouble))) if absolute else (lambda a: np.asarray(a, dtype=np.longdouble))
        A, B, Gx, Ex = f(SA), f(SB), f(G).reshape(2, 2), f(E)
        out = np.empty((Na + Nb - 3,) * 2, dtype=np.longdouble)
        out[3:Na, 3:Na] = A[3:, 3:]
        out[np.ix_(io, io)] = _D_times(_D_times(B, Gx).T, Gx).T + Ex @ A[:3, :3] @ Ex.T
        out[np.ix_(io, mid)] = Ex @ A[:3, 3:]
        out[np.ix_(mid, io)] = A[3:, :3] @ Ex.T
        outs.append(out)
    return outs[0], outs[1]


CROSS_OPS = 3   # a cross entry (exactly one index among A's landmarks): one product and two fused steps


def entry_gamma(Na, rows, cols):
    """the header's gamma per entry of the joined map: gamma_14 where both indices are the pose's or B's, gamma_3 where
    exactly one is among A's landmarks [3, Na), and 0 -- the entry is not touched, so it is exact -- where both are"""
    a, b = (np.asarray(rows) >= 3) & (np.asarray(rows) < Na), (np.asarray(cols) >= 3) & (np.asarray(cols) < Na)
    return np.where(a & b, 0.0, np.where(a | b, gamma(CROSS_OPS), gamma(OPS))).astype(np.longdouble)


def bound_ratio(got, SA, SB, G, E):
    """max_ij |got - J S J^T|_ij / (gamma_k (|J| |S| |J|^T)_ij), k per entry as entry_gamma says; where the bound is 0 the
    entry must be exact"""
    want, mag = reference(SA, SB, G, E)
    res = np.abs(np.asarray(got, dtype=np.longdouble) - want)
    idx = np.arange(want.shape[0])
    bound = entry_gamma(SA.shape[0], idx[:, None], idx[None, :]) * mag
    assert np.all(res[bound == 0] == 0)
    return float(np.max(res[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def jacobian_row(Na, Nb, G, E, r):
    """row r of the Jacobian without forming it -> (column indices into (A, B), values in long double)"""
    if 3 <= r < Na:
        return np.array([r]), np.ones(1, dtype=np.longdouble)
    k = r if r < 3 else r - Na + 3
    G = np.asarray(G, dtype=np.longdouble).reshape(2, 2)
    if k == 0:
        cols, vals = [Na], [np.longdouble(1)]
    else:
        p = k if k % 2 else k - 1
        cols, vals = [Na + p, Na + p + 1], list(G[k - p])
    return np.array([0, 1, 2] + cols), np.concatenate([np.asarray(E[k], dtype=np.longdouble), np.array(vals, dtype=np.longdouble)])


def sampled_bound_ratio(got, SA, Na, SB, Nb, G, E, rows, cols):
    """max over the samples t of |got[t] - (J S J^T)[rows[t], cols[t]]| / (gamma_k (|J| |S| |J|^T)[rows[t], cols[t]]), k per
    entry as entry_gamma says (an untouched entry must be exact), the
    two rows of J taken one at a time: nothing N x N is formed.  SA, SB: arrays whose leading corners are the operands."""
    def S(p, q):
        if p < Na and q < Na:
            return np.longdouble(SA[p, q])
        if p >= Na and q >= Na:
            return np.longdouble(SB[p - Na, q - Na])
        return np.longdouble(0)
    worst = 0.0
    for v, r, c in zip(got, rows, cols):
        ci, cv = jacobian_row(Na, Nb, G, E, int(r))
        di, dv = jacobian_row(Na, Nb, G, E, int(c))
        M = np.array([[S(p, q) for q in di] for p in ci], dtype=np.longdouble)
        want, mag = cv @ M @ dv, np.abs(cv) @ np.abs(M) @ np.abs(dv)
        err, bound = abs(np.longdouble(v) - want), entry_gamma(Na, int(r), int(c)) * mag
        assert bound > 0 or err == 0, (r, c)                      # (an untouched entry is exact)
        if bound > 0:
            worst = max(worst, float(err / bound))
    return worst


# ---- the state ----------------------------------------------------------------------------------------------------------------

def g(xa, xb, dtype=np.float64):
    """the joined state: (theta_A + theta_B (not wrapped), p_A + M p_B, A's landmarks, p_A + M m_j), M = R(theta_A)"""
    xa, xb = np.asarray(xa, dtype=dtype), np.asarray(xb, dtype=dtype)
    Na, Nb = xa.shape[0], xb.shape[0]
    c, s = np.cos(xa[0]), np.sin(xa[0])
    out = np.empty(Na + Nb - 3, dtype=dtype)
    out[:Na] = xa
    io = iota(Na, Nb)
    out[0] = xa[0] + xb[0]
    out[io[1::2]] = xa[1] + c * xb[1::2] - s * xb[2::2]
    out[io[2::2]] = xa[2] + s * xb[1::2] + c * xb[2::2]
    return out


def join_terms(xa, xb):
    """-> G = M = R(theta_A) (2 x 2), E (Nb x 3): row 0 [1, 0, 0], rows (1, 2) [M' p_B | I], rows (3 + 2 j, 4 + 2 j) [M' m_j | I]"""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    c, s = math.cos(xa[0]), math.sin(xa[0])
    M, Md = np.array([[c, -s], [s, c]]), np.array([[-s, -c], [c, -s]])
    E = np.zeros((xb.shape[0], 3))
    E[0, 0] = 1.0
    md = Md @ np.stack([xb[1::2], xb[2::2]])
    E[1::2, 0], E[2::2, 0] = md[0], md[1]
    E[1::2, 1], E[2::2, 2] = 1.0, 1.0
    return M, E


def state_model(xa, xb, c, s):
    """ekf_dense64_join_map's state and E, operation by operation, given the cos and sin the device used -> (state', E)"""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    Na, Nb = xa.shape[0], xb.shape[0]
    mx = fma(-s, xb[2::2], c * xb[1::2])
    my = fma(c, xb[2::2], s * xb[1::2])
    out = np.empty(Na + Nb - 3)
    out[:Na] = xa
    io = iota(Na, Nb)
    out[0] = xa[0] + xb[0]
    out[io[1::2]], out[io[2::2]] = mx + xa[1], my + xa[2]
    E = np.zeros((Nb, 3))
    E[0, 0] = 1.0
    E[1::2, 0], E[2::2, 0] = -my, mx
    E[1::2, 1], E[2::2, 2] = 1.0, 1.0
    return out, E
