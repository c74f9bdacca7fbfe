"""Shared by tests/test_gpu_dense64_value.py and tests/test_dense64_value_host.py: what observing each landmark would gain
(ekf_dense64_value_operands, include/ekfslam.h).  A float64 numpy model that performs the defined operations in the defined
order (parametrised by tile_rows, which fixes the order of the sums), an exact model in integers and Fractions, a
long-double model with the componentwise bound of the model against it, the bound of the closed forms against an actual
correction, and the data families."""
from fractions import Fraction

import numpy as np

import dense_invert_cases as di
from dense_factor_cases import U, bits, gamma, same_bits   # noqa: F401  (shared helpers)
from dense_frame_cases import fma

LD = np.longdouble


def lm_cols(i):
    return np.array([0, 1, 2, 3 + 2 * i, 4 + 2 * i], dtype=np.int32)


def all_cols(first_lm, count):
    return np.stack([lm_cols(first_lm + j) for j in range(count)])


def sizes(tile_rows, tile_lm):
    """n_lm with Na = 3 + 2 n_lm just below, on (Na is odd: where tile_rows is, too) and just above one and two tile_rows,
    around one landmark tile, and the smallest map"""
    around = lambda rows: {(rows - 3) // 2 - (rows % 2 == 0), (rows - 3) // 2, (rows - 3) // 2 + 1}   # noqa: E731
    n = {1} | around(tile_rows) | around(2 * tile_rows) | {tile_lm - 1, tile_lm, tile_lm + 1}
    return sorted(k for k in n if k >= 1)


# ---- the models ---------------------------------------------------------------------------------------------------------------

def model_S(C, first_lm, Hc, R):
    """S [n][2][2] as k_dsp_score forms it at m = 2, s = 5: T'[a][b] = fma chain of Hc[a][k] G[k][b] from +0 in ascending k,
    S[a][b] = (fma chain of T'[a][k] Hc[b][k]) + R[a][b]; G = Sigma[cols, cols]"""
    n = len(Hc)
    cols = all_cols(first_lm, n)
    G = C[cols[:, :, None], cols[:, None, :]]
    with np.errstate(all="ignore"):
        T = np.zeros((n, 2, 5))
        for k in range(5):
            T = fma(Hc[:, :, k, None], G[:, None, k, :], T)
        S = np.zeros((n, 2, 2))
        for k in range(5):
            S = fma(T[:, :, None, k], Hc[:, None, :, k], S)
        return S + R[None]


def _rows_of(C, Na, first_lm, n, dtype):
    idx = first_lm + np.arange(n)
    s = np.empty((Na, n, 5), dtype=dtype)
    s[:, :, 0:3] = C[:Na, None, 0:3]
    s[:, :, 3] = C[:Na, 3 + 2 * idx]
    s[:, :, 4] = C[:Na, 4 + 2 * idx]
    return s


def model_G(C, Na, first_lm, Hc, tile_rows):
    """-> G [n][3] = (G00, G01, G11), P [n][3]: u from +0 in ascending k, the products rounded on their own, the sums from +0
    in ascending r inside a row tile, then the tiles' sums from +0 in ascending tile"""
    n = len(Hc)
    s = _rows_of(np.asarray(C, dtype=np.float64), Na, first_lm, n, np.float64)
    with np.errstate(all="ignore"):
        u = np.zeros((Na, n, 2))
        for k in range(5):
            u = u + s[:, :, k, None] * Hc[None, :, :, k]
        a = np.stack([u[:, :, 0] * u[:, :, 0], u[:, :, 0] * u[:, :, 1], u[:, :, 1] * u[:, :, 1]], axis=2)   # [Na][n][3]
        G = np.zeros((n, 3))
        for r0 in range(0, Na, tile_rows):
            acc = np.zeros((n, 3))
            for r in range(r0, min(Na, r0 + tile_rows)):
                acc = acc + a[r]
            G = G + acc
        P = np.zeros((n, 3))
        for r in range(min(3, Na)):
            P = P + a[r]
    return G, P


def trace_chain(A, g):
    """((A00 g00 + A01 g01) + A10 g01) + A11 g11, every operation in the type of the operands"""
    return ((A[0, 0] * g[0] + A[0, 1] * g[1]) + A[1, 0] * g[1]) + A[1, 1] * g[2]


def better(v, i, bv, bi):
    """does (v, i) beat (bv, bi)?  the larger value, then the lower index; a NaN never; bi < 0: nothing yet"""
    return v == v and (bi < 0 or v > bv or (v == bv and i < bi))


def winners(values, flags, in_view):
    out = {}
    for name, v in values.items():
        bv, bi = float("nan"), -1
        for j in range(len(v)):
            if flags[j] == 0 and in_view[j] and better(v[j], j, bv, bi):
                bv, bi = float(v[j]), j
        out["i_" + name], out["v_" + name] = bi, bv
    return out


def np_value(C, Na, first_lm, Hc, R, tile_rows, in_view=None):
    """the whole call in float64 -> dict(dtrace, dtrace_pose, detS, S, flags, G, P, best)"""
    Hc, R = np.asarray(Hc, dtype=np.float64), np.asarray(R, dtype=np.float64)
    n = len(Hc)
    S = model_S(C, first_lm, Hc, R)
    G, P = model_G(C, Na, first_lm, Hc, tile_rows)
    dt, dp, det = (np.full(n, np.nan) for _ in range(3))
    flags = np.ones(n, dtype=np.int32)
    with np.errstate(all="ignore"):
        for j in range(n):
            e = di.eliminate(S[j])
            if e["verdict"]:
                continue
            flags[j] = 0
            dt[j], dp[j] = trace_chain(e["X"], G[j]), trace_chain(e["X"], P[j])
            det[j] = S[j, 0, 0] * S[j, 1, 1] - S[j, 0, 1] * S[j, 1, 0]
    view = np.ones(n, dtype=np.uint8) if in_view is None else np.asarray(in_view)
    return dict(dtrace=dt, dtrace_pose=dp, detS=det, S=S, flags=flags, G=G, P=P,
                best=winners(dict(trace=dt, pose=dp, det=det), flags, view))


def exact_value(C, Na, first_lm, Hc, R):
    """the integer family in Python integers and Fractions -> dict as np_value's plus `exact`: every u, every partial sum of G
    in ANY order (the sum of the magnitudes) and S stay below 2^53, and the Fraction elimination of S produced doubles only"""
    Ci = np.asarray(C[:Na, :Na]).astype(np.int64)
    Hi, Ri = np.asarray(Hc).astype(np.int64), np.asarray(R).astype(np.int64)
    assert (Ci == C[:Na, :Na]).all() and (Hi == Hc).all() and (Ri == R).all()
    n = len(Hi)
    s = _rows_of(Ci, Na, first_lm, n, np.int64)
    u = np.einsum("rnk,nak->rna", s, Hi)
    uabs = np.einsum("rnk,nak->rna", np.abs(s), np.abs(Hi))
    a = np.stack([u[:, :, 0] * u[:, :, 0], u[:, :, 0] * u[:, :, 1], u[:, :, 1] * u[:, :, 1]], axis=2)
    G, P = a.sum(axis=0), a[:3].sum(axis=0)
    cols = all_cols(first_lm, n)
    G5 = Ci[cols[:, :, None], cols[:, None, :]]
    S = np.einsum("nak,nkl,nbl->nab", Hi, G5, Hi) + Ri[None]
    Sabs = np.einsum("nak,nkl,nbl->nab", np.abs(Hi), np.abs(G5), np.abs(Hi)) + np.abs(Ri)[None]
    exact = bool(max(uabs.max() ** 2 * Na, Sabs.max(), np.abs(a).sum(axis=0).max()) < 2 ** 52)
    dt, dp, det, dtdet = [], [], [], []
    flags = np.zeros(n, dtype=np.int32)
    for j in range(n):
        e = di.eliminate(S[j].astype(np.float64), number=Fraction)
        d = int(S[j, 0, 0] * S[j, 1, 1] - S[j, 0, 1] * S[j, 1, 0])
        det.append(float(d))
        if e["verdict"]:
            flags[j] = 1
            dt.append(float("nan")); dp.append(float("nan")); dtdet.append(None)
            continue
        exact = exact and e["inexact"] == 0
        g, p = [int(v) for v in G[j]], [int(v) for v in P[j]]
        t, tp = trace_chain(e["X"], g), trace_chain(e["X"], p)
        for v in (t, tp, e["X"][0, 0] * g[0], e["X"][0, 1] * g[1], e["X"][1, 1] * g[2]):
            exact = exact and Fraction(float(v)) == v
        dt.append(float(t)); dp.append(float(tp))
        dtdet.append(t * d)   # = tr(adj(S) G), an integer
    return dict(dtrace=np.array(dt), dtrace_pose=np.array(dp), detS=np.array(det), S=S.astype(np.float64), flags=flags,
                G=G.astype(np.float64), P=P.astype(np.float64), dtrace_det=dtdet, exact=exact)


def long_value(C, Na, first_lm, Hc, R):
    """the closed forms in long double from the same float64 inputs, and the componentwise bound of the float64 model (and of
    the device) against them.  With u_a = sum_k s_k h_ak (5 products, 5 sums), G_ab = sum_r u_a u_b (Na products and sums)
    and sabs_a = sum_k |s_k| |h_ak|:  |fl(G_ab) - G_ab| <= gamma_{Na + 12} sum_r sabs_a sabs_b =: eG_ab.
    S is 35 fused operations and one sum a entry: |dS| <= gamma_12 (|Hc| |G5| |Hc|^T + |R|); the elimination of a 2 x 2
    adds gamma_8 |S| (backward), so to first order |dA| <= |A| (|dS| + gamma_8 |S|) |A|, doubled for the higher orders.
    Then |d tr(A G)| <= sum_ab (|A_ab| eG_ab + dA_ab (|G_ab| + eG_ab)) + gamma_4 sum_ab |A_ab| |G_ab|  (the chain itself).
    -> dict(dtrace, dtrace_pose, detS, bound_trace, bound_pose, bound_det, A, Gabs, Pabs: the sums of sabs_a sabs_b)"""
    n = len(Hc)
    Cl, Hl, Rl = np.asarray(C, dtype=LD), np.asarray(Hc, dtype=LD), np.asarray(R, dtype=LD)
    s = _rows_of(Cl, Na, first_lm, n, LD)
    u = np.einsum("rnk,nak->rna", s, Hl)
    ua = np.einsum("rnk,nak->rna", np.abs(s), np.abs(Hl))
    full = lambda w, rows: np.stack([(w[rows, :, 0] * w[rows, :, 0]).sum(0), (w[rows, :, 0] * w[rows, :, 1]).sum(0),   # noqa: E731
                                     (w[rows, :, 1] * w[rows, :, 1]).sum(0)], axis=1)
    every, pose = slice(0, Na), slice(0, 3)
    G, P, Ga, Pa = full(u, every), full(u, pose), full(ua, every), full(ua, pose)
    cols = all_cols(first_lm, n)
    G5 = Cl[cols[:, :, None], cols[:, None, :]]
    S = np.einsum("nak,nkl,nbl->nab", Hl, G5, Hl) + Rl[None]
    Sa = np.einsum("nak,nkl,nbl->nab", np.abs(Hl), np.abs(G5), np.abs(Hl)) + np.abs(Rl)[None]
    g = lambda k: LD(gamma(k))   # noqa: E731
    out = dict(dtrace=np.empty(n, LD), dtrace_pose=np.empty(n, LD), detS=np.empty(n, LD), bound_trace=np.empty(n, LD),
               bound_pose=np.empty(n, LD), bound_det=np.empty(n, LD), A=[], Gabs=Ga, Pabs=Pa)
    for j in range(n):
        det = S[j, 0, 0] * S[j, 1, 1] - S[j, 0, 1] * S[j, 1, 0]
        A = np.array([[S[j, 1, 1], -S[j, 0, 1]], [-S[j, 1, 0], S[j, 0, 0]]], dtype=LD) / det
        dS = g(12) * Sa[j]
        dA = 2 * np.abs(A) @ (dS + g(8) * np.abs(S[j])) @ np.abs(A)
        for name, M, Ma, rows in (("trace", G[j], Ga[j], Na), ("pose", P[j], Pa[j], 3)):
            eG = g(rows + 12) * Ma
            pairs = ((0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 2))
            out["d" + name if name == "trace" else "dtrace_pose"][j] = sum(A[a, b] * M[c] for a, b, c in pairs)
            out["bound_" + name][j] = sum(abs(A[a, b]) * eG[c] + dA[a, b] * (abs(M[c]) + eG[c]) + g(4) * abs(A[a, b] * M[c])
                                          for a, b, c in pairs)
        out["detS"][j] = det
        out["bound_det"][j] = g(3) * (abs(S[j, 0, 0] * S[j, 1, 1]) + abs(S[j, 0, 1] * S[j, 1, 0])) + \
            2 * (dS[0, 0] * abs(S[j, 1, 1]) + dS[1, 1] * abs(S[j, 0, 0]) + dS[0, 1] * abs(S[j, 1, 0]) + dS[1, 0] * abs(S[j, 0, 1]))
        out["A"].append(A)
    return out


def drop_bound(lv, j, C_before, n_rows):
    """what tr Sigma - tr Sigma+ over the first n_rows (Na or 3) diagonal entries of an actual fp64 correction (the numpy
    model of correct_sparse or the device's) may differ from the long-double closed form by, beyond lv's own bound.  Each
    diagonal entry of Sigma+ is Sigma_ii - sum_q K_iq T_qi with K = U A (2 products a term, rounded) and T from 5 products:
    at most gamma_16 (|Sigma_ii| + (|U| |A| |U|^T)_ii) each, the entries then summed in long double by the test; the
    inverse's own error is in lv's bound already."""
    A = np.abs(lv["A"][j])
    Ga = lv["Pabs"][j] if n_rows == 3 else lv["Gabs"][j]
    diag = np.abs(np.diag(np.asarray(C_before, dtype=LD)))[:n_rows].sum()
    quad = A[0, 0] * Ga[0] + (A[0, 1] + A[1, 0]) * Ga[1] + A[1, 1] * Ga[2]
    return LD(gamma(16)) * (diag + quad)


# ---- the families -------------------------------------------------------------------------------------------------------------

S_TARGETS = (((4, 2), (2, 2)), ((2, 0), (0, 8)), ((1, 1), (1, 2)), ((2, 4), (4, 4)))   # eliminations exact in binary64


def full_tile_cases(tile_rows):
    """(n_lm, spare) with Na = 3 + 2 n_lm + spare exactly one and two tile_rows: a last row tile that is exactly full.  Na is
    odd without spare states behind the last landmark, so an even tile_rows is reached with one of them"""
    return [((rows - 3) // 2, (rows - 3) % 2) for rows in (tile_rows, 2 * tile_rows)]


def integer_family(n_lm, seed=0, spare=0):
    """-> C (symmetric, small integers), Hc (integers), R (integers): the landmark's own diagonal block is chosen so that
    S is one of S_TARGETS exactly -- power-of-two pivots, with and without a row exchange and with a tie -- so the whole
    call is exact in binary64 (exact_value proves it).  spare: states behind the last landmark, live and coupled like the rest"""
    rng = np.random.default_rng([n_lm, seed, 11] + ([spare] if spare else []))
    Na = 3 + 2 * n_lm + spare
    C = rng.integers(-3, 4, size=(Na, Na))
    C = np.triu(C) + np.triu(C, 1).T
    Hc = np.zeros((n_lm, 2, 5), dtype=np.int64)
    Hc[:, :, :3] = rng.integers(-2, 3, size=(n_lm, 2, 3))
    Hc[:, 0, 3] = Hc[:, 1, 4] = 1
    R = np.array([[2, 1], [1, 3]])
    for i in range(n_lm):
        c = lm_cols(i)
        C[np.ix_(c[3:], c[3:])] = 0
        rest = Hc[i] @ C[np.ix_(c, c)] @ Hc[i].T
        C[np.ix_(c[3:], c[3:])] = np.array(S_TARGETS[i % len(S_TARGETS)]) - R - rest
    assert (C == C.T).all()
    return C.astype(np.float64), Hc.astype(np.float64), R.astype(np.float64)


def float_family(n_lm, seed=0, kind="wide", spare=0):
    """-> C = A A^T + D symmetrised in bits, Hc, R.  'wide': Jacobians of order one; 'slam': the reference's shape (a unit
    bearing row over the range, entries down to 1 / d^2).  spare: states behind the last landmark"""
    rng = np.random.default_rng([n_lm, seed, 23, len(kind)] + ([spare] if spare else []))
    Na = 3 + 2 * n_lm + spare
    A = rng.normal(size=(Na, 6))
    C = A @ A.T + np.diag(rng.uniform(0.5, 2.0, size=Na))
    C = 0.5 * (C + C.T)
    assert same_bits(C, C.T)
    if kind == "wide":
        Hc = rng.normal(size=(n_lm, 2, 5))
    else:
        dx, dy = rng.uniform(-9, 9, size=n_lm), rng.uniform(1, 9, size=n_lm)
        d = dx * dx + dy * dy
        q = np.sqrt(d)
        Hc = np.stack([np.stack([0 * q, -dx / q, -dy / q, dx / q, dy / q], 1),
                       np.stack([-1 + 0 * q, dy / d, -dx / d, -dy / d, dx / d], 1)], 1)
    return C, np.ascontiguousarray(Hc), np.eye(2) * 0.01


FLOAT_KINDS = ("wide", "slam")


def symmetric_map(n_lm, seed=0):
    """a surveyed map for the model tests: a state with landmarks a few metres out and a coupled symmetric covariance"""
    rng = np.random.default_rng([n_lm, seed, 31])
    C = float_family(n_lm, seed, "wide")[0] * 0.01
    x = np.concatenate([[0.3, 0.5, -0.2], rng.uniform(-8, 8, size=2 * n_lm)])
    return C, x
