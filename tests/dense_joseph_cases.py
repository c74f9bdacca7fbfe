"""ekf_dense64_correct_sparse_joseph as include/ekfslam.h defines it: an op-by-op float64 numpy model built on the model of
the sparse calls (dense_sparse_cases: T = H Sigma, U = Sigma H^T, S = T H^T + R and its inverse on the embedded H), the
long-double Joseph expression it is judged against, the tile count, and the families of cases.
  integer_case    the construction of the sparse tests: small-integer Sigma (unsymmetric), Hc, nu and R = D - H Sigma H^T with
                  D = diag(2^k), so S = D exactly; S^-1, G, K (for weights that are multiples of 1/4), D = U - K S and every
                  product of the update are dyadic rationals far inside 53 bits: ANY order of summation gives the same bits.
                  With w in {0, 1} the residual D is exactly 0 on the active rows and U on the considered ones.
  slam_case       dense_factor_cases.slam_like (symmetric positive definite) with a random Hc and a positive definite R
  weights(...)    the weight vectors: None, random in (0, 1], quarters, and zeros in one contiguous range, scattered singly,
                  or covering whole tiles
  ILL             the committed ill-conditioned family (see its comment)"""
import numpy as np

import dense_factor_cases as fc
import dense_sparse_cases as sp

JOSEPH_MAX_M = 32      # EKF_DENSE64_JOSEPH_MAX_M
LM_JOSEPH = 8          # EKF_DENSE64_LM_JOSEPH
TOL = 1e-12            # against the long-double expression, relative to sqrt(Sigma_ii Sigma_jj)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


# ---- the model ------------------------------------------------------------------------------------------------------------

def panels(Sigma, cols, Hc, R):
    """T [m][Na], U [Na][m], S, S^-1: the expressions of sp.np_correct on the embedded H, spelled on the listed rows and
    columns alone as the sparse calls gather them (an entry of Sigma outside them -- a planted NaN -- is never touched)"""
    cols = np.asarray(cols)
    T, U = Hc @ Sigma[cols, :], Sigma[:, cols] @ Hc.T
    S = T[:, cols] @ Hc.T + R
    return T, U, S, np.linalg.inv(S)


def gain(U, Si, w):
    """K[i][k] = +0.0 where w_i == 0, else w_i * G[i][k] with G = U S^-1"""
    G = U @ Si
    if w is None:
        return G
    return np.where((w == 0.0)[:, None], 0.0, w[:, None] * G)


def residual(U, K, S):
    """D = U - K S: the accumulator starts at U and takes the terms in ascending l"""
    D = U.copy()
    for l in range(S.shape[0]):
        D = D - K[:, l:l + 1] * S[l:l + 1, :]
    return D


def np_joseph(state, Sigma, cols, Hc, R, nu=None, w=None, Na=None):
    """the definition on the live corner [:Na, :Na] of Sigma (N x N) -> state', Sigma', nis (None without nu).  The K T
    terms are folded first, then the D K^T terms; an entry whose row and column are both considered keeps its bits, as does
    a considered state and everything at an index >= Na"""
    N = Sigma.shape[0]
    Na = N if Na is None else Na
    C = Sigma[:Na, :Na]
    wl = None if w is None else np.asarray(w, dtype=np.float64)[:Na]
    T, U, S, Si = panels(C, cols, Hc, R)
    K = gain(U, Si, wl)
    D = residual(U, K, S)
    on = np.ones(Na, dtype=bool) if wl is None else wl != 0.0
    acc = C.copy()
    with np.errstate(invalid="ignore"):   # (a NaN planted in a considered entry goes through the arithmetic and is dropped)
        for k in range(K.shape[1]):
            acc = acc - K[:, k:k + 1] * T[k:k + 1, :]
        for k in range(K.shape[1]):
            acc = acc - D[:, k:k + 1] * K[:, k:k + 1].T
    held = ~on[:, None] & ~on[None, :]
    out = Sigma.copy()
    out[:Na, :Na] = np.where(held, C, acc)
    x = np.array(state, dtype=np.float64)
    nis = None
    if nu is not None:
        x[:Na] = np.where(on, x[:Na] + K @ nu, x[:Na])
        nis = float(nu @ Si @ nu)
    return x, out, nis


def np_short_form(Sigma, cols, Hc, R, w=None):
    """Sigma - K T with the SAME (weighted) gain: what a route to the short form would store"""
    T, U, S, Si = panels(Sigma, cols, Hc, R)
    return Sigma - gain(U, Si, None if w is None else np.asarray(w, dtype=np.float64)) @ T


def joseph_longdouble(Sigma, cols, Hc, R, w=None):
    """(I - K H) Sigma (I - K H)^T + K R K^T in numpy.longdouble for the model's K (the expression holds for any gain, so
    the rounding of K itself is not an error of the result) -> float64"""
    N = Sigma.shape[0]
    _, U, _, Si = panels(Sigma, cols, Hc, R)
    K = gain(U, Si, None if w is None else np.asarray(w, dtype=np.float64)).astype(np.longdouble)
    H = sp.embed(cols, Hc, N).astype(np.longdouble)
    A = np.eye(N, dtype=np.longdouble) - K @ H
    return A @ Sigma.astype(np.longdouble) @ A.T + K @ np.asarray(R, dtype=np.longdouble) @ K.T


def rel_cov_error(got, want, Sigma):
    """max |got - want| / sqrt(Sigma_ii Sigma_jj), the difference in long double"""
    d = np.sqrt(np.abs(np.diagonal(Sigma)))
    diff = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(want, dtype=np.longdouble))
    return float(np.max(diff / (d[:, None] * d[None, :])))


def tiles_skipped(Na, w, tile_rows, tile_cols):
    """(row groups without a w != 0) * (column groups without one), groups aligned at 0; 0 for w None"""
    if w is None:
        return 0
    on = np.asarray(w)[:Na] != 0.0
    idle = lambda side: sum(1 for i0 in range(0, Na, side) if not on[i0:i0 + side].any())
    return idle(tile_rows) * idle(tile_cols)


# ---- the families ---------------------------------------------------------------------------------------------------------

SIZES = [5, 127, 128, 129, 300]
MS = [1, 2, 3, 32]
SS = [1, 5, 64]


def shapes(Na):
    """(m, s, order) for a live dimension: every m and s that fit, ascending and permuted lists"""
    out = []
    for m in MS:
        for s in SS:
            if m <= Na and s <= Na:
                out.append((m, s, "asc" if (m + s) % 2 else "scattered"))
    return out


def integer_case(N, m, s, order, seed, Na=None, pool=None):
    """-> dict(Sigma, x, cols, Hc, R, nu) on the live corner Na of an N x N handle (the tail is the caller's to poison);
    pool: the listed columns are drawn from [0, pool)"""
    Na = N if Na is None else Na
    rng = np.random.default_rng(seed)
    Sigma = np.zeros((N, N))
    Sigma[:Na, :Na] = rng.integers(-3, 4, size=(Na, Na))
    x = np.zeros(N)
    x[:Na] = rng.integers(-9, 10, size=Na)
    cols = sp.index_list(Na if pool is None else pool, s, order, rng)
    Hc = rng.integers(-2, 3, size=(m, s)).astype(np.float64)
    nu = rng.integers(-4, 5, size=m).astype(np.float64)
    R = np.diag(2.0 ** rng.integers(1, 5, size=m)) - Hc @ Sigma[np.ix_(cols, cols)] @ Hc.T
    return dict(Sigma=Sigma, x=x, cols=cols, Hc=Hc, R=R, nu=nu)


def slam_case(N, m, s, order, seed, Na=None, pool=None):
    Na = N if Na is None else Na
    rng = np.random.default_rng(seed)
    Sigma = np.zeros((N, N))
    Sigma[:Na, :Na] = fc.slam_like(Na, seed)
    x = np.zeros(N)
    x[:Na] = rng.uniform(-2.0, 2.0, size=Na)
    B = rng.standard_normal((m, m))
    return dict(Sigma=Sigma, x=x, cols=sp.index_list(Na if pool is None else pool, s, order, rng), Hc=rng.standard_normal((m, s)),
                R=B @ B.T / m + 0.01 * np.eye(m), nu=0.1 * rng.standard_normal(m))


WEIGHT_KINDS = ("random", "quarters", "range", "scattered", "tiles")


def active_prefix(kind, Na, tile_cols=128):
    """the states below this index are active in weights(kind, ...) unless a zero is scattered there; Na for the other kinds"""
    return (tile_cols if Na > tile_cols else (Na + 1) // 2) if kind == "tiles" else Na


def weights(kind, N, Na, seed, tile_cols=128):
    """N weights (those at indices >= Na are junk the call must ignore).  random: (0, 1]; quarters: {1/4, 1/2, 3/4, 1};
    range: 0 on one contiguous range that starts and ends inside tiles; scattered: single zeros; tiles: 0 from the first
    multiple of the tile width on (whole tiles considered where Na reaches that far, else the upper half)"""
    rng = np.random.default_rng(seed)
    w = np.ones(N)
    if kind == "random":
        w[:Na] = 1.0 - rng.random(Na)
    elif kind == "quarters":
        w[:Na] = rng.integers(1, 5, size=Na) / 4.0
    elif kind == "range":
        w[Na // 3:max(Na // 3 + 1, (2 * Na) // 3)] = 0.0
    elif kind == "scattered":
        w[rng.choice(Na, size=max(1, Na // 7), replace=False)] = 0.0
    elif kind == "tiles":
        w[active_prefix(kind, Na, tile_cols):Na] = 0.0
    else:
        raise ValueError(kind)
    w[Na:] = np.nan
    return w


# ---- the committed ill-conditioned family ---------------------------------------------------------------------------------
# Na = 13 (a pose and five landmarks), m = 2, s = 5 (the pose and landmark 2), prior variance 1e12 on that landmark,
# R = 1e-6 I.  The gain K = U S^-1 carries a relative rounding error of about cond(S) * 2^-53.  The short form stores
# Sigma - K T, where that error enters at FIRST order, times T ~ 1e12; the Joseph form is a covariance for any gain, so the
# same error enters at second order and what is left is the rounding of the accumulation itself, ~ 2^-53 * 1e12 ~ 1e-4.
# The search (tests/test_dense64_joseph_host.py documents and re-runs the acceptance rule) went over seeds and over the scales
# of the rows of Hc until, for the model AND for 32 copies of it whose gain is perturbed by one ulp per entry at random (what
# another order of summation in G = U S^-1 may do) and whose result is perturbed by up to two ulp of the entry of Sigma the
# accumulator started from (what another association of the 2 m terms may do), the Cholesky model of dense_factor_cases stops on the short form's result
# and completes on the Joseph model's, each with a pivot margin of at least 1e3 ulp of the pivot.
ILL = dict(Na=13, m=2, s=5, landmark=2, prior=1e12, r=1e-6, seed=12, row_scale=(1e-4, 1e-3))


def ill_case(p=None):
    """-> dict(Sigma, x, cols, Hc, R, nu) of the family's parameters"""
    p = ILL if p is None else p
    Na, l = p["Na"], p["landmark"]
    rng = np.random.default_rng(p["seed"])
    B = rng.standard_normal((Na, Na))
    Sigma = B @ B.T / Na + 0.5 * np.eye(Na)
    a = 3 + 2 * l
    c = Sigma[:, a:a + 2].copy() * np.sqrt(p["prior"]) * 0.5        # cross-covariances at half the Cauchy-Schwarz scale
    Sigma[:, a:a + 2], Sigma[a:a + 2, :] = c, c.T
    Sigma[a:a + 2, a:a + 2] = p["prior"] * np.eye(2)
    Sigma = np.tril(Sigma) + np.tril(Sigma, -1).T
    cols = sp.slam_cols(l)
    Hc = rng.standard_normal((p["m"], p["s"])) * np.asarray(p["row_scale"])[:, None]
    return dict(Sigma=Sigma, x=rng.uniform(-1.0, 1.0, size=Na), cols=cols, Hc=Hc, R=p["r"] * np.eye(p["m"]),
                nu=np.array([0.01, -0.02]))


def ulp(v):
    return float(np.spacing(abs(float(v))))


def ill_margins(case, n_perturbed=32, seed=99):
    """-> (short: [(ok, fail_pivot / ulp)], joseph: [(ok, min_pivot / ulp)]) for the model and its perturbed copies; the
    ulp is that of the diagonal entry the pivot was subtracted from, the scale at which that subtraction rounds"""
    C, cols, Hc, R = case["Sigma"], case["cols"], case["Hc"], case["R"]
    T, U, S, Si = panels(C, cols, Hc, R)
    K0 = gain(U, Si, None)
    rng = np.random.default_rng(seed)
    short, jos = [], []
    for i in range(1 + n_perturbed):
        K = K0 if i == 0 else K0 + rng.integers(-1, 2, size=K0.shape) * np.spacing(np.abs(K0))
        # another association of the 2 m terms rounds at the scale of the accumulator's start: up to two ulp of it
        noise = 0.0 if i == 0 else rng.integers(-2, 3, size=C.shape) * np.spacing(np.abs(C))
        A = C - K @ T + noise
        rep, _ = fc.np_factor(A)
        short.append((rep["ok"], rep["fail_pivot"] / ulp(A[rep["fail_index"], rep["fail_index"]]) if not rep["ok"] else 0.0))
        D = residual(U, K, S)
        J = A.copy()
        for k in range(K.shape[1]):
            J = J - D[:, k:k + 1] * K[:, k:k + 1].T
        rep, _ = fc.np_factor(J)
        jos.append((rep["ok"], rep["min_pivot"] / ulp(J[rep["min_pivot_i"], rep["min_pivot_i"]]) if rep["ok"] else 0.0))
    return short, jos
