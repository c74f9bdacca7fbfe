"""Shared by tests/test_gpu_dense64_invert.py and tests/test_dense64_invert_host.py: operands that hand an arbitrary m x m
matrix R to the dense fp64 handle's inversion (gj_invert / gj_quadratic, ekf_dense64_invert.hpp) and bring its inverse back
bit for bit, a restatement of that elimination over a generic number type (fractions.Fraction, numpy.float64,
numpy.longdouble), the matrix families on which every step of it is exact in fp64, and the families of prescribed
conditioning on which its accuracy is measured.

The door.  For N >= 2 m take H = [I_m | 0 | 0] and Sigma = [[0, I_m, 0], [I_m, 0, 0], [0, 0, 0]].  Sigma is never
symmetrised and S is summed as (H Sigma) H^T + R, so T = H Sigma = [0 | I_m | 0], T H^T = 0 and S = R exactly;
U = Sigma H^T = [0; I_m; 0], K = [0; S^-1; 0].  After correct(H, R, nu) on a zero state Sigma'[m:2m, m:2m] = -S^-1 (every
product has one nonzero term, 0 - x is exact), state'[m:2m] = S^-1 nu as the device summed it, the rest of Sigma and of the
state is unchanged and nis is gj_quadratic's value.  score() with the same H returns S_out = R and the quadratic form of the
same inverse."""
from fractions import Fraction

import numpy as np

U52 = 2.0 ** -52   # the unit the accuracy bound is stated in: kappa_2(R) * 2^-52
SIZES = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 63, 64)   # 2 m crosses the wave width between 31 and 33
BIG_N = 300


# ---- the door ----------------------------------------------------------------------------------------------------------

def door(N, m):
    """-> H (m x N), Sigma (N x N) with S = R exactly for any R"""
    assert N >= 2 * m
    H = np.zeros((m, N))
    H[:, :m] = np.eye(m)
    Sigma = np.zeros((N, N))
    Sigma[:m, m:2 * m] = np.eye(m)
    Sigma[m:2 * m, :m] = np.eye(m)
    return H, Sigma


def through_the_door(Sigma0, Sigma1, state1, m):
    """-> X = -Sigma'[m:2m, m:2m], w = state'[m:2m] after correct() on a zero state, and whether everything else is as it
    was (the rest of Sigma the same bits, the rest of the state zero)"""
    blk = slice(m, 2 * m)
    a, b = Sigma0.copy(), Sigma1.copy()
    a[blk, blk] = 0.0
    b[blk, blk] = 0.0
    rest = state1.copy()
    rest[blk] = 0.0
    return -Sigma1[blk, blk], state1[blk].copy(), bool(np.array_equal(a, b) and not rest.any())


# ---- the elimination over a generic number type ------------------------------------------------------------------------

def _is_double(v):
    try:
        return Fraction(float(v)) == v
    except OverflowError:
        return False


def eliminate(R, nu=None, number=np.float64, tie_highest=False):
    """Gauss-Jordan with partial pivoting on [R | I] as the header of ekf_dense64_invert.hpp describes it, then the
    quadratic form.  For p = 0 .. m - 1: (1) the pivot is the entry of column p at or below the diagonal with the largest
    magnitude, the lowest row on a tie; a zero or non-finite one ends the run with verdict 1; (2) that row and row p change
    places, and the row now at p is divided by the pivot; (3) every other row r loses (its entry in column p) times the
    scaled pivot row, over all 2 m columns.  An inverse that is not finite is verdict 1 too.  Then w = X nu row by row and
    nis = nu . w, both summed in ascending order.

    number: fractions.Fraction (exact; rows with a zero multiplier are left alone, which changes no value),
    numpy.float64 or numpy.longdouble.  tie_highest picks the HIGHEST row on a tie (what the device must not do).
    -> dict: X (None on verdict 1), verdict, step (the p at which a pivot failed, m for an overflowed inverse, else None),
    pivots [(p, pivot row)], swaps, big (largest magnitude produced), inexact (Fraction only: how many produced values,
    products included, are not doubles), w, nis."""
    exact = number is Fraction
    m = len(R)
    out = dict(X=None, verdict=1, step=None, pivots=[], swaps=0, big=0.0, inexact=0, w=None, nis=None)
    if exact:
        M = np.empty((m, 2 * m), dtype=object)
        for r in range(m):
            for c in range(m):
                M[r, c] = Fraction(float(R[r][c]))
                M[r, m + c] = Fraction(int(r == c))
    else:
        M = np.zeros((m, 2 * m), dtype=number)
        M[:, :m] = np.asarray(R, dtype=number)
        M[:, m:] = np.eye(m, dtype=number)
        if not np.isfinite(M).all():
            out["step"] = 0
            return out

    def seen(values):
        for v in values:
            out["big"] = max(out["big"], abs(v))
            if exact and not _is_double(v):
                out["inexact"] += 1

    with np.errstate(all="ignore"):
        for p in range(m):
            best, pr, finite = -1, p, True
            for r in range(p, m):
                x = M[r, p]
                finite = finite and (exact or bool(np.isfinite(x)))
                a = abs(x)
                if a > best or (tie_highest and a == best):
                    best, pr = a, r
            if not finite or not best > 0:
                out["step"] = p
                return out
            out["pivots"].append((p, pr))
            out["swaps"] += pr != p
            pv = M[pr, p]
            row = M[pr] / pv
            M[pr] = M[p]
            M[p] = row
            f = M[:, p].copy()
            f[p] = 0 * pv
            if exact:
                rows = [r for r in range(m) if f[r] != 0]
                cols = [c for c in range(2 * m) if row[c] != 0]
                seen(row)
                for r in rows:
                    for c in cols:
                        prod = f[r] * row[c]
                        M[r, c] = M[r, c] - prod
                        seen((prod, M[r, c]))
            else:
                new = M - f[:, None] * row[None, :]
                new[p] = row
                M = new
                big = np.abs(M).max()
                out["big"] = max(out["big"], float(big) if np.isfinite(big) else float("inf"))
        X = M[:, m:]
        if not exact and not np.isfinite(X).all():
            out["step"] = m
            return out
        out["X"], out["verdict"] = X, 0
        if nu is not None:
            v = [Fraction(float(x)) for x in nu] if exact else np.asarray(nu, dtype=number)
            w = X[:, 0] * v[0]
            for l in range(1, m):
                w = w + X[:, l] * v[l]
            nis = v[0] * w[0]
            for k in range(1, m):
                nis = nis + v[k] * w[k]
            out["w"], out["nis"] = w, nis
    return out


def sums_exact(X, nu):
    """With X and nu exact (Fractions): every term of X nu (per row) and of nu^T X nu is a multiple of one power of two q,
    and the sum of their magnitudes stays below 2^53 q -- then every partial sum in every order, fused or not, is a double,
    and the device's state' and nis are the exact values whatever its order of summation."""
    m = len(nu)
    v = [Fraction(float(x)) for x in nu]

    def ok(terms):
        terms = [abs(t) for t in terms if t != 0]
        if not terms:
            return True
        if any(t.denominator & (t.denominator - 1) for t in terms):
            return False
        # dyadic terms: q is the largest power of two that divides every one of them
        val = min((t.numerator & -t.numerator).bit_length() - t.denominator.bit_length() for t in terms)
        q = Fraction(2) ** val
        return sum(terms) / q < 2 ** 53

    rows = all(ok([X[t, l] * v[l] for l in range(m)]) for t in range(m))
    return rows and ok([v[k] * X[k, l] * v[l] for k in range(m) for l in range(m)])


def as_float(a):
    return np.array([[float(v) for v in r] for r in a]) if np.ndim(a) == 2 else np.array([float(v) for v in a])


# ---- families on which every step is exact -----------------------------------------------------------------------------

def _derangement(m, rng):
    if m == 1:
        return np.array([0])
    while True:
        p = rng.permutation(m)
        if not (p == np.arange(m)).any():
            return p


def signed_perm(m, rng, cyclic=False):
    """P diag(+-2^k): column i has its one entry in row perm[i] != i (cyclic: row i + 1, so the diagonal is zero and the
    matrix is a scaled cyclic shift)"""
    perm = (np.arange(m) + 1) % m if cyclic else _derangement(m, rng)
    A = np.zeros((m, m))
    A[perm, np.arange(m)] = rng.choice([-1.0, 1.0], size=m) * 2.0 ** rng.integers(-3, 4, size=m)
    return A


def nilpotent(m, rng, layout, pow2=False):
    """E with small dyadic entries (k / 8, |k| <= 4; pow2: 0 or +-2^-j, j = 1 .. 3) and E^2 = 0: nonzero only in rows
    < m / 2 and columns >= m / 2 ('upper'), or the transposed layout ('lower'); dense up to m = 17, a few entries per row
    above (the exact run stays cheap)"""
    h = m // 2
    E = np.zeros((m, m))
    if pow2:
        blk = rng.choice([-1.0, 0.0, 1.0], size=(h, m - h)) * 2.0 ** -rng.integers(1, 4, size=(h, m - h))
    else:
        blk = rng.integers(-4, 5, size=(h, m - h)) / 8.0
    if m > 17:
        blk *= rng.random(size=blk.shape) < 3.0 / (m - h)
    if layout == "upper":
        E[:h, h:] = blk
    else:
        E[h:, :h] = blk.T
    return E


def perm_nilpotent(m, rng, layout, pow2=False):
    """P (I + E) diag(+-2^k), P a permutation without a fixed point.  The scaling is by COLUMN: column c is +-2^k times
    (e_c + E[:, c]) with |E| <= 1 / 2, so its pivot is the power of two and every quotient is exact.  (With the scaling on
    the rows an entry 3 / 8 * 2^k of E can outgrow the diagonal, and dividing by it is not exact.)"""
    d = rng.choice([-1.0, 1.0], size=m) * 2.0 ** rng.integers(-3, 4, size=m)
    A = (np.eye(m) + nilpotent(m, rng, layout, pow2)) * d[None, :]
    return A[np.argsort(_derangement(m, rng))]


def exact_families(m, seed):
    """-> [(name, R)]: matrices whose whole elimination the Fraction run shows to be exact in fp64"""
    rng = np.random.default_rng(1000 * m + seed)
    fams = [("perm", signed_perm(m, rng)), ("cyclic", signed_perm(m, rng, cyclic=True))]
    if m >= 2:
        for layout in ("upper", "lower"):
            fams.append((f"perm_nilpotent_{layout}", perm_nilpotent(m, rng, layout)))
    return fams


def exact_nu(m, rng):
    nu = rng.integers(-4, 5, size=m).astype(np.float64)
    nu[rng.integers(0, m)] = 3.0
    return nu


TIE_SMALL, TIE_BIG = 2.0 ** -520, 2.0 ** 520


def tie_matrix(m, rows, c0=0):
    """The identity, except that column c0 holds the same magnitude a = 2^-520 in every row of `rows` (rows[0] == c0, the
    diagonal; a second row of a pair carries -a) and each later row of `rows` has B = 2^520 on its own diagonal.  The
    lowest row wins the tie and nothing overflows: the inverse is finite (entries 1 / a, 1 / B, 1) and exact.  Any other
    winner's scaled row holds B / a = 2^1040 = Inf, so the tie rule shows in the verdict and in the bits."""
    assert rows[0] == c0 and all(r > c0 for r in rows[1:]) and max(rows) < m
    A = np.eye(m)
    for r in rows:
        A[r, c0] = TIE_SMALL
    if len(rows) == 2:
        A[rows[1], c0] = -TIE_SMALL
    for r in rows[1:]:
        A[r, r] = TIE_BIG
    return A


def tie_cases(m):
    """-> [(name, R, rows)] for this m"""
    out = []
    if m >= 2:
        out.append(("tie2_first", tie_matrix(m, [0, m - 1]), [0, m - 1]))
    if m >= 3:
        out.append(("tie3_first", tie_matrix(m, [0, 1, m - 1]), [0, 1, m - 1]))
    if m >= 5:
        c0 = m // 2
        out.append(("tie2_mid", tie_matrix(m, [c0, c0 + 1], c0), [c0, c0 + 1]))
        out.append(("tie3_mid", tie_matrix(m, [c0, c0 + 1, m - 1], c0), [c0, c0 + 1, m - 1]))
    return out


def rank_deficient(m, seed, how):
    """An exactly singular R whose first pivots are fine: (I + E) diag(+-2^k) with power-of-two E (every step exact)
    whose last row is replaced by a copy of the row before it ('equal_rows') or by the sum of rows 0 and 1
    ('sum_of_two'), then its rows permuted."""
    assert m >= 3
    rng = np.random.default_rng(77 * m + seed)
    d = rng.choice([-1.0, 1.0], size=m) * 2.0 ** rng.integers(-3, 4, size=m)
    A = (np.eye(m) + nilpotent(m, rng, "upper", pow2=True)) * d[None, :]
    A[m - 1] = A[m - 2] if how == "equal_rows" else A[0] + A[1]
    return A[np.argsort(_derangement(m, rng))]


# ---- families of prescribed conditioning -------------------------------------------------------------------------------

KAPPAS = (1e2, 1e6, 1e10, 1e12)
ACC_SIZES = (2, 5, 16, 17, 33, 64)
ACC_SEEDS = (0, 1, 2)


def svd_matrix(m, kappa, seed, spd):
    """R = U diag(sigma) V^T, orthogonal U, V from seeded QR, sigma log-spaced from 1 to 1 / kappa; spd: V = U"""
    rng = np.random.default_rng([m, seed, int(spd), int(round(np.log10(kappa)))])
    U = np.linalg.qr(rng.normal(size=(m, m)))[0]
    V = U if spd else np.linalg.qr(rng.normal(size=(m, m)))[0]
    sigma = np.logspace(0.0, -np.log10(kappa), m) if m > 1 else np.ones(1)
    return (U * sigma) @ V.T


def graded_matrix(m, seed):
    """diag(10^-a) G diag(10^-b), a and b spread over six decades: small pivots, a harmless condition after scaling"""
    rng = np.random.default_rng([m, seed, 99])
    a, b = rng.uniform(0.0, 6.0, size=m), rng.uniform(0.0, 6.0, size=m)
    return (10.0 ** -a)[:, None] * rng.normal(size=(m, m)) * (10.0 ** -b)[None, :]


def accuracy_cases():
    """-> [(family, m, kappa or None, seed, R)]"""
    out = []
    for m in ACC_SIZES:
        for seed in ACC_SEEDS:
            for kappa in KAPPAS:
                out.append(("general", m, kappa, seed, svd_matrix(m, kappa, seed, False)))
                out.append(("spd", m, kappa, seed, svd_matrix(m, kappa, seed, True)))
            out.append(("graded", m, None, seed, graded_matrix(m, seed)))
    return out


def accuracy_nu(m, seed):
    return np.random.default_rng([m, seed, 7]).normal(size=m)


def truth(R, nu=None):
    """the long-double run of the elimination: 64 significand bits, kappa * 2^-64 is three orders below the bound"""
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is not the x87 extended format here"
    t = eliminate(R, nu, np.longdouble)
    assert t["verdict"] == 0
    return t


def rel_err(X, Xt):
    """max |X - X_true| / max |X_true|, the difference taken in long double"""
    Xt = np.asarray(Xt, dtype=np.longdouble)
    return float(np.abs(np.asarray(X, dtype=np.longdouble) - Xt).max() / np.abs(Xt).max())


def accuracy_bound(R, Xt):
    """max(8 * err_lapack, kappa_2(R) * 2^-52): both terms from the reference side.  -> bound, err_lapack, kappa_2"""
    err_lapack = rel_err(np.linalg.inv(R), Xt)
    kappa2 = float(np.linalg.cond(R, 2))
    return max(8.0 * err_lapack, kappa2 * U52), err_lapack, kappa2


# ---- the verdict -------------------------------------------------------------------------------------------------------

def overflow_one_entry(m):
    """Upper bidiagonal in its first three rows: [[1, -2^600, 0], [0, 1, -2^600], [0, 0, 1]] in the identity.  Every pivot
    is 1; the inverse has 2^600 twice and 2^1200 once -- one entry that overflows."""
    assert m >= 3
    A = np.eye(m)
    A[0, 1] = A[1, 2] = -2.0 ** 600
    return A


def permutation(m, seed):
    A = np.zeros((m, m))
    A[_derangement(m, np.random.default_rng(5 * m + seed)), np.arange(m)] = 1.0
    return A
