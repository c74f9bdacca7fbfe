"""Shared by tests/test_gpu_dense64_deferred.py and tests/test_dense64_deferred_host.py: a numpy model of the deferred sparse
correction (Sigma_cur = Sigma_base - sum_q K^T[q] T[q] kept as factors, the gather and the scoring reading through them,
the flush), the integer chains on which the deferred and the eager sequence are the same numbers exactly, and the exact
integer replay that proves a chain stays inside float64."""
from fractions import Fraction

import numpy as np

import dense_sparse_cases as sp

MAX_ROWS = 64                                              # EKF_DENSE64_PENDING_MAX_ROWS
PAIRS = [(1, 1), (2, 5), (16, 16), (17, 5), (2, 64)]       # (m, s) of the chains
ORDERS = ("asc", "desc", "scattered")
CHAIN_N = [1, 5, 63, 64, 65, 200, 403]


class DeferredModel:
    """The handle's deferred calls in numpy: Sigma_base, the state and the pending rows Kt [p][N], Tp [p][N].  Every read
    of Sigma goes x = base; x = x - Kt[q][row] * Tp[q][col] for q ascending (the device's fma, exact on the integer
    chains), then the sparse calls' products."""

    def __init__(self, Sigma, state):
        self.base = np.array(Sigma, dtype=np.float64)
        self.state = np.array(state, dtype=np.float64)
        self.N = len(self.state)
        self.Kt, self.Tp = np.zeros((0, self.N)), np.zeros((0, self.N))

    @property
    def pending(self):
        return len(self.Kt)

    def read(self, rows, cols):
        """Sigma_cur[np.ix_(rows, cols)] through the pending rows"""
        x = self.base[np.ix_(rows, cols)].copy()
        for q in range(self.pending):
            x = x - np.outer(self.Kt[q][rows], self.Tp[q][cols])
        return x

    def gather(self, cols, Hc):
        """-> T [m][N] from s rows, U^T [m][N] from s columns of Sigma_cur"""
        every = np.arange(self.N)
        return Hc @ self.read(cols, every), Hc @ self.read(every, cols).T

    def scores(self, cols, Hc, R, nu=None):
        J, m = Hc.shape[0], Hc.shape[1]
        S, nis = np.empty((J, m, m)), None if nu is None else np.empty(J)
        for j in range(J):
            S[j] = (Hc[j] @ self.read(cols[j], cols[j])) @ Hc[j].T + (R if R.ndim == 2 else R[j])
            if nu is not None:
                nis[j] = float(nu[j] @ np.linalg.inv(S[j]) @ nu[j])
        return S, nis

    def correct_deferred(self, cols, Hc, R, nu):
        if self.pending + len(Hc) > MAX_ROWS:
            self.flush()
        T, Ut = self.gather(cols, Hc)
        Si = np.linalg.inv(T[:, cols] @ Hc.T + R)
        Kt = (Ut.T @ Si).T
        self.state = self.state + Kt.T @ nu
        self.Kt, self.Tp = np.vstack([self.Kt, Kt]), np.vstack([self.Tp, T])
        return float(nu @ Si @ nu)

    def flush(self):
        self.base = self.base - self.Kt.T @ self.Tp
        self.Kt, self.Tp = np.zeros((0, self.N)), np.zeros((0, self.N))

    @property
    def sigma_cur(self):
        return self.base - self.Kt.T @ self.Tp


# ---- integer chains ---------------------------------------------------------------------------------------------------------

def sparse_rows(rng, m, s, nonzero=2):
    """Hc [m][s] with entries in {-1, 0, 1}, at most `nonzero` of them per row and at least one: the growth of a chain is
    quadratic in |Hc Sigma|, so the rows are kept thin"""
    Hc = np.zeros((m, s))
    for a in range(m):
        idx = rng.choice(s, size=min(s, nonzero), replace=False)
        Hc[a, idx] = rng.choice([-1.0, 1.0], size=len(idx))
    return Hc


def exact_candidates(Sigma_cur, J, m, s, order, rng, first=None):
    """the construction of test_gpu_dense64_sparse._exact_candidates against the CURRENT covariance: R_j = D_j - H_j
    Sigma_cur H_j^T with D_j = diag(2^k), so S_j = D_j exactly; candidate 0 has its list in `order` (or is `first`), the others scattered"""
    N = len(Sigma_cur)
    cols = np.stack([sp.index_list(N, s, order if j == 0 else "scattered", rng) for j in range(J)])
    if first is not None:
        cols[0] = first
    Hc = np.stack([sparse_rows(rng, m, s) for _ in range(J)])
    nu = rng.integers(-2, 3, size=(J, m)).astype(np.float64)
    R, D = np.empty((J, m, m)), np.empty((J, m, m))
    for j in range(J):
        D[j] = np.diag(2.0 ** rng.integers(0, 3, size=m))
        R[j] = D[j] - Hc[j] @ Sigma_cur[np.ix_(cols[j], cols[j])] @ Hc[j].T
    return cols, Hc, R, nu, D


def chain_shapes(N, order, length=3):
    fit = [p for p in PAIRS if p[0] <= N and p[1] <= N]
    first = ORDERS.index(order) * 2 + CHAIN_N.index(N) if N in CHAIN_N else 0
    return [fit[(first + i) % len(fit)] for i in range(length)]


def integer_chain(N, order, seed=None, shapes=None, J=3, Sigma0=None, lists=None):
    """Sigma0, x0 in small integers and per step the J candidates built against the covariance the eager numpy sequence
    (sp.np_correct with candidate 0) has reached, with what that sequence gives: S, nis of the candidates BEFORE the step's
    correction, the state and Sigma after it; "after": one more set of candidates against the final covariance.
    lists: the list of candidate 0 per step where the caller chooses it.  -> dict"""
    rng = np.random.default_rng(9000 + 7 * N + ORDERS.index(order) if seed is None else seed)
    Sigma = rng.integers(-1, 2, size=(N, N)).astype(np.float64) if Sigma0 is None else np.array(Sigma0, dtype=np.float64)
    x = rng.integers(-9, 10, size=N).astype(np.float64)
    chain = {"N": N, "Sigma0": Sigma.copy(), "x0": x.copy(), "steps": []}
    shapes = chain_shapes(N, order) if shapes is None else list(shapes)
    for i, (m, s) in enumerate(shapes):
        cols, Hc, R, nu, D = exact_candidates(Sigma, J, m, s, order, rng, None if lists is None else lists[i])
        S, nis = sp.np_scores(Sigma, cols, Hc, R, nu)
        x, Sigma, n0 = sp.np_correct(x, Sigma, cols[0], Hc[0], R[0], nu[0])
        chain["steps"].append({"m": m, "s": s, "cols": cols, "Hc": Hc, "R": R, "nu": nu, "D": D, "S": S, "nis": nis,
                               "nis0": n0, "state": x.copy(), "Sigma": Sigma.copy()})
    m, s = shapes[-1]
    cols, Hc, R, nu, D = exact_candidates(Sigma, J, m, s, order, rng)
    S, nis = sp.np_scores(Sigma, cols, Hc, R, nu)
    chain["after"] = {"m": m, "s": s, "cols": cols, "Hc": Hc, "R": R, "nu": nu, "D": D, "S": S, "nis": nis}
    return chain


def block_sigma(N, size, rng):
    """small integers in diagonal blocks of `size`, zero elsewhere: a correction listed inside one block changes that block
    alone, so a long sequence over distinct blocks does not compound"""
    S = np.zeros((N, N))
    for b in range(0, N - size + 1, size):
        S[b:b + size, b:b + size] = rng.integers(-1, 2, size=(size, size))
    return S


def capacity_chain(N, name):
    """the sequences that fill the 64 pending rows -> chain; `name`:
    pairs  32 x (m = 2) to exactly 64, then m = 1 (flushes first: 1 pending)
    big    17 + 17 + 17 + 13 to exactly 64, then m = 1
    odd    17 + 17 + 17 + 12 = 63, then m = 2 (flushes first: 2 pending)
    full   m = 64 on an empty store, then m = 1"""
    rng = np.random.default_rng(700 + N + len(name))
    size = 2 if name == "pairs" else 5
    ms = {"pairs": [2] * 32 + [1], "big": [17, 17, 17, 13, 1], "odd": [17, 17, 17, 12, 2], "full": [64, 1]}[name]
    lists = [np.arange(size * (i % (N // size)), size * (i % (N // size)) + size, dtype=np.int32) for i in range(len(ms))]
    lists[-1] = lists[0]                                       # the call that overflows goes back to the first block
    return integer_chain(N, "asc", seed=700 + N + len(name), shapes=[(m, size) for m in ms], J=1,
                         Sigma0=block_sigma(N, size, rng), lists=lists)


def _trim(A, e):
    """(int64 array, exponent) with the common factors of two divided out"""
    while e > 0 and not (A & 1).any():
        A, e = A >> 1, e - 1
    return A, e


def exact_replay(chain, limit=2 ** 52):
    """The chain's correction of candidate 0 per step in exact integer arithmetic: every matrix is an int64 array over a
    common power of two.  Before each product the sum of the absolute values of its terms is bounded below `limit`, so every
    partial sum in ANY order (numpy's, the device's fold, the matrix cores' in the flush) is an integer below 2^53 over
    that power of two: exactly representable.  -> per step (state, Sigma) as (int array, exponent) pairs; raises
    AssertionError when a bound is passed (the chain's seed must then be replaced)."""
    S, e = chain["Sigma0"].astype(np.int64), 0
    x, ex = chain["x0"].astype(np.int64), 0
    out = []
    total, finest = np.abs(chain["Sigma0"]), 0      # |Sigma0| + sum |K| |T| in real units; the finest power of two of a term
    for st in chain["steps"]:
        cols, Hc, nu = st["cols"][0], st["Hc"][0].astype(np.int64), st["nu"][0].astype(np.int64)
        k = np.round(np.log2(np.diag(st["D"][0]))).astype(np.int64)
        aS, aH = np.abs(S).astype(np.float64), np.abs(Hc).astype(np.float64)
        assert (aH @ aS[cols, :]).max() < limit and (aS[:, cols] @ aH.T).max() < limit
        T, U = Hc @ S[cols, :], S[:, cols] @ Hc.T                      # exponent e
        assert ((aH @ aS[np.ix_(cols, cols)]) @ aH.T).max() + float(2 ** (e + 2)) < limit      # S - R and R themselves
        kmax = int(k.max())
        K = U * (1 << (kmax - k))[None, :]                             # K = U D^-1 at exponent e + kmax
        eK = e + kmax
        grow = float(2 ** eK)
        assert (np.abs(K).astype(np.float64) @ np.abs(T).astype(np.float64) + aS * grow).max() < limit
        total = total + (np.abs(K).astype(np.float64) @ np.abs(T).astype(np.float64)) / float(2 ** (e + eK))
        finest = max(finest, e + eK)
        assert total.max() * float(2 ** finest) < limit               # a flush of everything so far, in any order
        S, e = _trim(S * (1 << eK) - K @ T, e + eK)                    # Sigma - K T at exponent 2 e + kmax
        up = max(eK, ex)                                               # state + K nu
        assert (np.abs(K).astype(np.float64) @ np.abs(nu) * 2.0 ** (up - eK) + np.abs(x) * 2.0 ** (up - ex)).max() < limit
        x, ex = _trim(x * (1 << (up - ex)) + (K @ nu) * (1 << (up - eK)), up)
        out.append(((x, ex), (S, e)))
    return out


def same_number(value, pair, where):
    """float64 `value`[where] against the exact (int array, exponent) pair, as fractions"""
    A, e = pair
    return all(Fraction(float(value[i])) == Fraction(int(A[i]), 2 ** e) for i in where)
