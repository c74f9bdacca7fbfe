"""Shared by tests/test_gpu_dense64_swap.py and tests/test_dense64_swap_host.py: the exchange of two blocks of states of the
dense fp64 handle (ekf_dense64_swap_blocks) in numpy -- Sigma <- P Sigma P^T, state <- P state by fancy indexing with the
permutation, the same on a pair of pending panels -- the data whose every entry is unique (so a misplaced copy shows), and the
grid of (N, a, b, r) that walks the edges of the kernel's masking."""
import numpy as np

GRID_N = [4, 67, 128, 131, 203]
GRID_R = [1, 2, 3, 64]
STRIP = 64                                                 # columns (rows) of a panel strip of k_d64_swap


def perm(N, a, b, r):
    """p with p[a + k] = b + k, p[b + k] = a + k and p[i] = i elsewhere: an involution"""
    assert r >= 1 and 0 <= a and 0 <= b and a + r <= N and b + r <= N and abs(a - b) >= r
    p = np.arange(N)
    p[a:a + r] = np.arange(b, b + r)
    p[b:b + r] = np.arange(a, a + r)
    return p


def swap_model(Sigma, x, a, b, r):
    """-> (P Sigma P^T, P x) as copies: new Sigma[i][j] = Sigma[p[i]][p[j]], new x[i] = x[p[i]]; every entry keeps its bits"""
    p = perm(len(x), a, b, r)
    return Sigma[np.ix_(p, p)].copy(), x[p].copy()


def swap_panels(Kt, Tp, a, b, r):
    """the pending panels [rows][N] through the same permutation: every row v becomes P v"""
    p = perm(Kt.shape[1], a, b, r)
    return Kt[:, p].copy(), Tp[:, p].copy()


def explicit_P(N, a, b, r):
    P = np.zeros((N, N))
    P[np.arange(N), perm(N, a, b, r)] = 1.0
    return P


def unique_data(N, seed=0):
    """Sigma[i][j] = i N + j (non-symmetric, every entry unique) and x[i] = -(i + 1), with a sprinkling of -0.0 and of NaNs
    whose payloads are all different"""
    rng = np.random.default_rng(1000 * N + seed)
    S = (np.arange(N)[:, None] * float(N) + np.arange(N)[None, :]).astype(np.float64)
    x = -(np.arange(N, dtype=np.float64) + 1.0)
    k = max(2, N * N // 9)
    at = rng.choice(N * N, size=2 * k, replace=False)
    flat = S.reshape(-1)
    flat[at[:k]] = -0.0
    flat.view(np.uint64)[at[k:]] = np.uint64(0x7FF8000000000000) + (np.uint64(1) + at[k:].astype(np.uint64))
    for i in rng.choice(N, size=max(1, N // 5), replace=False):
        x[i] = -0.0
    xs = rng.choice(N, size=max(1, N // 5), replace=False)
    x.view(np.uint64)[xs] = np.uint64(0xFFF8000000000000) + (np.uint64(5) + xs.astype(np.uint64))
    return S, x


def cases(N):
    """the (a, b, r) with a < b run at dimension N: adjacent blocks, a = 0, b + r = N, a block across a 64-boundary
    (a = 62), both blocks inside one strip and in different strips, N = 2 r (no entry outside A u B)"""
    out = []
    for r in GRID_R:
        if 2 * r > N:
            continue
        c = [(0, r), (0, N - r), (N - 2 * r, N - r)]                     # adjacent at 0; a = 0 and b + r = N; adjacent at N
        if 62 + 2 * r <= N:
            c += [(62, 62 + r), (62, N - r)]                              # across the boundary: adjacent, and apart
        if 5 + 2 * r + 1 <= STRIP <= N:
            c += [(5, 5 + r + 1)]                                         # one strip, a gap of one
        if r == 64 and N >= 131:
            c += [(3, 67)]                                                # both blocks across a boundary
        if N >= 131 and 70 + r <= N - r:
            c += [(1, 70), (70, N - r)]                                   # different strips
        out += [(a, b, r) for a, b in dict.fromkeys(c) if a >= 0 and b - a >= r and b + r <= N]
    return out


def grid():
    return [(N, a, b, r) for N in GRID_N for a, b, r in cases(N)]


def spd(N, rng):
    A = rng.normal(size=(N, N))
    return A @ A.T / N + np.eye(N)
