"""Shared by tests/test_gpu_dense64_pairs.py and tests/test_dense64_pairs_host.py: the operands that define the score of a
landmark pair (ekf_dense64_score_landmark_pairs, include/ekfslam.h), a float64 op-by-op numpy model of that score (the
documented order of the sums, then the m = 2 elimination of dense_invert_cases), the model of the whole scan and of the
merge (correction, then the deletion semantics of the removal recipe), and the data families of the tests."""
import itertools
import math

import numpy as np

import dense_invert_cases as di

HC = np.array([[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, -1.0]])
R_MERGES = (0.0, 0.5, 4.0)


def pair_operands(state, a, b, r_merge):
    """-> cols [4], Hc [2][4], R [2][2], nu [2] of the pair (a, b) as given (the definition takes a < b)"""
    cols = np.array([3 + 2 * a, 4 + 2 * a, 3 + 2 * b, 4 + 2 * b], dtype=np.int32)
    nu = np.array([state[cols[0]] - state[cols[2]], state[cols[1]] - state[cols[3]]])
    return cols, HC.copy(), np.eye(2) * r_merge, nu


def merge_operands(state, a, b, r_merge):
    """the operands ekf_dense64_merge_landmarks corrects with: the pair's for (lo, hi), the innovation that of the reading
    0 of x_lo - x_hi, which is the exact negative of the score's nu"""
    cols, Hc, R, nu = pair_operands(state, min(a, b), max(a, b), r_merge)
    return cols, Hc, R, np.array([state[cols[2]] - state[cols[0]], state[cols[3]] - state[cols[1]]])


def all_pairs(n_lm):
    return list(itertools.combinations(range(n_lm), 2))


def stacked_operands(state, pairs, r_merge):
    """the operands of one score_sparse() call over `pairs` -> cols (J, 4), Hc (J, 2, 4), R (2, 2), nu (J, 2)"""
    ops = [pair_operands(state, a, b, r_merge) for a, b in pairs]
    return (np.stack([o[0] for o in ops]), np.stack([o[1] for o in ops]), np.eye(2) * r_merge,
            np.stack([o[3] for o in ops]))


def model_S(Sigma, cols, Hc, R):
    """S in the documented order, one float64 operation at a time: T'[a][j] = sum_k Hc[a][k] G[k][j] from +0 in ascending
    k, S[a][b] = (sum_k T'[a][k] Hc[b][k]) + R[a][b].  Every Hc entry is 0 or +-1, so each product is exact and a fused
    multiply-add is the plain addition written here."""
    G = Sigma[np.ix_(cols, cols)].astype(np.float64)
    m, s = Hc.shape
    with np.errstate(all="ignore"):
        T = np.zeros((m, s))
        for a in range(m):
            for j in range(s):
                acc = np.float64(0.0)
                for k in range(s):
                    acc = acc + np.float64(Hc[a, k]) * G[k, j]
                T[a, j] = acc
        S = np.zeros((m, m))
        for a in range(m):
            for b in range(m):
                acc = np.float64(0.0)
                for k in range(s):
                    acc = acc + T[a, k] * np.float64(Hc[b, k])
                S[a, b] = acc + R[a, b]
    return S


def model_score(Sigma, state, a, b, r_merge, number=np.float64):
    """-> (d2 or NaN, flag, S) of the pair in the order given; number: the type the elimination runs in"""
    cols, Hc, R, nu = pair_operands(state, a, b, r_merge)
    S = model_S(Sigma, cols, Hc, R)
    e = di.eliminate(S, nu, number=number)
    if e["verdict"]:
        return float("nan"), 1, S
    return e["nis"], 0, S


def better(d, i, bd, bi):
    """the argmin's order: smaller score, then lower index; a NaN never wins; bi < 0: nothing yet"""
    return d == d and (bi < 0 or d < bd or (d == bd and i < bi))


def fold(n_lm, pairs, scores, flags, gate):
    """(nearest, d2, n_below, n_flagged) from the scores of `pairs` (a < b): what the scan returns"""
    nearest, d2 = np.full(n_lm, -1, dtype=np.int32), np.full(n_lm, np.inf)
    for (a, b), d, f in zip(pairs, scores, flags):
        if f:
            continue
        for me, other in ((a, b), (b, a)):
            if better(d, other, d2[me], nearest[me]):
                d2[me], nearest[me] = d, other
    ok = np.asarray(flags) == 0
    with np.errstate(invalid="ignore"):
        below = int(np.count_nonzero(ok & (np.asarray(scores, dtype=np.float64) < gate)))
    return nearest, d2, below, int(np.count_nonzero(~ok))


def model_scan(Sigma, state, n_lm, r_merge, gate):
    pairs = all_pairs(n_lm)
    out = [model_score(Sigma, state, a, b, r_merge)[:2] for a, b in pairs]
    return fold(n_lm, pairs, [o[0] for o in out], [o[1] for o in out], gate)


def np_merge(state, Sigma, known, a, b, r_merge, sigma0=100.0):
    """the merge in plain numpy on the first 3 + 2 known states: the correction x_lo = x_hi with noise r_merge I, then hi
    deleted: the last landmark takes its slot, the last slot goes back to the prior.  -> state, Sigma, known, moved_from, d2"""
    lo, hi, last = min(a, b), max(a, b), known - 1
    state, Sigma = state.copy(), Sigma.copy()
    P = 3 + 2 * known
    cols, Hc, R, nu = pair_operands(state, lo, hi, r_merge)
    H = np.zeros((2, P))
    H[:, cols] = Hc
    Sg = Sigma[:P, :P]
    S = H @ Sg @ H.T + R
    K = Sg @ H.T @ np.linalg.inv(S)
    d2 = float(nu @ np.linalg.inv(S) @ nu)
    state[:P] = state[:P] + K @ (-nu)   # the innovation of the reading 0 of x_lo - x_hi is 0 - (x_lo - x_hi)
    Sigma[:P, :P] = Sg - K @ H @ Sg
    bh, bl = slice(3 + 2 * hi, 5 + 2 * hi), slice(3 + 2 * last, 5 + 2 * last)
    if hi != last:
        perm = np.arange(len(state))
        perm[bh], perm[bl] = np.arange(bl.start, bl.stop), np.arange(bh.start, bh.stop)
        state, Sigma = state[perm], Sigma[np.ix_(perm, perm)]
    Sigma[bl, :] = 0.0
    Sigma[:, bl] = 0.0
    Sigma[bl, bl] = sigma0 * np.eye(2)
    return state, Sigma, known - 1, (last if hi != last else -1), d2


# ---- the data families ---------------------------------------------------------------------------------------------------

def integer_family(n_lm, N, seed):
    """Sigma = small-integer A A^T + k I with an ASYMMETRIC integer perturbation (Sigma_ab != Sigma_ba^T), integer states;
    outside the corner of the n_lm landmarks the matrix is filled as well (a tail must not be read)"""
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, size=(N, 4)).astype(np.float64)
    Sigma = A @ A.T + 7.0 * np.eye(N) + rng.integers(-2, 3, size=(N, N)).astype(np.float64)
    state = rng.integers(-9, 10, size=N).astype(np.float64)
    return state, Sigma


def random_family(n_lm, N, seed, dup_every=5):
    """Sigma = A A^T + I with planted near-duplicates: every dup_every-th landmark j gets a partner i = j - 1 with
    x_j = x_i + eps and strongly correlated rows"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(N, N)) / math.sqrt(N)
    state = np.concatenate([rng.normal(size=3), rng.uniform(-20.0, 20.0, size=N - 3)])
    for j in range(1, n_lm, dup_every):
        i = j - 1
        for c in range(2):
            A[3 + 2 * j + c] = A[3 + 2 * i + c] + 0.05 * rng.normal(size=N) / math.sqrt(N)
            state[3 + 2 * j + c] = state[3 + 2 * i + c] + 0.01 * rng.normal()
    return state, A @ A.T + np.eye(N)


def degenerate_family(n_lm, N, seed):
    """the random family with, where n_lm allows: landmark 1 an exact copy of landmark 0 (singular S at r_merge = 0: flagged),
    a NaN in the block of landmark 2, and landmarks 4 and 5 at exactly the same d2 from landmark 3 (the lowest index wins).
    -> state, Sigma, what (the names of the cases planted)"""
    state, Sigma = random_family(n_lm, N, seed, dup_every=10 ** 9)
    what = []
    if n_lm >= 2:
        r0, r1 = slice(3, 5), slice(5, 7)
        Sigma[r1, :] = Sigma[r0, :]
        Sigma[:, r1] = Sigma[:, r0]
        state[r1] = state[r0]
        what.append("copy")
    if n_lm >= 3:
        Sigma[7, 8] = np.nan
        what.append("nan")
    if n_lm >= 6:
        # 3, 4, 5 decoupled from everything, 4 and 5 identical in law and mirrored about 3: equal d2, bit for bit
        blk = slice(9, 15)
        Sigma[blk, :] = 0.0
        Sigma[:, blk] = 0.0
        Sigma[blk, blk] = np.diag([2.0, 3.0, 1.5, 2.5, 1.5, 2.5])
        state[9:11] = [100.0, -200.0]   # (far from the others, which lie in [-20, 20])
        state[11:13] = [100.5, -199.25]
        state[13:15] = [99.5, -200.75]
        what.append("tie")
    return state, Sigma, what
