"""ekf_dense64_extract_map as include/ekfslam.h defines it: the live corner of a source handle (Nb = 3 + 2 b states), or the
part of it that a list keep [k] of distinct landmarks names, copied into a destination handle.  With
iota: 0, 1, 2 -> 0, 1, 2 and 3 + 2 t + c -> 3 + 2 keep[t] + c (c = 0, 1; Nd = 3 + 2 k):
Sigma_dst[i][j] = Sigma_src[iota(i)][iota(j)], x_dst[i] = x_src[iota(i)], bits kept; a pending row goes through the same
gather, K_dst[q][i] = K_src[q][iota(i)], zero from Nd on.  Here: that model in numpy, the families of keep lists, a source
corner that is NOT SYMMETRIC and holds payload NaNs and -0.0 (so a transposed gather, an arithmetic step or a canonicalised
NaN shows), and the sizes the GPU test runs."""
import numpy as np

from dense_frame_cases import odd_near, same_bits   # noqa: F401
from dense_join_cases import sizes as join_sizes


def sizes(tr, tc):
    """the source's live dimension: the distinct odd numbers nearest {3, 5, 7, T - 1, T, T + 1, 2 T + 1, 3 T + 2}, T in {tr, tc}"""
    return join_sizes(tr, tc)


# ---- the model --------------------------------------------------------------------------------------------------------------

def as_list(keep, b):
    """None is the identity list of all b landmarks"""
    return np.arange(b, dtype=np.int64) if keep is None else np.asarray(keep, dtype=np.int64).reshape(-1)


def iota(keep):
    """the source's index of every state of the destination: (3 + 2 k,)"""
    keep = np.asarray(keep, dtype=np.int64).reshape(-1)
    return np.concatenate([np.arange(3), (3 + 2 * keep[:, None] + np.arange(2)[None, :]).reshape(-1)]).astype(np.int64)


def expected_corner(S, keep):
    io = iota(keep)
    return np.asarray(S)[np.ix_(io, io)]


def transposed_corner(S, keep):
    """what a kernel that walks the source by columns would give: Sigma_src[iota(j)][iota(i)]"""
    return expected_corner(np.asarray(S).T, keep)


def expected_state(x, keep):
    return np.asarray(x)[iota(keep)]


def panel_gather(P, keep, width=None):
    """rows of a pending panel (p, >= Nb) through the same index: (p, width), zero from Nd on (width = Nd by default)"""
    io = iota(keep)
    P = np.asarray(P)
    out = np.zeros((P.shape[0], io.size if width is None else width))
    out[:, :io.size] = P[:, io]
    return out


def brute_corner(S, keep):
    """the definition as a double loop over landmarks and their two components, no fancy indexing"""
    keep = [int(v) for v in keep]
    Nd = 3 + 2 * len(keep)

    def src(i):
        return i if i < 3 else 3 + 2 * keep[(i - 3) // 2] + (i - 3) % 2
    out = np.empty((Nd, Nd))
    for i in range(Nd):
        for j in range(Nd):
            out[i, j] = S[src(i)][src(j)]
    return out


def run_flags(keep, lc):
    """per column tile of lc landmarks: its entries are a contiguous ascending run of the source (what the library finds
    while it validates the list, and what decides which path a tile's loads take)"""
    keep = np.asarray(keep, dtype=np.int64).reshape(-1)
    return [bool(np.array_equal(keep[t:t + lc], keep[t] + np.arange(min(lc, keep.size - t)))) for t in range(0, keep.size, lc)]


# ---- the families of keep lists ---------------------------------------------------------------------------------------------

def two_runs(b, first):
    """the source's last `first` landmarks, then the others: two ascending runs, swapped"""
    assert 0 < first < b
    return np.concatenate([np.arange(b - first, b), np.arange(b - first)])


def two_runs_inside(b, lr, lc):
    """... with the boundary strictly inside a row tile and inside a column tile (None where b < 2)"""
    if b < 2:
        return None
    first = b // 2
    if first % lr == 0 or first % lc == 0:
        first += 1
    return two_runs(b, first) if first < b else None


def two_runs_on_edge(b, lr, lc):
    """... with the boundary on the edge of the first column tile, which is an edge of a row tile too (None where the map has
    no second column tile)"""
    assert lc % lr == 0
    return two_runs(b, lc) if b > lc else None


def families(b, lr, lc, seed=0):
    """name -> keep (None: the NULL list) for a source of b landmarks and tiles of lr x lc landmarks"""
    rng = np.random.default_rng(5000 + 7 * b + seed)
    subset = rng.permutation(b)[:max(1 if b else 0, (2 * b) // 3)]
    out = {"identity": None, "identity_list": np.arange(b), "reversed": np.arange(b)[::-1].copy(),
           "every_second": np.arange(0, b, 2), "random": rng.permutation(subset), "k0": np.zeros(0, dtype=np.int64)}
    if b:
        out["one"] = np.array([b // 2])
    for name, keep in (("two_runs_inside", two_runs_inside(b, lr, lc)), ("two_runs_on_edge", two_runs_on_edge(b, lr, lc))):
        if keep is not None:
            out[name] = keep
    return out


# ---- the source -------------------------------------------------------------------------------------------------------------

def payload_nan(k):
    return np.array([0x7FF8000000000000 + 0xC3C300 + k], dtype=np.uint64).view(np.float64)[0]


def source_corner(Nb, seed=0):
    """floats, not symmetric (not even in its 3 x 3 corner), with payload NaNs and -0.0 at seeded places -- one of each on
    the diagonal block of the last landmark and in the pose rows where the map has landmarks"""
    rng = np.random.default_rng(3000 + 17 * Nb + seed)
    S = rng.standard_normal((Nb, Nb))
    n = min(8, Nb * Nb // 4)
    at = rng.choice(Nb * Nb, size=2 * n, replace=False)
    S.reshape(-1)[at[:n]] = [payload_nan(k) for k in range(n)]
    S.reshape(-1)[at[n:]] = -0.0
    S[0, 1], S[1, 0], S[2, 2] = 0.25, -0.75, -0.0
    if Nb > 3:
        S[Nb - 1, Nb - 2], S[Nb - 2, Nb - 1], S[1, Nb - 1], S[Nb - 2, 2] = payload_nan(100), -0.0, payload_nan(101), -0.0
    return S


def source_state(Nb, seed=0):
    rng = np.random.default_rng(3500 + Nb + seed)
    x = rng.uniform(-9.0, 9.0, size=Nb)
    x[Nb // 2] = -0.0
    x[Nb - 1] = payload_nan(200)
    return x
