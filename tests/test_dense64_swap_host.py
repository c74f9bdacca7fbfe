"""CPU (not gpu): the numpy model of ekf_dense64_swap_blocks (tests/dense_swap_cases.py) is what the call is specified to
be -- an involution, equal to P Sigma P^T with an explicit P, compatible with the carried representation exactly, and, with
init_block(s = 0) and the corner taken, the deletion of a landmark's rows and columns; and the symbol is in the header, in
capi.SYMBOLS and in the built library."""
import ctypes

import numpy as np
import pytest

import dense_swap_cases as sc
from ekf_slam_ml_amd import capi


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("N", sc.GRID_N)
def test_model_is_an_involution_and_keeps_every_bit(N):
    S, x = sc.unique_data(N)
    assert np.isnan(S).any() and (np.signbit(S) & (S == 0)).any()
    for a, b, r in sc.cases(N):
        S1, x1 = sc.swap_model(S, x, a, b, r)
        assert not np.array_equal(_bits(S1), _bits(S)) and np.array_equal(_bits(x1[a:a + r]), _bits(x[b:b + r]))
        assert sorted(_bits(S1).ravel()) == sorted(_bits(S).ravel())       # a permutation of the entries, bits and all
        S2, x2 = sc.swap_model(S1, x1, a, b, r)
        assert np.array_equal(_bits(S2), _bits(S)) and np.array_equal(_bits(x2), _bits(x)), (N, a, b, r)
        Sr, xr = sc.swap_model(S, x, b, a, r)                              # (b, a) is (a, b)
        assert np.array_equal(_bits(Sr), _bits(S1)) and np.array_equal(_bits(xr), _bits(x1))
    assert len(sc.cases(N)) >= 1


def test_grid_holds_the_edges():
    g = sc.grid()
    assert (128, 0, 64, 64) in g                                           # N = 2 r: nothing outside A u B
    assert any(a == 62 and r == 3 for _, a, _, r in g) and any(b == a + r for _, a, b, r in g)
    assert any(a == 0 for _, a, _, _ in g) and any(b + r == N for N, _, b, r in g)
    assert any(a // 64 == (b + r - 1) // 64 for _, a, b, r in g) and any(a // 64 != b // 64 for _, a, b, _ in g)
    assert {N for N, *_ in g} == set(sc.GRID_N) and {r for *_, r in g} == set(sc.GRID_R)


@pytest.mark.parametrize("N,a,b,r", [(4, 0, 2, 2), (67, 62, 65, 2), (131, 3, 67, 64), (203, 62, 200, 3)])
def test_model_equals_p_sigma_pt_and_the_elementwise_contract(N, a, b, r):
    rng = np.random.default_rng(N)
    S = rng.integers(-50, 51, size=(N, N)).astype(np.float64)
    x = rng.integers(-9, 10, size=N).astype(np.float64)
    P = sc.explicit_P(N, a, b, r)
    S1, x1 = sc.swap_model(S, x, a, b, r)
    assert np.array_equal(S1, P @ S @ P.T) and np.array_equal(x1, P @ x)
    A, B = np.arange(a, a + r), np.arange(b, b + r)
    out = np.array([i for i in range(N) if i not in set(A) | set(B)], dtype=int)
    assert np.array_equal(S1[np.ix_(A, out)], S[np.ix_(B, out)]) and np.array_equal(S1[np.ix_(B, out)], S[np.ix_(A, out)])
    assert np.array_equal(S1[np.ix_(out, A)], S[np.ix_(out, B)]) and np.array_equal(S1[np.ix_(out, B)], S[np.ix_(out, A)])
    assert np.array_equal(S1[np.ix_(out, out)], S[np.ix_(out, out)])
    assert np.array_equal(S1[np.ix_(A, A)], S[np.ix_(B, B)]) and np.array_equal(S1[np.ix_(B, B)], S[np.ix_(A, A)])
    # the off-diagonal blocks are exchanged, not transposed
    assert np.array_equal(S1[np.ix_(A, B)], S[np.ix_(B, A)]) and np.array_equal(S1[np.ix_(B, A)], S[np.ix_(A, B)])
    assert not np.array_equal(S1[np.ix_(A, B)], S[np.ix_(A, B)].T)


@pytest.mark.parametrize("N,a,b,r,p", [(67, 62, 65, 2, 2), (131, 3, 67, 64, 64), (203, 0, 200, 3, 17)])
def test_carried_algebra_is_exact_on_integers(N, a, b, r, p):
    """P (Sigma_base - K^T T) P^T == P Sigma_base P^T - (K P^T)^T (T P^T): the swap on Sigma_base and on the rows of both
    panels is the swap of the current covariance, in integers exactly"""
    rng = np.random.default_rng(7 * N + p)
    base = rng.integers(-9, 10, size=(N, N)).astype(np.float64)
    Kt, Tp = (rng.integers(-3, 4, size=(p, N)).astype(np.float64) for _ in range(2))
    x = rng.integers(-9, 10, size=N).astype(np.float64)
    cur = base - Kt.T @ Tp
    P = sc.explicit_P(N, a, b, r)
    Kp, Tq = sc.swap_panels(Kt, Tp, a, b, r)
    assert np.array_equal(Kp, Kt @ P.T) and np.array_equal(Tq, Tp @ P.T)
    want, _ = sc.swap_model(cur, x, a, b, r)
    got = sc.swap_model(base, x, a, b, r)[0] - Kp.T @ Tq
    assert np.array_equal(got, want) and np.array_equal(want, P @ cur @ P.T)
    # the read-through on permuted lists is the read-through on the original lists
    q = sc.perm(N, a, b, r)
    rows, cols = rng.permutation(N)[:9], rng.permutation(N)[:11]
    assert np.array_equal(got[np.ix_(q[rows], q[cols])], cur[np.ix_(rows, cols)])


@pytest.mark.parametrize("n,i", [(20, 7), (20, 0), (20, 18), (5, 2)])
def test_removal_recipe_equals_deleting_rows_and_columns(n, i):
    """swap landmark i with the last one, zero the last block's rows and columns, take the corner: np.delete on both axes
    with the last landmark moved into slot i.  Equal as arrays."""
    N = 3 + 2 * n
    rng = np.random.default_rng(n + i)
    S = sc.spd(N, rng)
    x = rng.normal(size=N)
    first, last = 3 + 2 * i, N - 2
    S1, x1 = sc.swap_model(S, x, first, last, 2)
    S1[last:, :] = 0.0
    S1[:, last:] = 0.0
    S1[last:, last:] = 100.0 * np.eye(2)
    keep = np.arange(N - 2)
    keep[first:first + 2] = [last, last + 1]                               # the last landmark in slot i
    assert np.array_equal(S1[:last, :last], S[np.ix_(keep, keep)]) and np.array_equal(x1[:last], x[keep])
    # up to the order of the survivors that is the deletion itself
    gone = np.delete(np.delete(S, [first, first + 1], axis=0), [first, first + 1], axis=1)
    back = np.argsort(keep, kind="stable")                                 # the survivors in their original order
    assert np.array_equal(S1[:last, :last][np.ix_(back, back)], gone)
    assert np.array_equal(x1[:last][back], np.delete(x, [first, first + 1]))
    assert not S1[:last, last:].any() and not S1[last:, :last].any()       # decoupled: set_live(N - 2) is exact


def test_symbol_is_declared_listed_and_exported():
    assert "ekf_dense64_swap_blocks" in capi.SYMBOLS
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "ekf_dense64_swap_blocks")
    assert hasattr(capi.DensePropagator64, "swap_blocks")
    fn = capi.load().ekf_dense64_swap_blocks
    assert len(fn.argtypes) == 5
    assert fn(None, 0, 2, 2, None) == 1                                    # a NULL handle is refused before any device is looked at
    assert b"null handle" in capi.load().ekf_last_error()
