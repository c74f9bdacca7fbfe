"""-m gpu: the operand buffers of the fp64 dense handle that are allocated on first use and grow with the calls -- the stacked
Jacobians and the workspace of score, the one buffer of score_sparse, which the landmark front end reserves too, the pending
panels and the decision record.  One long-lived handle at N = 65 (ld = 128) makes a sequence of calls whose buffers are
allocated, reused, outgrown and laid out anew; after each call its outputs are compared bit for bit with those of a fresh
handle that holds the same Sigma and state and makes that call alone.  Integer operands, so S is also exact against numpy."""
import numpy as np
import pytest

import dense_landmark_cases as lc

pytestmark = pytest.mark.gpu
N = 65


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got[:3], want[:3])):   # nis, S, flags (elapsed_ms is left out)
        assert (g is None and w is None) or _bits(g, w), (what, k)


def _fresh(hip, Sigma, x):
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    return d


def test_buffers_that_grow_give_the_bits_of_a_fresh_handle(hip):
    rng = np.random.default_rng(65)
    Sigma = rng.integers(-3, 4, size=(N, N)).astype(np.float64)          # asymmetric
    x = rng.integers(-4, 5, size=N).astype(np.float64)
    d = _fresh(hip, Sigma, x)

    # score: m = 3 does not divide 64 (a copy per row group); sc_H grows once (J = 43: three groups) and is reused; (128, 16)
    # needs at least 128 * 16 * 16 = 32768 doubles of partial blocks, more than ld^2 = 16384: the handle's own workspace;
    # (1, 3) again falls back to the product buffer
    for J, m in ((1, 3), (43, 3), (2, 3), (128, 16), (1, 3)):
        H = rng.integers(-2, 3, size=(J, m, N)).astype(np.float64)
        R = rng.integers(-5, 6, size=(J, m, m)).astype(np.float64)
        nu = rng.integers(-3, 4, size=(J, m)).astype(np.float64)
        got = d.score(H, R, nu, want_S=True)
        f = _fresh(hip, Sigma, x)
        _same(got, f.score(H, R, nu, want_S=True), ("score", J, m))
        f.close()
        T = (H.reshape(-1, N) @ Sigma).reshape(H.shape)                   # small integers: exact in any order
        assert np.array_equal(got[1], np.einsum("jan,jbn->jab", T, H) + R), ("score", J, m)

    # score_sparse: the buffer grows and its layout changes between the calls (S present, absent, present)
    def sparse_operands(J, s=5, m=2):
        cols = np.stack([rng.permutation(N)[:s] for _ in range(J)]).astype(np.int32)
        Hc = rng.integers(-2, 3, size=(J, m, s)).astype(np.float64)
        R = rng.integers(-5, 6, size=(J, m, m)).astype(np.float64)
        nu = rng.integers(-3, 4, size=(J, m)).astype(np.float64)
        return cols, Hc, R, nu

    for J, want_S in ((1, True), (70, False), (2, True)):
        cols, Hc, R, nu = sparse_operands(J)
        got = d.score_sparse(cols, Hc, R, nu, want_S=want_S)
        f = _fresh(hip, Sigma, x)
        _same(got, f.score_sparse(cols, Hc, R, nu, want_S=want_S), ("score_sparse", J, want_S))
        f.close()
        assert (got[1] is not None) == want_S
        if want_S:
            blocks = np.stack([Sigma[np.ix_(c, c)] for c in cols])
            assert np.array_equal(got[1], np.einsum("jak,jkl,jbl->jab", Hc, blocks, Hc) + R), ("score_sparse", J)
    assert _bits(d.sigma, Sigma) and _bits(d.state, x)                    # scoring is read-only

    # the landmark front end: its reservation for n_max = 31 and the public call share the one buffer; the deferred
    # correction leaves two pending rows, which the scoring call after it reads through
    n_max, known = 31, 3
    xl, Sl = lc.spiral_map(n_max)
    z = [lc.reading_of(xl, 1)]
    cols, Hc, R, nu = sparse_operands(70)
    f = _fresh(hip, Sl, xl)
    d.set(Sigma=Sl)
    d.state = xl
    out = []
    for h in (d, f):
        k, assoc, best, _ = h.associate_landmarks(z, known, n_max, deferred=True)
        assert (k, assoc[0]) == (known, 1) and h.pending == 2, (k, assoc)
        out.append((best, h.score_sparse(cols, Hc, R, nu)))
    assert _bits(out[0][0], out[1][0])
    _same(out[0][1], out[1][1], "score_sparse through the pending rows")
    for h in (d, f):
        h.flush()
    assert _bits(d.sigma, f.sigma) and _bits(d.state, f.state)
    assert not _bits(d.sigma, Sl)                                         # the corrections were applied
    d.close(); f.close()
