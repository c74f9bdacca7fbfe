"""-m gpu: the measurement update and the candidate scoring of the fp64 dense handle for a Jacobian given by its non-zero
columns (ekf_dense64_correct_sparse, ekf_dense64_score_sparse, ekf_dense64_sparse.hip): H[:, cols[k]] = Hc[:, k].
Integer operands bit-exact against numpy on the embedded H; the dense calls on random operands within 1e-12 per block
(NOT bit-equal: the dense calls sum per-chunk partial panels on the matrix cores, the sparse calls one chain of s fused
multiply-adds); the bit-level properties of the fixed order of arithmetic; permutation of the list; nothing touched on
failure; the reference's own measurement() and calculate_maha_dis (live through oracle.RefEKF and from the two fixtures);
a 20-step SLAM cycle against the same cycle through the dense calls; N = 10003 with the full map (5000 candidates) in one
call; and the two time conditions against the dense calls timed in the same test.

Worst values seen on the MI355X (printed by test_zz_report): against the dense calls S 1.7e-15 per block, nis 1.4e-15,
Sigma' / state 1.1e-15 per block; permuted lists 5.4e-16; the reference's measurement() live (n = 20 / 200) and from its
fixture 3.3e-16 per block, nis 1.1e-13 relative (numpy's literal spelling is at the same 1.1e-13 on that case); its
calculate_maha_dis live 1.9e-14 / 9.3e-16 and from its fixture 1.9e-14 (the dense calls' figures for the same cases: 5.4e-16
and 1.9e-14); the 20-step cycle against the dense cycle scores 4.1e-16, state and Sigma 1.7e-16 per block; N = 10003 S 0,
nis 3.6e-16, the correction 1.9e-16 against numpy.  Times at N = 10003: correct_sparse(2, 5) 0.341 ms against
correct(m = 2) 0.589 ms; score_sparse 12.2 us for 1024 candidates and 13.6 us for the full map of 5000 against 319 us for
32 candidates through score."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest

import dense_correct_cases as dc
import dense_score_cases as ds
import dense_sparse_cases as sp
from parity import FP64_TOL, worst

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {}
TIGHT = 1e-12   # sparse against dense, and against numpy at full size: the bound the handle's tests hold against numpy


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {v:.3e}")


def _slam_inputs(n, rng):
    spec = importlib.util.spec_from_file_location("dense64_bench", os.path.join(os.path.dirname(HERE), "tools",
                                                                                "dense64_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.slam_inputs(n, rng)


def _random_sigma(N, rng):
    assert N % 2 == 1   # 3 + 2 n
    _, S, _ = _slam_inputs((N - 3) // 2, rng)
    return S + 1e-3 * np.abs(S) * rng.normal(size=S.shape)      # slightly asymmetric


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel_blocks(got, want):
    g, w = got.reshape(len(got), -1), want.reshape(len(want), -1)
    return float((np.abs(g - w).max(axis=1) / np.abs(w).max(axis=1)).max())


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- exact integers ----------------------------------------------------------------------------------------------------

def _exact_candidates(Sigma, J, m, s, order, rng):
    """J candidates with small-integer Hc and nu and R_j = D_j - H_j Sigma H_j^T, D_j = diag(2^k): S_j = D_j exactly, and
    S^-1, K, K nu, K T and the difference are exact dyadic rationals far inside 53 bits (the construction of the dense
    correct / score tests).  Candidate 0 has its list in `order`, the others scattered."""
    N = len(Sigma)
    cols = np.stack([sp.index_list(N, s, order if j == 0 else "scattered", rng) for j in range(J)])
    Hc = rng.integers(-2, 3, size=(J, m, s)).astype(np.float64)
    nu = rng.integers(-4, 5, size=(J, m)).astype(np.float64)
    R = np.empty((J, m, m))
    for j in range(J):
        G = Sigma[np.ix_(cols[j], cols[j])]
        R[j] = np.diag(2.0 ** rng.integers(1, 5, size=m)) - Hc[j] @ G @ Hc[j].T
    return cols, Hc, R, nu


@pytest.mark.parametrize("N", [1, 5, 63, 64, 65, 200, 403])
def test_sparse_integer_operands_exact(hip, N):
    """pins the row gather against the column gather (Sigma is unsymmetric), the transposes through LDS, the wave and the
    workgroup form of the scoring kernel, the strips at the padding edge and every order of the list; the identity
    propagation after each case would show anything written into the padding"""
    rng = np.random.default_rng(4000 + N)
    Sigma = rng.integers(-3, 4, size=(N, N)).astype(np.float64)
    x = rng.integers(-9, 10, size=N).astype(np.float64)
    d = hip.DensePropagator64(N)
    d.set(F=np.eye(N), Q=np.zeros((N, N)))
    cases = 0
    for m in (1, 2, 16, 17, 64):
        for s in sorted({1, 5, 16, 64} | ({N} if N <= 64 else set())):
            if m > N or s > N:
                continue
            for order in ("asc", "desc", "scattered"):
                cols, Hc, R, nu = _exact_candidates(Sigma, 3, m, s, order, rng)
                d.set(Sigma=Sigma)
                d.state = x
                nis, S, flags, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
                wS, wnis = sp.np_scores(Sigma, cols, Hc, R, nu)
                what = f"N={N} m={m} s={s} {order}"
                assert np.array_equal(S, wS) and np.array_equal(nis, wnis) and not flags.any(), what
                cnis, _ = d.correct_sparse(cols[0], Hc[0], R[0], nu[0])
                wx, wSig, wn = sp.np_correct(x, Sigma, cols[0], Hc[0], R[0], nu[0])
                got = d.sigma
                bad = got != wSig
                assert not bad.any(), f"{what}: {bad.sum()} wrong elements, first at {np.argwhere(bad)[0]}"
                assert np.array_equal(d.state, wx) and cnis == wn and cnis == nis[0], what
                d.propagate(1)                                   # I Sigma I^T + 0: exact unless the padding is not zero
                assert np.array_equal(d.sigma, got) and np.array_equal(d.state, wx), what
                cases += 1
    d.close()
    assert cases >= 3


# ---- against the dense calls -------------------------------------------------------------------------------------------

def _slam_state(N, rng):
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-2.0, 2.0, size=N - 3)])
    return x


def _general_case(N, m, s, rng):
    cols = sp.index_list(N, s, "scattered", rng)
    Hc = rng.normal(size=(m, s))
    R = 0.01 * np.eye(m) + 1e-3 * rng.normal(size=(m, m))     # neither diagonal nor symmetric
    return cols, Hc, R, rng.normal(size=m)


# General operands have m well below s (or m = s = 1): S = Hc G Hc^T + R is then conditioned like G's landmark block
# (a wide Gaussian Hc has a condition number near ((sqrt s + sqrt m) / (sqrt s - sqrt m))^2 <= 34 here), so a difference
# of a few ulp in S between the two summation orders stays a few ulp in K and nis.  A square Hc over a block that mixes
# pose (1e-4) and landmark (100) variances would amplify those ulp by cond(S) ~ 1e8 and measure the operands, not the code.
GENERAL = [(43, 1, 1), (43, 2, 5), (403, 8, 16), (403, 5, 64), (2003, 16, 64), (2003, 32, 64)]


@pytest.mark.parametrize("N,m,s", [(43, 2, 0), (403, 2, 0), (2003, 2, 0)] + GENERAL)
def test_sparse_against_dense_calls(hip, N, m, s):
    """s = 0: SLAM-shaped (the reference's five columns for a random landmark).  Sigma', state, nis from correct_sparse
    against correct with the embedded H, S and nis from score_sparse against score: <= 1e-12 per block, not bit-equal"""
    rng = np.random.default_rng(13 * N + 5 * m + s)
    Sigma = _random_sigma(N, rng)
    x = _slam_state(N, rng)
    J = 6
    if s == 0:
        picks = rng.choice((N - 3) // 2, size=J, replace=False)
        terms = [sp.slam_terms(x[:3], x, int(i), 0.7, -0.4) for i in picks]
        cols, Hc = np.stack([t[0] for t in terms]), np.stack([t[1] for t in terms])
        R, nu = np.stack([t[2] for t in terms]), np.stack([t[4] for t in terms])
    else:
        terms = [_general_case(N, m, s, rng) for _ in range(J)]
        cols, Hc, R, nu = (np.stack([t[k] for t in terms]) for k in range(4))
    H = sp.embed(cols, Hc, N)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    nis_s, S_s, f_s, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
    nis_d, S_d, f_d, _ = d.score(H, R, nu, want_S=True)
    assert not f_s.any() and not f_d.any()
    eS, en = _rel_blocks(S_s, S_d), float((np.abs(nis_s - nis_d) / np.abs(nis_d)).max())
    _note("vs_dense_S", eS); _note("vs_dense_score_nis", en)
    assert eS <= TIGHT and en <= TIGHT, (eS, en)
    cn_s, _ = d.correct_sparse(cols[0], Hc[0], R[0], nu[0])
    got_s, x_s = d.sigma, d.state
    d.set(Sigma=Sigma)
    d.state = x
    cn_d, _ = d.correct(H[0], R[0], nu[0])
    got_d, x_d = d.sigma, d.state
    d.close()
    w, e = worst(x_s, got_s, x_d, got_d)
    ec = abs(cn_s - cn_d) / abs(cn_d)
    _note("vs_dense_correct", w); _note("vs_dense_correct_nis", ec)
    assert w <= TIGHT and ec <= TIGHT, (e, ec)
    assert np.abs(got_s - Sigma).max() > 0.0


# ---- bit-level properties of the fixed order of arithmetic -------------------------------------------------------------

@pytest.mark.parametrize("N,m,s", [(403, 2, 5), (403, 16, 16), (403, 16, 64), (403, 17, 5), (2003, 64, 64)])
def test_sparse_same_operands_same_bits(hip, N, m, s):
    """(2, 5) and (16, 16): a wave per candidate; (16, 64): m <= 16 but the block does not fit a wave's share of LDS;
    (17, 5), (64, 64): a workgroup per candidate"""
    rng = np.random.default_rng(17 * N + 3 * m + s)
    Sigma = _random_sigma(N, rng)
    x = rng.normal(size=N)
    J = 9
    terms = [_general_case(N, m, s, rng) for _ in range(J)]
    cols, Hc, R, nu = (np.stack([t[k] for t in terms]) for k in range(4))
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    nis, S, flags, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
    assert not flags.any()
    a, b, f, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)                            # the same call twice
    assert _same_bits(a, nis) and _same_bits(b, S) and np.array_equal(f, flags)
    for j in (0, J // 2, J - 1):                                                         # alone
        a, b, f, _ = d.score_sparse(cols[j:j + 1], Hc[j:j + 1], R[j:j + 1], nu[j:j + 1], want_S=True)
        assert _same_bits(a[0], nis[j]) and _same_bits(b[0], S[j]) and f[0] == flags[j], j
    perm = rng.permutation(J)                                                            # first, last, in the middle
    a, b, f, _ = d.score_sparse(cols[perm], Hc[perm], R[perm], nu[perm], want_S=True)
    assert _same_bits(a, nis[perm]) and _same_bits(b, S[perm])
    a, b, _, _ = d.score_sparse(cols[perm][:4], Hc[perm][:4], R[perm][:4], nu[perm][:4], want_S=True)
    assert _same_bits(a, nis[perm][:4]) and _same_bits(b, S[perm][:4])                   # another batch size
    a, b, _, _ = d.score_sparse(cols, Hc, R[0], nu, want_S=True)                         # R shared against replicated
    a2, b2, _, _ = d.score_sparse(cols, Hc, np.stack([R[0]] * J), nu, want_S=True)
    assert _same_bits(a, a2) and _same_bits(b, b2)
    for j in (3, 0):                                                                     # score, then the correction
        d.set(Sigma=Sigma)
        d.state = x
        a, b, _, _ = d.score_sparse(cols[j:j + 1], Hc[j:j + 1], R[j:j + 1], nu[j:j + 1], want_S=True)
        cn, _ = d.correct_sparse(cols[j], Hc[j], R[j], nu[j])
        assert _same_bits(cn, a[0]) and _same_bits(a[0], nis[j]) and _same_bits(b[0], S[j]), j
    first = (d.sigma, d.state)
    d.set(Sigma=Sigma)
    d.state = x
    d.correct_sparse(cols[0], Hc[0], R[0], nu[0])                                        # the same correction twice
    assert _same_bits(d.sigma, first[0]) and _same_bits(d.state, first[1])
    d.close()


@pytest.mark.parametrize("m,s", [(2, 5), (16, 16), (17, 33), (64, 64)])
def test_sparse_bits_do_not_depend_on_where_the_columns_sit(hip, m, s):
    """the same Sigma[cols, cols], Hc, R, nu planted at three column sets in each of two N"""
    rng = np.random.default_rng(100 * m + s)
    G = rng.normal(size=(s, s)) + 3.0 * np.eye(s)
    _, Hc, R, nu = _general_case(1000, m, s, rng)
    seen = []
    for N in (203, 1003):
        base = rng.normal(size=(N, N))
        d = hip.DensePropagator64(N)
        for order in ("asc", "desc", "scattered"):
            cols = sp.index_list(N, s, order, rng)
            Sigma = base.copy()
            Sigma[np.ix_(cols, cols)] = G
            d.set(Sigma=Sigma)
            nis, S, flags, _ = d.score_sparse(cols[None], Hc[None], R, nu[None], want_S=True)
            cn, _ = d.correct_sparse(cols, Hc, R, nu)
            seen.append((nis[0], S[0], int(flags[0]), cn))
        d.close()
    for got in seen[1:]:
        assert _same_bits(got[0], seen[0][0]) and _same_bits(got[1], seen[0][1]) and got[2] == seen[0][2] == 0
        assert _same_bits(got[3], seen[0][3])


@pytest.mark.parametrize("N,m,s", [(403, 2, 5), (403, 8, 16), (2003, 16, 64)])
def test_sparse_permuted_list_agrees(hip, N, m, s):
    """permuting cols together with the columns of Hc reorders every sum: agreement to 1e-12, not bit for bit"""
    rng = np.random.default_rng(23 * N + m + s)
    Sigma = _random_sigma(N, rng)
    x = rng.normal(size=N)
    cols, Hc, R, nu = _general_case(N, m, s, rng)
    perm = rng.permutation(s)
    d = hip.DensePropagator64(N)
    out = []
    for c, h in ((cols, Hc), (cols[perm], np.ascontiguousarray(Hc[:, perm]))):
        d.set(Sigma=Sigma)
        d.state = x
        nis, S, _, _ = d.score_sparse(c[None], h[None], R, nu[None], want_S=True)
        cn, _ = d.correct_sparse(c, h, R, nu)
        out.append((nis[0], S[0], cn, d.state, d.sigma))
    d.close()
    w, e = worst(out[1][3], out[1][4], out[0][3], out[0][4])
    eS, en = _rel(out[1][1], out[0][1]), abs(out[1][0] - out[0][0]) / abs(out[0][0])
    _note("permuted", max(w, eS, en))
    assert w <= TIGHT and eS <= TIGHT and en <= TIGHT and abs(out[1][2] - out[0][2]) <= TIGHT * abs(out[0][2]), e


# ---- untouched on failure ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("why", ["equal_rows", "nan"])
def test_correct_sparse_singular_S_leaves_everything(hip, why):
    """two equal integer rows of Hc with R = 0: S = [[a, a], [a, a]] bit for bit, and a - a * (a / a) is an exact zero"""
    N, m, s = 203, 2, 5
    rng = np.random.default_rng(29)
    Sigma = _random_sigma(N, rng)
    x = rng.normal(size=N)
    cols = sp.index_list(N, s, "scattered", rng)
    Hc = np.tile(rng.integers(1, 4, size=(1, s)).astype(np.float64), (m, 1))
    R = np.zeros((m, m))
    if why == "nan":
        Hc, R = rng.normal(size=(m, s)), 0.01 * np.eye(m)
        Hc[1, 2] = np.nan
    nu = rng.normal(size=m)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    with pytest.raises(hip.EkfError) as e:
        d.correct_sparse(cols, Hc, R, nu)
    assert e.value.status == 5                                   # EKF_ERR_STATE
    assert _same_bits(d.sigma, Sigma) and _same_bits(d.state, x)
    c2, H2, R2, nu2 = _general_case(N, 2, 5, rng)                # the handle works afterwards
    wx, wS, wn = sp.np_correct(x, Sigma, c2, H2, R2, nu2)
    nis, _ = d.correct_sparse(c2, H2, R2, nu2)
    assert worst(d.state, d.sigma, wx, wS)[0] <= FP64_TOL and abs(nis - wn) <= FP64_TOL * abs(wn)
    d.close()


@pytest.mark.parametrize("N,m,s", [(203, 2, 5), (403, 17, 16)])
def test_score_sparse_flags_one_candidate_only(hip, N, m, s):
    rng = np.random.default_rng(N + m)
    Sigma = _random_sigma(N, rng)
    x = rng.normal(size=N)
    J = 11
    terms = [_general_case(N, m, s, rng) for _ in range(J)]
    cols, Hc, R, nu = (np.stack([t[k] for t in terms]) for k in range(4))
    sing, nan = 1, J - 2
    Hb, Rb = Hc.copy(), R.copy()
    Hb[sing] = np.tile(rng.integers(1, 4, size=(1, s)).astype(np.float64), (m, 1))
    Rb[sing] = 0.0                                               # equal integer rows, R = 0: every row of S the same
    Hb[nan, 0, s // 2] = np.nan
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    nis0, S0, f0, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
    nis1, S1, f1, _ = d.score_sparse(cols, Hb, Rb, nu, want_S=True)   # returns: the call is EKF_OK
    good = np.ones(J, dtype=bool)
    good[[sing, nan]] = False
    assert not f0.any() and f1[sing] == 1 and f1[nan] == 1 and not f1[good].any()
    assert np.isnan(nis1[sing]) and np.isnan(nis1[nan])
    assert _same_bits(nis0[good], nis1[good]) and _same_bits(S0[good], S1[good])
    assert _same_bits(d.sigma, Sigma) and _same_bits(d.state, x)
    # a NaN in Sigma outside every listed row / column pair changes no score
    used = np.zeros((N, N), dtype=bool)
    for c in cols:
        used[np.ix_(c, c)] = True
    free = np.argwhere(~used)
    Sn = Sigma.copy()
    for i, j in free[rng.choice(len(free), size=20, replace=False)]:
        Sn[i, j] = np.nan
    d.set(Sigma=Sn)
    nis2, S2, f2, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
    d.close()
    assert _same_bits(nis2, nis0) and _same_bits(S2, S0) and not f2.any()


def test_score_sparse_is_read_only(hip):
    """Sigma and the state directly; F and Q through the propagation that follows (bit for bit with and without scoring)"""
    N = 403
    rng = np.random.default_rng(47)
    F, S, Q = _slam_inputs((N - 3) // 2, rng)
    x = rng.normal(size=N)
    terms = [_general_case(N, 2, 5, rng) for _ in range(40)]
    cols, Hc, R, nu = (np.stack([t[k] for t in terms]) for k in range(4))
    big = [_general_case(N, 64, 64, rng) for _ in range(2)]
    bc, bH, bR, bnu = (np.stack([t[k] for t in big]) for k in range(4))
    out = []
    for with_score in (False, True):
        d = hip.DensePropagator64(N)
        d.set(F, S, Q)
        d.state = x
        if with_score:
            d.score_sparse(cols, Hc, R, nu, want_S=True)
            d.score_sparse(bc, bH, bR, bnu)
            assert _same_bits(d.sigma, S) and _same_bits(d.state, x)
        d.propagate(1)
        if with_score:
            d.score_sparse(cols, Hc, R, nu)
        nis, _ = d.correct(sp.embed(cols[0], Hc[0], N), R[0], nu[0])
        out.append((d.sigma, d.state, nis))
        d.close()
    assert _same_bits(out[0][0], out[1][0]) and _same_bits(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_sparse_index_errors_with_a_live_handle(hip):
    """an index >= N passes the NULL-handle checks of the host test only with a handle: EKF_ERR_INVALID, nothing touched"""
    N = 30
    rng = np.random.default_rng(3)
    Sigma, x = rng.normal(size=(N, N)), rng.normal(size=N)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    lib = hip.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    Hc, R, nu = np.ones((2, 5)), np.eye(2), np.ones(2)
    nis, flags = ctypes.c_double(), np.zeros(2, dtype=np.int32)
    for bad in ([0, 1, 2, 7, N], [0, 1, 2, 7, 1 << 30], [0, 1, 2, 7, 7], [0, -1, 2, 7, 8]):
        c = np.array(bad, dtype=np.int32)
        st = lib.ekf_dense64_correct_sparse(d._h, 2, 5, c.ctypes.data_as(ip), Hc.ctypes.data_as(dp), R.ctypes.data_as(dp),
                                            nu.ctypes.data_as(dp), ctypes.byref(nis), None)
        assert st == 1 and b"ekf_dense64_correct_sparse" in lib.ekf_last_error(), bad
        c2 = np.array([[0, 1, 2, 3, 4], bad], dtype=np.int32)
        H2, nu2 = np.ones((2, 2, 5)), np.ones((2, 2))
        st = lib.ekf_dense64_score_sparse(d._h, 2, 2, 5, c2.ctypes.data_as(ip), H2.ctypes.data_as(dp),
                                          R.ctypes.data_as(dp), 1, nu2.ctypes.data_as(dp), None, None,
                                          flags.ctypes.data_as(ip), None)
        assert st == 1 and b"ekf_dense64_score_sparse" in lib.ekf_last_error(), bad
        assert _same_bits(d.sigma, Sigma) and _same_bits(d.state, x)
    with pytest.raises(ValueError):
        d.correct_sparse([0, 1, 2, 7, N], Hc, R, nu)
    with pytest.raises(ValueError):
        d.correct_sparse(list(range(N)), np.ones((N + 1, N)), np.eye(N + 1))
    nis, ms = d.correct_sparse([0, 1, 2, 7, 8], Hc, R)            # no innovation: the state stays, no score
    assert nis is None and ms > 0.0 and _same_bits(d.state, x)
    d.close()


# ---- the reference -----------------------------------------------------------------------------------------------------

def _gpu_sparse_correct(hip, N):
    d = hip.DensePropagator64(N)

    def correct(state, Sigma, cols, Hc, R, nu):
        d.set(Sigma=Sigma)
        d.state = state
        nis, _ = d.correct_sparse(cols, Hc, R, nu)
        return d.state, d.sigma, nis
    return d, sp.sparse_correct_of(correct)


def _check_measurement(hip, case, key):
    d, correct = _gpu_sparse_correct(hip, len(case["state0"]))
    s, c, nis = dc.replay_case(case, correct)
    d.close()
    w, e = worst(s, c, case["state1"], case["cov1"])
    rel = abs(nis - float(case["maha"])) / abs(float(case["maha"]))
    _note(key, w); _note(key + "_nis", rel)
    assert w <= FP64_TOL, e
    assert rel <= FP64_TOL, (nis, float(case["maha"]))


def _check_scores(hip, case, key):
    state, cov, n = case["state"], case["cov"], int(case["n"])
    d = hip.DensePropagator64(len(state))
    d.set(Sigma=cov)
    d.state = state
    for k, (sx, sy) in enumerate(case["readings"]):
        ref = case["maha"][k]
        assert ds.margins_hold(ref), f"reading {k}: the scenario's seed must be replaced"   # on the REFERENCE's scores
        cols, Hc, R, nu = sp.candidate_terms(state, sx, sy)
        nis, _, flags, _ = d.score_sparse(cols, Hc, R, nu)        # every landmark in one call: J = n, m = 2, s = 5
        assert nis.shape == (n,) and not flags.any()
        rel = float((np.abs(nis - ref) / np.abs(ref)).max())
        _note(key, rel)
        assert rel <= FP64_TOL, (k, rel)
        assert ds.reference_rule(nis) == ds.reference_rule(ref), k
    d.close()


def _reference_or_skip(oracle):
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")


@pytest.mark.parametrize("n", [20, 200])
@pytest.mark.parametrize("name,nvis,off", dc.CASES)
def test_correct_sparse_against_the_reference(hip, oracle, n, name, nvis, off):
    """measurement() of the reference's own ekf_slam.cpp, one sparse correction (m = 2, s = 5) per visible landmark"""
    _reference_or_skip(oracle)
    _check_measurement(hip, dc.record_case(oracle.RefEKF, n, nvis, n + off), f"reference_live_measurement_n{n}")


@pytest.mark.parametrize("n", [20, 200])
def test_score_sparse_against_the_reference(hip, oracle, n):
    """calculate_maha_dis of the reference for every reading x every landmark; the same winner and gate class"""
    _reference_or_skip(oracle)
    _check_scores(hip, ds.record_scores(oracle.RefEKF, n, ds.SEEDS[n]), f"reference_live_scores_n{n}")


@pytest.mark.parametrize("name", [c[0] for c in dc.CASES])
def test_correct_sparse_reference_fixture_replayed(hip, name):
    """tests/golden/dense_correct_ref.npz through the sparse call -- never skips"""
    z = np.load(os.path.join(HERE, "golden", "dense_correct_ref.npz"))
    case = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    assert int(case["vis"].sum()) == dict((c[0], c[1]) for c in dc.CASES)[name]
    _check_measurement(hip, case, "reference_fixture_measurement")


def test_score_sparse_reference_fixture(hip):
    """tests/golden/dense_score_ref.npz through the sparse call -- never skips"""
    z = np.load(os.path.join(HERE, "golden", "dense_score_ref.npz"))
    _check_scores(hip, {k: z[k] for k in z.files}, "reference_fixture_scores")


# ---- the cycle ---------------------------------------------------------------------------------------------------------

def cycle_scenario(n, steps, seed):
    """a map of n landmarks known to about 3 cm, a pose that moves a little every step and one noisy sighting per step"""
    rng = np.random.default_rng(seed)
    N = 3 + 2 * n
    world = rng.uniform(-2.0, 2.0, size=(n, 2))
    _, S, _ = _slam_inputs(n, rng)
    S[3:, 3:] *= 1e-5                                            # landmark variances ~1e-3
    S[:3, 3:] *= 1e-2
    S[3:, :3] *= 1e-2
    S = S + 1e-3 * np.abs(S) * rng.normal(size=S.shape)
    x0 = np.concatenate([np.zeros(3), (world + rng.normal(0, 0.02, size=(n, 2))).reshape(-1)])
    pose = np.zeros(3)
    moves = []
    for _ in range(steps):
        dx = np.array([rng.uniform(-0.05, 0.05), rng.uniform(0.0, 0.03), rng.uniform(-0.01, 0.01)])
        Fr = np.eye(3)
        Fr[1, 0], Fr[2, 0] = rng.uniform(-0.03, 0.03, size=2)   # the shape of the reference's At (:84-97)
        pose = pose + dx
        L = int(rng.integers(0, n))
        dw = world[L] - pose[1:] + rng.normal(0, 0.01, size=2)
        c, s_ = math.cos(pose[0]), math.sin(pose[0])
        moves.append((Fr, 1e-6 * np.eye(3), dx, (c * dw[0] + s_ * dw[1], -s_ * dw[0] + c * dw[1])))
    return N, S, x0, moves


def run_cycle(d, moves, sparse):
    """propagate_block, score every known landmark, the reference's rule, correct the winner -> decisions, scores"""
    decisions, scores = [], []
    for Fr, Qr, dx, (sx, sy) in moves:
        d.propagate_block(0, Fr, Qr, dx)
        state = d.state
        cols, Hc, R, nu = sp.candidate_terms(state, sx, sy)
        if sparse:
            nis, _, flags, _ = d.score_sparse(cols, Hc, R, nu)
        else:
            nis, _, flags, _ = d.score(sp.embed(cols, Hc, d.N), R, nu)
        assert not flags.any()
        win, kind = ds.reference_rule(nis)
        decisions.append((win, kind))
        scores.append(nis)
        if kind == "update":
            c, h, R, _, wrapped = sp.slam_terms(state[:3], state, win, sx, sy)
            if sparse:
                d.correct_sparse(c, h, R, wrapped)
            else:
                d.correct(sp.embed(c, h, d.N), R, wrapped)
    return decisions, scores


def test_sparse_slam_cycle_against_dense_cycle(hip):
    """20 steps at n = 200: propagate_block -> score_sparse over every known landmark -> reference_rule -> correct_sparse
    on the winner, against the same cycle through score / correct: identical decisions, <= 1e-12 per block at the end"""
    N, S, x0, moves = cycle_scenario(200, 20, 2025)
    out = []
    for sparse in (True, False):
        d = hip.DensePropagator64(N)
        d.set(Sigma=S)
        d.state = x0
        dec, sc = run_cycle(d, moves, sparse)
        out.append((dec, sc, d.state, d.sigma))
        d.close()
    for k, nis in enumerate(out[1][1]):
        assert ds.margins_hold(nis), f"step {k}: the seed must be replaced"
    assert out[0][0] == out[1][0]
    assert sum(kind == "update" for _, kind in out[0][0]) >= 5
    en = max(float((np.abs(a - b) / np.abs(b)).max()) for a, b in zip(out[0][1], out[1][1]))
    w, e = worst(out[0][2], out[0][3], out[1][2], out[1][3])
    _note("cycle_scores", en); _note("cycle_state_cov", w)
    assert en <= TIGHT and w <= TIGHT, (en, e)


# ---- full size -----------------------------------------------------------------------------------------------------------

def _full_size_sigma(N, rng):
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    S += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))   # asymmetric
    return S


def _median(f, iters=9, warmup=2):
    ms = [f() for _ in range(warmup + iters)][warmup:]
    return float(np.median(ms))


def test_sparse_full_size_n10003_and_time(hip):
    """the reference's full-map association (every one of the 5000 landmarks, :300-314) in ONE call, which the dense call
    cannot take; sampled candidates against numpy on the gathered blocks; correct_sparse(2, 5) on sampled rows and
    columns; then the two time conditions, medians of 9 HIP-event times after 2 untimed calls, against the dense calls
    timed here: (a) correct_sparse(m = 2, s = 5) < correct(m = 2) with the embedded H, (b) score_sparse(J = 1024) <
    score(J = 32), one row group of the dense call"""
    N, n = 10003, 5000
    rng = np.random.default_rng(8)
    Sigma = _full_size_sigma(N, rng)
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    cols, Hc, R, nu = sp.candidate_terms(x, 0.7, -0.4)
    assert cols.shape == (n, 5) and n * 2 > hip.DensePropagator64.SCORE_MAX_ROWS
    nis, S, flags, ms_full = d.score_sparse(cols, Hc, R, nu, want_S=True)
    assert not flags.any()
    print(f"score_sparse J={n} m=2 s=5 at N={N}: {ms_full:.4f} ms")
    for j in sorted(set([0, 1, n - 1] + list(rng.integers(0, n, size=20)))):
        G = Sigma[np.ix_(cols[j], cols[j])]
        wS = Hc[j] @ G @ Hc[j].T + R
        wn = float(nu[j] @ np.linalg.inv(wS) @ nu[j])
        eS, en = _rel(S[j], wS), abs(nis[j] - wn) / abs(wn)
        _note("full_size_S", eS); _note("full_size_nis", en)
        assert eS <= TIGHT and en <= TIGHT, (j, eS, en)
    assert _same_bits(d.state, x)
    # one correction on sampled rows and columns
    j = 3333
    last = (N - 1) // 128 * 128
    rows = np.array(sorted(set([0, 1, 2, N - 1, 3 + 2 * j, 4 + 2 * j] + list(range(last, N, 3)) +
                               list(rng.integers(0, N, size=18)))))
    cc = np.array(sorted(set([0, 1, 2, N - 1, N - 2, 3 + 2 * j, 4 + 2 * j] + list(rng.integers(0, N, size=12)))))
    T = Hc[j] @ Sigma[cols[j], :]
    U = Sigma[:, cols[j]] @ Hc[j].T
    Si = np.linalg.inv(T[:, cols[j]] @ Hc[j].T + R)
    K = U @ Si
    cn, ms_one = d.correct_sparse(cols[j], Hc[j], R, nu[j])
    got = d.sigma
    wr, wc, wx = Sigma[rows] - K[rows] @ T, Sigma[:, cc] - K @ T[:, cc], x + K @ nu[j]
    errs = (_rel(got[rows], wr), _rel(got[:, cc], wc), _rel(d.state, wx), abs(cn - nis[j]) / abs(nis[j]))
    del got
    _note("full_size_correct", max(errs))
    assert max(errs) <= TIGHT, errs
    # time: the same handle, Sigma as the correction left it (times do not depend on the values)
    Hd = sp.embed(cols[j], Hc[j], N)
    t_sparse = _median(lambda: d.correct_sparse(cols[j], Hc[j], R, nu[j])[1])
    t_dense = _median(lambda: d.correct(Hd, R, nu[j])[1])
    t_sparse2 = _median(lambda: d.correct_sparse(cols[j], Hc[j], R, nu[j])[1])
    print(f"(a) correct_sparse(2, 5) {t_sparse:.4f} ms (again {t_sparse2:.4f}) against correct(m = 2) {t_dense:.4f} ms: "
          f"{t_dense / t_sparse:.2f} x")
    H32 = sp.embed(cols[:32], Hc[:32], N)
    t_s1024 = _median(lambda: d.score_sparse(cols[:1024], Hc[:1024], R, nu[:1024])[3])
    t_d32 = _median(lambda: d.score(H32, R, nu[:32])[3])
    t_full = _median(lambda: d.score_sparse(cols, Hc, R, nu)[3])
    print(f"(b) score_sparse(J = 1024) {t_s1024:.4f} ms against score(J = 32) {t_d32:.4f} ms: {t_d32 / t_s1024:.1f} x; "
          f"score_sparse(J = {n}) {t_full:.4f} ms")
    d.close()
    assert t_sparse < t_dense, (t_sparse, t_dense)
    assert t_s1024 < t_d32, (t_s1024, t_d32)


def test_zz_report():
    for k in sorted(WORST):
        print(f"dense64 sparse worst {k}: {WORST[k]:.3e}")
    assert all(v <= FP64_TOL for v in WORST.values())
