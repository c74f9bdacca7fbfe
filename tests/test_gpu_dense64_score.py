"""-m gpu: batched Mahalanobis scoring of candidates on the fp64 dense handle (ekf_dense64_score, ekf_dense64_score.hip)
-- the reference's calculate_maha_dis (ekf_slam.cpp:217-276) for J arbitrary m x N Jacobians, read-only:
integer operands bit-exact, random SLAM-shaped operands within FP64_TOL of numpy, the reference's own scores (live through
oracle.RefEKF and from tests/golden/dense_score_ref.npz) with the same decisions, Sigma / state / propagate / correct
untouched by scoring, agreement with correct's nis, flagged singular candidates among good ones, position independence
and run-to-run determinism, N = 10003.

Worst values seen on the MI355X (printed by test_zz_report): random operands S 1.7e-15 per block, nis 1.6e-15 relative;
the reference live (n = 20 / 200) 1.9e-14 / 9.3e-16 and its fixture 1.9e-14 (numpy's literal spelling is at the same 1.9e-14
from calculate_maha_dis); nis against correct's 4.9e-16; the 20-step cycle S 1.2e-15, nis 1.2e-15, covariance 6.7e-15,
state 3.4e-14; N = 10003 S 1.8e-15, nis 1.1e-15."""
import importlib.util
import os

import numpy as np
import pytest

import dense_correct_cases as dc
import dense_score_cases as ds
from parity import FP64_TOL, cov_err, state_err

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {}
MAX_ROWS = 2048


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {v:.3e}")


def _slam_inputs(n, rng):
    spec = importlib.util.spec_from_file_location("dense64_bench", os.path.join(os.path.dirname(HERE), "tools",
                                                                                "dense64_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.slam_inputs(n, rng)


def _rel_blocks(got, want):
    """per candidate: max |got - want| over the block relative to the block's own max |want|"""
    g, w = got.reshape(len(got), -1), want.reshape(len(want), -1)
    return float((np.abs(g - w).max(axis=1) / np.abs(w).max(axis=1)).max())


def _batch_sizes(m):
    """one candidate, a group exactly full, one over the group boundary, and all the rows one call may have"""
    cpg = 64 // m
    return sorted({1, cpg, cpg + 1, MAX_ROWS // m})


# ---- 4: exact ----------------------------------------------------------------------------------------------------------

def _exact_S(Sigma, H, R):
    T = (H.reshape(-1, H.shape[2]) @ Sigma).reshape(H.shape)          # small integers: exact in any order
    return np.einsum("jan,jbn->jab", T, H) + R


@pytest.mark.parametrize("N", [1, 2, 43, 128, 129, 300, 2003])
def test_score_integer_operands_exact(hip, N):
    """pins the packing of candidates into row groups (m that divides 64 and m that does not, a candidate's rows across
    two 16-row MFMA blocks), the lane maps of both products, the zero fill of unused rows and the padding edges"""
    rng = np.random.default_rng(31 * N)
    Sigma = rng.integers(-3, 4, size=(N, N)).astype(np.float64)          # asymmetric
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    for m in (1, 2, 3, 5, 8, 17, 64):
        if m > N:
            continue
        for J in _batch_sizes(m):
            H = rng.integers(-2, 3, size=(J, m, N)).astype(np.float64)
            R = rng.integers(-5, 6, size=(J, m, m)).astype(np.float64)
            _, S, flags, _ = d.score(H, R, want_S=True)
            want = _exact_S(Sigma, H, R)
            bad = S != want
            assert not bad.any(), f"N={N} m={m} J={J}: {bad.sum()} wrong elements, first at {np.argwhere(bad)[0]}"
            assert flags.shape == (J,) and set(np.unique(flags)) <= {0, 1}
    d.close()


def test_score_integer_operands_exact_n10003(hip):
    N, m, J = 10003, 2, 1024
    rng = np.random.default_rng(77)
    Sigma = rng.integers(-3, 4, size=(N, N)).astype(np.float64)
    H = rng.integers(-2, 3, size=(J, m, N)).astype(np.float64)
    R = rng.integers(-5, 6, size=(m, m)).astype(np.float64)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    _, S, _, _ = d.score(H, R, want_S=True)
    d.close()
    pick = np.array(sorted(set([0, 1, 31, 32, 33, J - 1] + list(rng.integers(0, J, size=18)))))
    assert np.array_equal(S[pick], _exact_S(Sigma, H[pick], R))


# ---- 5: random SLAM-shaped operands ------------------------------------------------------------------------------------

def _random_sigma(N, rng):
    assert N % 2 == 1   # 3 + 2 n
    _, S, _ = _slam_inputs((N - 3) // 2, rng)
    return S + 1e-3 * np.abs(S) * rng.normal(size=S.shape)      # slightly asymmetric


def _random_candidates(N, J, m, rng):
    H = rng.normal(size=(J, m, N))
    R = 0.01 * np.eye(m) + 1e-3 * rng.normal(size=(J, m, m))    # neither diagonal nor symmetric
    nu = rng.normal(size=(J, m))
    return H, R, nu


@pytest.mark.parametrize("N,m,J", [(43, 1, 64), (43, 2, 33), (403, 2, 200), (403, 7, 10), (403, 16, 5), (2003, 2, 1024),
                                   (2003, 5, 100), (2003, 17, 7), (2003, 64, 3)])
def test_score_random_operands_vs_numpy(hip, N, m, J):
    rng = np.random.default_rng(11 * N + 3 * m + J)
    Sigma = _random_sigma(N, rng)
    H, R, nu = _random_candidates(N, J, m, rng)
    wS, wnis = ds.np_scores(Sigma, H, R, nu)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    nis, S, flags, ms = d.score(H, R, nu, want_S=True)
    d.close()
    assert not flags.any() and ms > 0.0
    eS, en = _rel_blocks(S, wS), float((np.abs(nis - wnis) / np.abs(wnis)).max())
    _note("random_S", eS); _note("random_nis", en)
    assert eS <= FP64_TOL and en <= FP64_TOL, (eS, en)


# ---- 6: the reference --------------------------------------------------------------------------------------------------

def _check_against_reference(hip, case, key):
    state, cov, n = case["state"], case["cov"], int(case["n"])
    d = hip.DensePropagator64(len(state))
    d.set(Sigma=cov)
    d.state = state
    for k, (sx, sy) in enumerate(case["readings"]):
        ref = case["maha"][k]
        assert ds.margins_hold(ref), f"reading {k}: the scenario's seed must be replaced"   # on the REFERENCE's scores
        H, R, nu = ds.candidate_terms(state, sx, sy)
        nis, _, flags, _ = d.score(H, R, nu)                      # every landmark in one call: J = n, m = 2
        assert nis.shape == (n,) and not flags.any()
        rel = float((np.abs(nis - ref) / np.abs(ref)).max())
        _note(key, rel)
        assert rel <= FP64_TOL, (k, rel)
        assert ds.reference_rule(nis) == ds.reference_rule(ref), k
    d.close()


@pytest.mark.parametrize("n", [20, 200])
def test_score_against_the_reference_live(hip, oracle, n):
    """every reading x every landmark, one call per reading, against calculate_maha_dis of the reference's own
    ekf_slam.cpp; the reference's decision rule gives the same winner and gate class on both score sets"""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    _check_against_reference(hip, ds.record_scores(oracle.RefEKF, n, ds.SEEDS[n]), f"reference_live_n{n}")


def test_score_reference_fixture(hip):
    """tests/golden/dense_score_ref.npz: the n = 20 scenario with the reference's recorded scores -- never skips"""
    z = np.load(os.path.join(HERE, "golden", "dense_score_ref.npz"))
    _check_against_reference(hip, {k: z[k] for k in z.files}, "reference_fixture")


# ---- 7: read-only ------------------------------------------------------------------------------------------------------

def test_score_leaves_sigma_and_state(hip):
    N, m, J = 203, 3, 30
    rng = np.random.default_rng(41)
    Sigma = _random_sigma(N, rng)
    x = rng.normal(size=N)
    H, R, nu = _random_candidates(N, J, m, rng)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    d.score(H, R, nu, want_S=True)
    assert np.array_equal(d.sigma, Sigma) and np.array_equal(d.state, x)
    H[4, 1] = 0.0; R[4, 1] = 0.0          # a singular candidate
    H[9, 0, 17] = np.nan                  # and one that is not finite
    _, _, flags, _ = d.score(H, R, nu)
    assert flags[4] == 1 and flags[9] == 1
    assert np.array_equal(d.sigma, Sigma) and np.array_equal(d.state, x)
    d.close()


def test_propagate_and_correct_unchanged_by_scoring_in_between(hip):
    """N large enough that the correction's panels AND the partial S blocks both live in the product buffer"""
    N, m = 3100, 4
    rng = np.random.default_rng(43)
    A = rng.standard_normal((N, 32))
    Sigma = A @ A.T / 32 + np.eye(N)
    F = np.eye(N) + 1e-2 * rng.standard_normal((N, N)) / np.sqrt(N)
    Q = 1e-3 * np.eye(N)
    x = rng.normal(size=N)
    steps = [(rng.normal(size=(m, N)), 0.01 * np.eye(m), rng.normal(size=m)) for _ in range(2)]
    cand = _random_candidates(N, 12, 2, rng)
    out = []
    for with_score in (False, True):
        d = hip.DensePropagator64(N)
        d.set(F, Sigma, Q)
        d.state = x
        res = []
        for H, R, nu in steps:
            if with_score:
                d.score(*cand)
            d.propagate(1)
            if with_score:
                d.score(*cand, want_S=True)
            res.append(d.correct(H, R, nu)[0])
            if with_score:
                d.score(*cand)
        out.append((d.sigma, d.state, res))
        d.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


# ---- 8: consistency with correct ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,m", [(403, 2), (403, 16), (2003, 5), (2003, 64)])
def test_score_agrees_with_correct(hip, N, m):
    rng = np.random.default_rng(5 * N + m)
    Sigma = _random_sigma(N, rng)
    H, R, nu = _random_candidates(N, 1, m, rng)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    nis, _, flags, _ = d.score(H, R, nu)
    nis_c, _ = d.correct(H[0], R[0], nu[0])
    d.close()
    rel = abs(nis[0] - nis_c) / abs(nis_c)
    _note("score_vs_correct_nis", rel)
    assert flags[0] == 0 and rel <= 1e-12, (nis[0], nis_c)


def test_predict_score_correct_cycle(hip):
    """20 steps of predict -> score 12 candidates -> the reference's decision rule -> correct the winner, against the same
    loop in numpy: same decision every step (its margins asserted on numpy's scores), same Sigma and state at the end"""
    N, m, J = 403, 2, 12
    rng = np.random.default_rng(2024)
    F, S, Q = _slam_inputs((N - 3) // 2, rng)
    x = rng.normal(size=N)
    d = hip.DensePropagator64(N)
    d.set(F, S, Q)
    d.state = x
    updates = 0
    for it in range(20):
        d.propagate(1)
        S = F @ S @ F.T + Q
        H = rng.normal(size=(J, m, N))
        R = 0.01 * np.eye(m)
        wS, _ = ds.np_scores(S, H, R)
        # innovations sized so that scores land on both sides of the gates
        nu = np.stack([np.linalg.cholesky((wS[j] + wS[j].T) / 2) @ rng.normal(size=m) for j in range(J)])
        nu *= rng.choice([0.3, 1.0, 3.0], size=(J, 1))
        _, wnis = ds.np_scores(S, H, R, nu)
        assert ds.margins_hold(wnis), f"step {it}: the seed must be replaced"
        nis, gS, flags, _ = d.score(H, R, nu, want_S=True)
        assert not flags.any()
        _note("cycle_S", _rel_blocks(gS, wS)); _note("cycle_nis", float((np.abs(nis - wnis) / np.abs(wnis)).max()))
        assert float((np.abs(nis - wnis) / np.abs(wnis)).max()) <= FP64_TOL
        want = ds.reference_rule(wnis)
        assert ds.reference_rule(nis) == want, it
        if want[1] == "update":
            updates += 1
            w = want[0]
            d.correct(H[w], R, nu[w])
            x, S, _ = dc.np_correct(x, S, H[w], R, nu[w])
    assert updates >= 5
    ec, es = max(cov_err(d.sigma, S).values()), max(state_err(d.state, x).values())
    d.close()
    _note("cycle_cov", ec); _note("cycle_state", es)
    assert ec <= FP64_TOL and es <= FP64_TOL


# ---- 9: singular among good --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,m,J", [(203, 5, 40), (203, 2, 70), (403, 17, 9), (303, 64, 4)])
def test_singular_candidates_among_good_ones(hip, N, m, J):
    rng = np.random.default_rng(N + m)
    Sigma = _random_sigma(N, rng)
    H, R, nu = _random_candidates(N, J, m, rng)
    zero, nan = 1, J - 2
    Hb, Rb = H.copy(), R.copy()
    Hb[zero, m - 1] = 0.0; Rb[zero, m - 1] = 0.0       # a zero row of H with a zero row of R: S has a zero row
    Hb[nan, 0, N // 2] = np.nan
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    nis0, S0, f0, _ = d.score(H, R, nu, want_S=True)
    nis1, S1, f1, _ = d.score(Hb, Rb, nu, want_S=True)   # returns: the call is EKF_OK
    d.close()
    good = np.ones(J, dtype=bool)
    good[[zero, nan]] = False
    assert not f0.any() and f1[zero] == 1 and f1[nan] == 1 and not f1[good].any()
    assert np.isnan(nis1[zero]) and np.isnan(nis1[nan])
    assert np.array_equal(nis0[good], nis1[good]) and np.array_equal(S0[good], S1[good])


# ---- 10: position independence and determinism -------------------------------------------------------------------------

@pytest.mark.parametrize("N,m", [(303, 1), (303, 2), (403, 5), (403, 17), (2003, 2), (2003, 64)])
def test_position_independence_and_determinism(hip, N, m):
    rng = np.random.default_rng(9 * N + m)
    Sigma = _random_sigma(N, rng)
    J = min(3 * (64 // m) + 2, MAX_ROWS // m)
    H, R, nu = _random_candidates(N, J, m, rng)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    nis, S, _, _ = d.score(H, R, nu, want_S=True)
    nis2, S2, _, _ = d.score(H, R, nu, want_S=True)
    assert np.array_equal(nis, nis2) and np.array_equal(S, S2)                       # the same call twice
    for j in (0, J // 2, J - 1):                                                     # alone
        a, b, _, _ = d.score(H[j:j + 1], R[j:j + 1], nu[j:j + 1], want_S=True)
        assert a[0] == nis[j] and np.array_equal(b[0], S[j]), j
    perm = rng.permutation(J)                                                        # shuffled: first, last, anywhere
    a, b, _, _ = d.score(H[perm], R[perm], nu[perm], want_S=True)
    assert np.array_equal(a, nis[perm]) and np.array_equal(b, S[perm])
    a, b, _, _ = d.score(H[perm][:J // 3], R[perm][:J // 3], nu[perm][:J // 3], want_S=True)   # another batch size
    assert np.array_equal(a, nis[perm][:J // 3]) and np.array_equal(b, S[perm][:J // 3])
    Rs = R[0]                                                                        # shared R against R replicated
    a, b, _, _ = d.score(H, Rs, nu, want_S=True)
    a2, b2, _, _ = d.score(H, np.stack([Rs] * J), nu, want_S=True)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    d.close()


# ---- 11: full size -----------------------------------------------------------------------------------------------------

def test_score_full_size_n10003(hip):
    N = 10003
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    Sigma = A @ A.T / 64 + np.eye(N)
    Sigma += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))   # asymmetric
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    for m, J in ((2, 1024), (64, 32)):
        H, R, nu = _random_candidates(N, J, m, rng)
        nis, S, flags, ms = d.score(H, R, nu, want_S=True)
        assert not flags.any()
        pick = np.array(sorted(set([0, J - 1] + list(rng.integers(0, J, size=6)))))
        wS, wnis = ds.np_scores(Sigma, H[pick], R[pick], nu[pick])
        eS, en = _rel_blocks(S[pick], wS), float((np.abs(nis[pick] - wnis) / np.abs(wnis)).max())
        _note(f"full_size_m{m}_S", eS); _note(f"full_size_m{m}_nis", en)
        print(f"N={N} m={m} J={J}: {ms:.3f} ms")
        assert eS <= FP64_TOL and en <= FP64_TOL, (m, eS, en)
    d.close()


def test_zz_report():
    for k in sorted(WORST):
        print(f"dense64 score worst {k}: {WORST[k]:.3e}")
    assert all(v <= FP64_TOL for v in WORST.values())
