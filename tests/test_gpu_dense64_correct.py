"""-m gpu: the fp64 dense measurement update for a general m x N Jacobian (ekf_dense64_correct,
ekf_dense64_correct.hip) -- the reference's literal correction (ekf_slam.cpp:178,186,191-192) for arbitrary operands:
integer operands bit-exact against `(eye - K H) Sigma`, random operands within FP64_TOL per block of numpy fp64, the
reference's own measurement() (live through oracle.RefEKF, and replayed from tests/golden/dense_correct_ref.npz) within
FP64_TOL, predict / correct cycles, the singular-S status, run-to-run determinism, N = 10003.

Worst values seen on the MI355X (printed by test_zz_report): random operands 2.4e-15 per covariance block
(state 1.6e-16, nis 4.8e-16 relative); the reference live and its fixture 5.4e-16 per block, nis 1.1e-13 relative (numpy's
literal spelling is at the same 1.1e-13 from calculate_maha_dis on that case); 20 predict / correct cycles 6.0e-15;
N = 10003 sampled rows / columns / state / nis 9.2e-16 (m = 2), 6.8e-16 (m = 64)."""
import importlib.util
import os

import numpy as np
import pytest

import dense_correct_cases as dc
from parity import FP64_TOL, cov_err, state_err, worst

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {v:.3e}")


def _slam_inputs(n, rng):
    spec = importlib.util.spec_from_file_location("dense64_bench", os.path.join(os.path.dirname(HERE), "tools",
                                                                                "dense64_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.slam_inputs(n, rng)


def _exact_operands(N, m, rng):
    """Integer Sigma (asymmetric), H, nu, state and R = D - H Sigma H^T with D = diag(2^k): S = D exactly, and S^-1, K,
    K nu, K T and the difference are exact dyadic rationals far inside 53 bits -- every order of summation gives the
    same bits."""
    Sigma = rng.integers(-3, 4, size=(N, N)).astype(np.float64)
    H = rng.integers(-2, 3, size=(m, N)).astype(np.float64)
    nu = rng.integers(-4, 5, size=m).astype(np.float64)
    x = rng.integers(-9, 10, size=N).astype(np.float64)
    D = np.diag(2.0 ** rng.integers(1, 5, size=m))
    R = D - H @ Sigma @ H.T
    return Sigma, H, R, nu, x, D


PAIRS = [(N, m) for N in (1, 2, 43, 128, 129, 300) for m in (1, 2, 3, 5, 8, 64) if m <= N]


@pytest.mark.parametrize("N,m", PAIRS)
def test_correct_operand_layouts_exact(hip, N, m):
    """pins row- vs column-gather (T vs U differ: Sigma is asymmetric), the MFMA lane maps, the zero fill of k up to 4
    and the padding edges"""
    rng = np.random.default_rng(1000 * N + m)
    Sigma, H, R, nu, x, D = _exact_operands(N, m, rng)
    K = Sigma @ H.T @ np.linalg.inv(D)
    want = (np.eye(N) - K @ H) @ Sigma      # the reference's spelling
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    nis, _ = d.correct(H, R, nu)
    got, gx = d.sigma, d.state
    d.close()
    assert np.array_equal(gx, x + K @ nu)
    bad = got != want
    assert not bad.any(), f"{bad.sum()} wrong elements, first at {np.argwhere(bad)[0]}"
    assert nis == float(nu @ np.linalg.inv(D) @ nu)


def _random_case(N, m, rng):
    _, S, _ = _slam_inputs((N - 3) // 2, rng)
    S = S + 1e-3 * np.abs(S) * rng.normal(size=S.shape)      # slightly asymmetric
    H = rng.normal(size=(m, N))
    R = 0.01 * np.eye(m) + 1e-3 * rng.normal(size=(m, m))     # neither diagonal nor symmetric
    nu = rng.normal(size=m)
    x = rng.normal(size=N)
    return S, H, R, nu, x


@pytest.mark.parametrize("N,m", [(N, m) for N in (43, 403, 2003) for m in (1, 2, 7, 16, 64) if m <= N])
def test_correct_random_operands_vs_numpy(hip, N, m):
    rng = np.random.default_rng(7 * N + m)
    S, H, R, nu, x = _random_case(N, m, rng)
    wx, wS, wnis = dc.np_correct(x, S, H, R, nu)
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = x
    nis, _ = d.correct(H, R, nu)
    ec, es = max(cov_err(d.sigma, wS).values()), max(state_err(d.state, wx).values())
    d.close()
    en = abs(nis - wnis) / abs(wnis)
    _note("random_cov", ec); _note("random_state", es); _note("random_nis", en)
    assert ec <= FP64_TOL and es <= FP64_TOL and en <= FP64_TOL, (ec, es, en)


# ---- the reference itself ----------------------------------------------------------------------------------------------

def _gpu_correct(hip, N):
    d = hip.DensePropagator64(N)

    def correct(state, Sigma, H, R, nu):
        d.set(Sigma=Sigma)
        d.state = state
        nis, _ = d.correct(H, R, nu)
        return d.state, d.sigma, nis
    return d, correct


def _check_case(hip, case, key):
    d, correct = _gpu_correct(hip, len(case["state0"]))
    s, c, nis = dc.replay_case(case, correct)
    d.close()
    w, e = worst(s, c, case["state1"], case["cov1"])
    rel = abs(nis - float(case["maha"])) / abs(float(case["maha"]))
    _note(key, w); _note(key + "_nis", rel)
    assert w <= FP64_TOL, e
    assert rel <= FP64_TOL, (nis, float(case["maha"]))


@pytest.mark.parametrize("n", [20, 200])
@pytest.mark.parametrize("name,nvis,off", dc.CASES)
def test_correct_against_the_reference(hip, oracle, n, name, nvis, off):
    """measurement() of the reference's own ekf_slam.cpp with one visible landmark IS one dense correction with m = 2;
    with three, three of them (pose terms from the pose captured before the call, landmark terms from the current state)"""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    _check_case(hip, dc.record_case(oracle.RefEKF, n, nvis, n + off), f"reference_live_{name}")


@pytest.mark.parametrize("name", [c[0] for c in dc.CASES])
def test_correct_reference_fixture_replayed(hip, name):
    """tests/golden/dense_correct_ref.npz: the same cases at n = 20 with the reference's recorded outputs -- never skips"""
    z = np.load(os.path.join(HERE, "golden", "dense_correct_ref.npz"))
    case = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    assert int(case["vis"].sum()) == dict((c[0], c[1]) for c in dc.CASES)[name]
    _check_case(hip, case, f"reference_fixture_{name}")


# ---- the handle --------------------------------------------------------------------------------------------------------

def test_predict_correct_cycle(hip):
    N, m = 403, 4
    rng = np.random.default_rng(99)
    F, S, Q = _slam_inputs((N - 3) // 2, rng)
    x = rng.normal(size=N)
    d = hip.DensePropagator64(N)
    d.set(F, S, Q)
    d.state = x
    for it in range(20):
        d.propagate(1)
        S = F @ S @ F.T + Q
        H = rng.normal(size=(m, N))
        R = 0.01 * np.eye(m)
        nu = rng.normal(size=m)
        nis, _ = d.correct(H, R, nu)
        x, S, wnis = dc.np_correct(x, S, H, R, nu)
        assert abs(nis - wnis) <= FP64_TOL * abs(wnis)
    ec, es = max(cov_err(d.sigma, S).values()), max(state_err(d.state, x).values())
    _note("cycle_cov", ec); _note("cycle_state", es)
    assert ec <= FP64_TOL and es <= FP64_TOL
    # the padding of Sigma is still zero: I Sigma I^T + 0 returns Sigma bit for bit
    before = d.sigma
    d.set(F=np.eye(N), Q=np.zeros((N, N)))
    d.propagate(1)
    assert np.array_equal(d.sigma, before)
    d.close()


@pytest.mark.parametrize("why", ["zero_row", "nan"])
def test_correct_singular_S_leaves_everything(hip, why):
    N, m = 203, 5
    rng = np.random.default_rng(17)
    S, H, R, nu, x = _random_case(N, m, rng)
    if why == "zero_row":
        H[2] = 0.0
        R = np.zeros((m, m))
    else:
        H[1, 77] = np.nan
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = x
    with pytest.raises(hip.EkfError) as e:
        d.correct(H, R, nu)
    assert e.value.status == 5                                 # EKF_ERR_STATE
    assert np.array_equal(d.sigma, S) and np.array_equal(d.state, x)
    # the handle works afterwards
    S2, H2, R2, nu2, _ = _random_case(N, m, rng)
    wx, wS, wnis = dc.np_correct(x, S, H2, R2, nu2)
    nis, _ = d.correct(H2, R2, nu2)
    assert max(cov_err(d.sigma, wS).values()) <= FP64_TOL and max(state_err(d.state, wx).values()) <= FP64_TOL
    assert abs(nis - wnis) <= FP64_TOL * abs(wnis)
    d.close()


def test_correct_argument_checks(hip):
    N = 30
    d = hip.DensePropagator64(N)
    assert not d.state.any()                                    # a new handle's state is zero
    H, R, nu = np.ones((2, N)), np.eye(2), np.ones(2)
    for bad in (lambda: d.correct(np.ones((2, N + 1)), R, nu), lambda: d.correct(np.ones((0, N)), np.eye(0)),
                lambda: d.correct(np.ones((N + 1, N)), np.eye(N + 1)), lambda: d.correct(H, np.eye(3), nu),
                lambda: d.correct(H, R, np.ones(3)), lambda: setattr(d, "state", np.zeros(N + 1))):
        with pytest.raises(ValueError):
            bad()
    d.set(Sigma=np.eye(N))
    nis, ms = d.correct(H, R)                                   # no innovation: the state stays, no score
    assert nis is None and ms > 0.0 and not d.state.any()
    d.close()


def test_correct_is_deterministic(hip):
    N, m = 2003, 16
    rng = np.random.default_rng(5)
    S, H, R, nu, x = _random_case(N, m, rng)
    d = hip.DensePropagator64(N)
    out = []
    for _ in range(2):
        d.set(Sigma=S)
        d.state = x
        nis, _ = d.correct(H, R, nu)
        out.append((d.sigma, d.state, nis))
    d.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_correct_full_size_n10003(hip):
    N = 10003
    rng = np.random.default_rng(8)
    last = (N - 1) // 128 * 128                                  # first row of the last 128-row block
    rows = np.array(sorted(set([0, 2, N - 1] + list(range(last, N, 3)) + list(rng.integers(0, N, size=18)))))
    cols = np.array(sorted(set([0, 1, N - 1, N - 2] + list(rng.integers(0, N, size=12)))))
    assert len(rows) >= 24 and (rows >= last).sum() >= 4
    d = hip.DensePropagator64(N)
    Sigma = rng.integers(-3, 4, size=(N, N)).astype(np.float64)
    for m in (2, 64):
        H = rng.integers(-2, 3, size=(m, N)).astype(np.float64)
        nu = rng.integers(-4, 5, size=m).astype(np.float64)
        x = rng.integers(-9, 10, size=N).astype(np.float64)
        Dinv = np.diag(2.0 ** -rng.integers(1, 5, size=m).astype(np.float64))
        T = H @ Sigma
        R = np.linalg.inv(Dinv) - T @ H.T
        K = (Sigma @ H.T) @ Dinv
        d.set(Sigma=Sigma)
        d.state = x
        nis, _ = d.correct(H, R, nu)
        got = d.sigma
        assert np.array_equal(got[rows], Sigma[rows] - K[rows] @ T), m
        assert np.array_equal(got[:, cols], Sigma[:, cols] - K @ T[:, cols]), m
        assert np.array_equal(d.state, x + K @ nu) and nis == float(nu @ Dinv @ nu)
    del Sigma, got
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    S += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))   # asymmetric
    for m in (2, 64):
        H = rng.standard_normal((m, N))
        R = 0.01 * np.eye(m) + 1e-3 * rng.standard_normal((m, m))
        nu = rng.standard_normal(m)
        x = rng.standard_normal(N)
        T = H @ S
        Si = np.linalg.inv(T @ H.T + R)
        K = (S @ H.T) @ Si
        d.set(Sigma=S)
        d.state = x
        nis, _ = d.correct(H, R, nu)
        got = d.sigma
        wr, wc = S[rows] - K[rows] @ T, S[:, cols] - K @ T[:, cols]
        er = np.abs(got[rows] - wr).max() / np.abs(wr).max()
        ecl = np.abs(got[:, cols] - wc).max() / np.abs(wc).max()
        wx = x + K @ nu
        es = np.abs(d.state - wx).max() / np.abs(wx).max()
        en = abs(nis - float(nu @ Si @ nu)) / abs(float(nu @ Si @ nu))
        _note(f"full_size_m{m}", max(er, ecl, es, en))
        assert max(er, ecl, es, en) <= FP64_TOL, (m, er, ecl, es, en)
    d.close()


def test_zz_report():
    for k in sorted(WORST):
        print(f"dense64 correct worst {k}: {WORST[k]:.3e}")
    assert all(v <= FP64_TOL for v in WORST.values())
