"""Shared by tests/test_gpu_dense64_block.py, tests/test_dense64_block_host.py and
tests/golden/make_dense_predict_golden.py: the block-structured prediction in numpy (the reference's literal spelling,
ekf_slam.cpp:99-102, and the three slice updates it amounts to), the operands of the reference's own motion model
(:76-96) built from a state snapshot, and the scenario a RefEKF-like object is driven through."""
import math

import numpy as np

Q_POSE = 1e-4   # the reference's process noise on the pose block


def embed(N, first, Fr, Qr=None):
    """-> F = identity with Fr in [first, first + r)^2, Q = zero with Qr in the same square"""
    r = len(Fr)
    F, Q = np.eye(N), np.zeros((N, N))
    F[first:first + r, first:first + r] = Fr
    if Qr is not None:
        Q[first:first + r, first:first + r] = Qr
    return F, Q


def np_predict_literal(state, Sigma, first, Fr, Qr=None, dx=None):
    """-> state', Sigma' with the reference's expressions: state + update; At*sigma*At.t() + Q (dense N x N operands)"""
    F, Q = embed(len(state), first, Fr, Qr)
    upd = np.zeros(len(state))
    if dx is not None:
        upd[first:first + len(Fr)] = dx
    return state + upd, F @ Sigma @ F.T + Q


def np_predict_slices(state, Sigma, first, Fr, Qr=None, dx=None):
    """The same as three slice updates (what the call is specified to do); nothing else is touched.  Works on copies."""
    r = len(Fr)
    b = slice(first, first + r)
    S = Sigma.copy()
    rows, cols, corner = Fr @ Sigma[b, :], Sigma[:, b] @ Fr.T, (Fr @ Sigma[b, b]) @ Fr.T
    S[b, :] = rows
    S[:, b] = cols
    S[b, b] = corner if Qr is None else corner + Qr
    s = state.copy()
    if dx is not None:
        s[b] = s[b] + dx
    return s, S


def model_operands(state, dtheta, dx):
    """Fr (3 x 3 = the pose block of At), Qr, update of the reference's motion model for the twist (dtheta, dx): both
    branches of ekf_slam.cpp:79"""
    th = float(state[0])
    Fr, upd = np.eye(3), np.zeros(3)
    if abs(dtheta) < 0.000001:
        upd[1], upd[2] = dx * math.cos(th), dx * math.sin(th)
        Fr[1, 0] += -dx * math.sin(th)
        Fr[2, 0] += dx * math.cos(th)
    else:
        q = dx / dtheta
        upd[0] = dtheta
        upd[1] = -q * math.sin(th) + q * math.sin(th + dtheta)
        upd[2] = q * math.cos(th) - q * math.cos(th + dtheta)
        Fr[1, 0] += -q * math.cos(th) + q * math.cos(th + dtheta)
        Fr[2, 0] += -q * math.sin(th) + q * math.sin(th + dtheta)
    return Fr, np.eye(3) * Q_POSE, upd


def unsymmetric_cov(N, rng, rel=1e-3):
    """random symmetric positive-definite Sigma with unsymmetric noise of relative size `rel` on top, so that rows and
    columns differ and a swapped Sigma[b, :] / Sigma[:, b] cannot pass"""
    A = rng.normal(size=(N, N))
    S = A @ A.T / N + np.eye(N)
    return S + rel * np.abs(S) * rng.normal(size=(N, N))


def replay_case(case, predict):
    """The recorded prediction() calls, one predict(state, Sigma, first, Fr, Qr, dx) -> (state', Sigma') per twist"""
    state, Sigma = np.array(case["state0"], dtype=np.float64), np.array(case["cov0"], dtype=np.float64)
    for dth, dx in np.asarray(case["twists"], dtype=np.float64).reshape(-1, 2):
        Fr, Qr, upd = model_operands(state, float(dth), float(dx))
        state, Sigma = predict(state, Sigma, 0, Fr, Qr, upd)
    return state, Sigma


def record_case(Ref, n, twists, seed):
    """Give the reference a random state and an unsymmetric covariance, run prediction() once per twist, record both ends."""
    rng = np.random.default_rng(seed)
    N = 3 + 2 * n
    r = Ref(n)
    state0 = rng.normal(size=N)
    cov0 = unsymmetric_cov(N, rng)
    r.state, r.cov = state0, cov0
    for dth, dx in twists:
        r.prediction(dth, dx)
    return {"n": n, "state0": state0, "cov0": cov0, "twists": np.array(twists, dtype=np.float64),
            "state1": r.state, "cov1": r.cov}


# name, twists (dtheta, dx), seed offset: one call per branch of :79, then five in a row (both branches among them)
CASES = [("straight", [(2e-7, 0.07)], 31),
         ("turn", [(0.05, 0.02)], 32),
         ("five", [(0.2, 0.1), (-0.15, 0.08), (0.0, 0.05), (0.3, -0.04), (0.011, 0.12)], 33)]
