"""-m gpu: ekf_dense64_solve and ekf_dense64_color (k_ds_back, k_dc_color of ekf_dense64_factor.hip) against
dense_solve_cases.  Sizes around the block side NB the library reports: Na in {1, 2, 3, NB - 1, NB, NB + 1, 2 NB + 1,
3 NB + 2}, each once with N = Na and once with N = Na + 5, live = Na and everything outside the corner (Sigma and the state)
poisoned with payload NaNs; 1, 3 and 64 right-hand sides.  1. the integer family, exact; 2. unit vectors: the columns of
get_factor(); 3. the derived componentwise bounds on slam_like; 4. position independence and repetition; 5. add_state and
pending rows; 6. refusals; 7. DenseEKFSLAM.sample_maps / map_solve."""
import ctypes

import numpy as np
import pytest

import dense_init_cases as ic
import dense_solve_cases as sc
from dense_factor_cases import integer_indefinite
from test_gpu_dense64_live import _poison

pytestmark = pytest.mark.gpu
_NB = []
_REF = {}     # (family, Na) -> arrays computed once, never changed
STATE_ERR = 5   # EKF_ERR_STATE


def _nb(hip):
    if not _NB:
        d = hip.DensePropagator64(3)
        info, finfo = d.solve_launch_info(), d.factor_launch_info()
        d.close()
        assert info["block"] == finfo["block"] and info["threads_back"] >= 64 and info["threads_color"] >= 64
        _NB.append(info["block"])
    return _NB[0]


def _integer(Na):
    if ("int", Na) not in _REF:
        C, L0 = sc.integer_factor(Na)
        for a in (C, L0):
            a.setflags(write=False)
        _REF["int", Na] = (C, L0)
    return _REF["int", Na]


def _slam(Na):
    if ("slam", Na) not in _REF:
        A, given = sc.slam_like(Na), sc.slam_like_input(Na)
        for a in (A, given):
            a.setflags(write=False)
        _REF["slam", Na] = (A, given)
    return _REF["slam", Na]


def _handle(hip, corner, tail, x=None):
    """a handle of dimension Na + tail that holds `corner` in its live corner Na, factored; with a tail everything else,
    the state beyond Na included, is poison"""
    Na = corner.shape[0]
    N = Na + tail
    x = np.arange(1.0, Na + 1.0) if x is None else x
    S, xs = _poison(N, Na, corner, x) if tail else (np.array(corner), np.array(x))
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = xs
    d.live = Na
    assert d.factor()["ok"] == 1
    return d, S, xs


def _refused(hip, call):
    with pytest.raises(hip.EkfError) as e:
        call()
    return e.value.status


SIZE_IDS = ["1", "2", "3", "NB-1", "NB", "NB+1", "2NB+1", "3NB+2"]
CASES = [(k, tail) for k in range(len(SIZE_IDS)) for tail in (0, 5)]
CASE_IDS = [f"{SIZE_IDS[k]}-{'tail' if tail else 'full'}" for k, tail in CASES]


# ---- 1. the integer family ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_integer_family_exact(hip, k, tail):
    Na = sc.sizes(_nb(hip))[k]
    C, L0 = _integer(Na)
    d, _, _ = _handle(hip, C, tail)
    for nrhs in (1, 3, 64):
        X0 = np.random.default_rng(100 * Na + nrhs).integers(-3, 4, size=(nrhs, Na)).astype(np.float64)
        B = X0 @ C
        white = d.whiten(B)
        got = d.solve(B, want_Y=True)
        assert sc.same_up_to_zero_sign(got["X"], X0), nrhs
        assert sc.same_bits(got["Y"], white["Y"]) and sc.same_bits(got["d2"], white["d2"]), nrhs
        assert sc.same_up_to_zero_sign(got["Y"], X0 @ L0)
        only = d.solve(B)
        assert only["Y"] is None and sc.same_bits(only["X"], got["X"]) and sc.same_bits(only["d2"], got["d2"])
        assert sc.same_up_to_zero_sign(d.color(X0)["X"], X0 @ L0.T), nrhs
        assert sc.same_up_to_zero_sign(d.color(white["Y"])["X"], B), nrhs
    d.close()


# ---- 2. unit vectors ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_color_of_unit_vectors_is_the_factor(hip, k, tail):
    NB = _nb(hip)
    Na = sc.sizes(NB)[k]
    d, _, _ = _handle(hip, _slam(Na)[1], tail)
    L = d.get_factor()
    starts = sorted({0, max(0, min(NB - 1, Na - 1) - 63), min(NB, Na - 1), max(0, Na - 64)})
    seen = set()
    for c0 in starts:                                            # 64 rows of the identity at a time
        cols = np.arange(c0, min(Na, c0 + 64))
        E = np.zeros((cols.size, Na))
        E[np.arange(cols.size), cols] = 1.0
        X = d.color(E)["X"]
        assert sc.same_up_to_zero_sign(X, L[:, cols].T), c0
        assert not np.isnan(X).any()                             # nothing from above the diagonal, nothing from the tail
        seen.update(int(c) for c in cols)
    d.close()
    assert {0, min(NB - 1, Na - 1), min(NB, Na - 1), Na - 1} <= seen


# ---- 3. the derived bounds ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_slam_like_componentwise_bounds(hip, k, tail):
    Na = sc.sizes(_nb(hip))[k]
    A, given = _slam(Na)
    rng = np.random.default_rng(31 + Na)
    state = rng.standard_normal(Na)
    d, _, _ = _handle(hip, given, tail, x=state)                 # garbage above the diagonal
    L = d.get_factor()
    B, Z = rng.standard_normal((64, Na)), rng.standard_normal((64, Na))
    got = d.solve(B, want_Y=True)
    plain, shifted = d.color(Z)["X"], d.color(Z, add_state=True)["X"]
    d.close()
    rows = range(0, 64, 7)
    back = max(sc.back_residual_ratio(L, got["X"][r], got["Y"][r]) for r in rows)
    col = max(sc.color_residual_ratio(L, plain[r], Z[r]) for r in rows)
    cols = max(sc.color_residual_ratio(L, shifted[r], Z[r], state) for r in rows)
    whole = max(sc.solve_residual_ratio(A, L, got["X"][r], B[r]) for r in rows)
    print(f"Na={Na} tail={tail}: of their bounds: backward {back:.3f}, colour {col:.3f}, with the state {cols:.3f}, "
          f"Sigma x - b {whole:.4f}")
    assert back <= 1.0 and col <= 1.0 and cols <= 1.0 and whole <= 1.0
    assert sc.same_bits(shifted, plain + state)                  # fl(sum + state), the addition last


# ---- 4. position independence, repetition ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 5, 7], ids=["NB-1", "NB+1", "3NB+2"])
def test_position_independence_and_repetition(hip, k):
    Na = sc.sizes(_nb(hip))[k]
    d, _, _ = _handle(hip, _slam(Na)[1], 5, x=np.linspace(-1.0, 1.0, Na))
    V = np.random.default_rng(77 + Na).standard_normal((64, Na))
    for call in (lambda M: d.solve(M)["X"], lambda M: d.color(M)["X"], lambda M: d.color(M, add_state=True)["X"]):
        full = call(V)
        assert sc.same_bits(call(V), full)                       # a second run
        alone = call(V[17])
        first = call(np.vstack([V[17], V[1], V[2]]))
        moved = V.copy()
        moved[63] = V[17]
        last = call(moved)
        assert sc.same_bits(alone[0], full[17]) and sc.same_bits(first[0], full[17]) and sc.same_bits(last[63], full[17])
        assert sc.same_bits(first[1:], full[1:3]) and sc.same_bits(last[:63], full[:63])
    d.close()


# ---- 5. add_state, pending rows -------------------------------------------------------------------------------------------

def test_pending_rows_stay_and_the_snapshot_is_used_as_taken(hip):
    Na = _nb(hip) + 1
    A = _slam(Na)[0]
    x0 = np.linspace(-1.0, 1.0, Na)
    d, _, _ = _handle(hip, A, 5, x=x0)
    twin, _, _ = _handle(hip, A, 5, x=x0)
    V = np.random.default_rng(5).standard_normal((3, Na))
    before = (d.solve(V, want_Y=True), d.color(V)["X"])
    rng = np.random.default_rng(17)
    for j in (1, Na // 2 - 3):
        cols = np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j])
        args = (cols, rng.standard_normal((2, 5)), 0.5 * np.eye(2), 0.1 * rng.standard_normal(2))
        d.correct_sparse_deferred(*args)
        twin.correct_sparse_deferred(*args)
    assert d.pending == 4
    after = d.solve(V, want_Y=True)
    assert d.pending == 4
    plain, shifted = d.color(V)["X"], d.color(V, add_state=True)["X"]
    assert d.pending == 4
    state = d.state_block(0, Na)
    assert d.pending == 4 and not sc.same_bits(state, x0)       # the corrections moved the state: the current one is added
    assert all(sc.same_bits(after[key], before[0][key]) for key in ("X", "Y", "d2")) and sc.same_bits(plain, before[1])
    assert sc.same_bits(shifted, plain + state)
    same = sc.same_bits(d.sigma, twin.sigma) and sc.same_bits(d.state, twin.state)   # (reading Sigma flushes both)
    d.close(); twin.close()
    assert same


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------

def test_refusals(hip):
    Na = 5
    C, _ = _integer(Na)
    d = hip.DensePropagator64(Na)
    d.set(Sigma=np.array(C))
    lib, buf = hip.load(), np.full(64 * Na, 7.0)
    untouched = buf.copy()
    a, b, c = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    solve, color = lib.ekf_dense64_solve, lib.ekf_dense64_color
    assert lib.ekf_dense64_solve_launch_info(d._h, None, ctypes.byref(b), ctypes.byref(c)) == 1
    assert lib.ekf_dense64_solve_launch_info(d._h, ctypes.byref(a), None, ctypes.byref(c)) == 1
    assert lib.ekf_dense64_solve_launch_info(d._h, ctypes.byref(a), ctypes.byref(b), None) == 1
    assert (a.value, b.value, c.value) == (7, 7, 7)

    def order():
        """the argument refusals, each reached with everything behind it wrong as well"""
        assert solve(None, 0, None, None, None, None, None) == 1 and b"null handle" in lib.ekf_last_error()
        assert solve(d._h, 0, None, None, None, None, None) == 1 and b"null B" in lib.ekf_last_error()
        assert solve(d._h, 0, p, None, None, None, None) == 1 and b"nrhs" in lib.ekf_last_error()
        assert solve(d._h, 65, p, None, None, None, None) == 1 and b"nrhs" in lib.ekf_last_error()
        assert solve(d._h, 1, p, None, None, None, None) == 1 and b"all NULL" in lib.ekf_last_error()
        assert color(None, 0, None, 0, None, None) == 1 and b"null handle" in lib.ekf_last_error()
        assert color(d._h, 0, None, 0, None, None) == 1 and b"null Z" in lib.ekf_last_error()
        assert color(d._h, 0, p, 0, None, None) == 1 and b"nrhs" in lib.ekf_last_error()
        assert color(d._h, 65, p, 0, None, None) == 1 and b"nrhs" in lib.ekf_last_error()
        assert color(d._h, 1, p, 0, None, None) == 1 and b"null X_out" in lib.ekf_last_error()

    def state_refused():
        assert solve(d._h, 1, p, p, p, p, None) == STATE_ERR and color(d._h, 1, p, 1, p, None) == STATE_ERR
        assert np.array_equal(buf, untouched)

    order()                                                      # INVALID comes before STATE
    state_refused()                                              # before any factor
    assert d.factor()["ok"] == 1
    order()
    assert solve(d._h, 1, p, p, p, p, None) == 0 and not np.array_equal(buf, untouched)
    buf[:] = untouched
    d.set(Sigma=integer_indefinite(Na, Na - 1, 3)[0])
    assert d.factor()["ok"] == 0
    state_refused()                                              # after a factor with ok = 0
    d.close()

    d, _, _ = _handle(hip, C, 5)
    d.live = Na - 2
    state_refused()                                              # the snapshot's Na is not the live dimension
    assert _refused(hip, lambda: d.solve(np.ones(Na - 2))) == STATE_ERR
    assert _refused(hip, lambda: d.color(np.ones(Na - 2))) == STATE_ERR
    d.live = Na
    assert sc.same_up_to_zero_sign(d.solve(np.ones(Na) @ C)["X"][0], np.ones(Na))
    for call in (lambda: d.solve(np.ones(Na - 1)), lambda: d.color(np.ones((65, Na))), lambda: d.color(np.ones((2, 2, Na)))):
        with pytest.raises(ValueError):
            call()
    d.close()


# ---- 7. DenseEKFSLAM ------------------------------------------------------------------------------------------------------

def test_sample_maps_and_map_solve(hip):
    """A 2-landmark map.  sample_maps with Z given is color(Z, add_state=True) bit for bit.  With 64 seeded draws every
    sample is within 2 gamma_{Na+1} (|Z| |L|^T + |state|) of numpy's state + Z @ L.T on the returned factor (each side is
    within gamma_{Na+1} of the exact value), and the sample mean and covariance are within what that perturbation E of the
    samples can do to them -- |mean(E)| and (|Wc|^T |Ec| + |Ec|^T |Wc| + |Ec|^T |Ec|) / (k - 1) -- plus numpy's own rounding in
    forming the two means (gamma_k) and the two covariances (gamma_{2k+4}, doubled): no statistical threshold.  map_solve(e) @ e
    is map_nees within 4 Na 2^-53 of it."""
    n, k = 2, 64
    f = hip.DenseEKFSLAM(n)
    for dth, dx, readings in ic.discovery_scenario(steps=n):
        f.prediction(dth, dx)
        f.data_association(readings)
    Na = 3 + 2 * n
    rep = f.factor()
    assert rep["ok"] == 1 and rep["Na"] == Na
    L, state = f.handle.get_factor(), f.state
    Z = np.random.default_rng(3).standard_normal((k, Na))
    X = f.sample_maps(k, rng=np.random.default_rng(3))
    assert X.shape == (k, Na) and sc.same_bits(X, f.sample_maps(k, Z=Z))
    assert sc.same_bits(X, f.handle.color(Z, add_state=True)["X"])
    assert sc.same_bits(f.sample_maps(3, Z=Z[5:8]), X[5:8])
    assert f.sample_maps(2).shape == (2, Na) and f.handle.pending == 0
    W = state + Z @ L.T
    E = 2 * sc.gamma(Na + 1) * (np.abs(Z) @ np.abs(L).T + np.abs(state))
    assert (np.abs(X - W) <= E).all()
    mean_bound = E.mean(axis=0) + 2 * sc.gamma(k) * np.abs(W).mean(axis=0)
    Wc, Ec = np.abs(W - W.mean(axis=0)), E + E.mean(axis=0)
    cov_bound = (Wc.T @ Ec + Ec.T @ Wc + Ec.T @ Ec) / (k - 1) + 2 * sc.gamma(2 * k + 4) * (Wc.T @ Wc) / (k - 1)
    dm, dc = np.abs(X.mean(axis=0) - W.mean(axis=0)), np.abs(np.cov(X, rowvar=False) - np.cov(W, rowvar=False))
    print(f"sample mean off by {dm.max():.2e} (bound {mean_bound.min():.2e}), covariance by {dc.max():.2e} (bound {cov_bound.min():.2e})")
    assert (dm <= mean_bound).all() and (dc <= cov_bound).all()

    truth = state + np.random.default_rng(4).normal(0.0, 0.05, size=Na)
    truth[0] = state[0] - 3.5                                    # a heading difference beyond pi: it has to be wrapped
    e = state - truth
    e[0] = hip.normalize_angles(e[:1])[0]
    nees = f.map_nees(truth)
    x = f.map_solve(truth=truth)
    assert sc.same_bits(x, f.map_solve(e)) and sc.same_bits(x, f.handle.solve(e)["X"][0])
    Sigma = f.handle.sigma[:Na, :Na]
    f.close()
    rel = abs(float(x @ e) - nees) / nees
    print(f"map_solve(e) @ e = {float(x @ e)!r}, map_nees = {nees!r}: relative difference {rel:.2e} of {4 * Na * sc.U:.2e}")
    assert rel <= 4 * Na * sc.U
    Sl = np.tril(Sigma) + np.tril(Sigma, -1).T
    assert sc.solve_residual_ratio(Sl, L, x, e) <= 1.0
