"""-m gpu: the dense fp64 handle over whole map lifetimes against ONE fp64 model (tests/dense_session_cases.py): the named
sessions grow_prune, grow_prune_high, policy_flips, capacity, dense_between and edges_walk at N in {67, 131, 203}, with the
carry policy on and off at the start, and two handles interleaved on one device.  Integer sessions: after EVERY call the
status, the pending count, live, the whole state, a score_sparse probe (S and nis through whatever is pending), a
sigma_block probe that straddles the block just touched and the live edge, and the nis a correction returns are the
model's numbers exactly; at the end all of Sigma, the tail's NaN payloads and -0.0 bit for bit.  A refused call returns
EKF_ERR_INVALID and the probes after it show that nothing changed.  Random forms (the same calls with Gaussian operands)
are held to FP64_TOL per block at every step against the plain float64 model, and the largest error is printed for
profiles/r17/dense64_sessions.txt.  tests/test_dense64_session_host.py proves the model."""
import ctypes

import numpy as np
import pytest

import dense_session_cases as ss
from parity import FP64_TOL, cov_err

pytestmark = pytest.mark.gpu
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
GRID = [(name, N, carry) for name, N in ss.CASES for carry in (True, False)]
IDS = [f"{name}-N{N}-{'carry' if carry else 'flush'}" for name, N, carry in GRID]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    """the same numbers; where the model holds a NaN (the tail's unique data) the same bits"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(a[~nan], b[~nan]) and np.array_equal(_bits(a)[nan], _bits(b)[nan])


def _p(a, kind=DP):
    return None if a is None else a.ctypes.data_as(kind)


def _refused(hip, d, op):
    """a call the handle must refuse, through the C ABI (the Python wrapper would stop some of them itself) -> status"""
    lib, k = hip.load(), op["op"]
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    if k in ("eager", "deferred"):
        fn = lib.ekf_dense64_correct_sparse_deferred if k == "deferred" else lib.ekf_dense64_correct_sparse
        cols, Hc, R, nu, nis = np.ascontiguousarray(op["cols"], dtype=np.int32), f64(op["Hc"]), f64(op["R"]), f64(op["nu"]), ctypes.c_double()
        return fn(d._h, Hc.shape[0], Hc.shape[1], _p(cols, IP), _p(Hc), _p(R), _p(nu), ctypes.byref(nis), None)
    if k == "propagate":
        Fr, Qr, dx = f64(op["Fr"]), f64(op["Qr"]), f64(op["dx"])
        return lib.ekf_dense64_propagate_block(d._h, int(op["first"]), len(Fr), _p(Fr), _p(Qr), _p(dx), None)
    if k == "swap":
        return lib.ekf_dense64_swap_blocks(d._h, int(op["a"]), int(op["b"]), int(op["r"]), None)
    raise KeyError(k)


def _call(hip, d, op):
    """one call of a session on the handle -> (status, value), what dense_session_cases.apply returns for the model"""
    k = op["op"]
    if op.get("refused"):
        return _refused(hip, d, op), None
    if k in ("eager", "deferred"):
        fn = d.correct_sparse_deferred if k == "deferred" else d.correct_sparse
        return ss.OK, fn(op["cols"], op["Hc"], op["R"], op["nu"])[0]
    if k == "propagate":
        d.propagate_block(op["first"], op["Fr"], op["Qr"], op["dx"])
    elif k == "init":
        d.init_block(op["first"], G=op["G"], cols=op["cols"], W=op["W"], xb=op["xb"], r=op["r"])
    elif k == "swap":
        d.swap_blocks(op["a"], op["b"], op["r"])
    elif k == "flush":
        d.flush()
    elif k == "live":
        d.live = op["Na"]
    elif k == "carry":
        d.carry = op["on"]
    elif k == "sigma_block":
        return ss.OK, d.sigma_block(op["rows"], op["cols"])
    elif k == "set":
        d.set(F=op["F"], Sigma=op["Sigma"], Q=op["Q"])
    elif k == "dense_propagate":
        d.propagate(1)
    elif k == "dense_correct":
        return ss.OK, d.correct(op["H"], op["R"], op["nu"])[0]
    elif k == "dense_score":
        nis, S, flags, _ = d.score(op["H"], op["R"], op["nu"], want_S=True)
        assert not flags.any()
        return ss.OK, (S, nis)
    elif k == "sigma":
        return ss.OK, d.sigma
    elif k == "coupling":
        return ss.OK, d.coupling(op["Na"])[:2]
    else:
        raise KeyError(k)
    return ss.OK, None


def _begin(hip, ses, carry):
    d = hip.DensePropagator64(ses["N"])
    d.set(Sigma=ses["Sigma0"])
    d.state = ses["x0"]
    d.carry = carry
    return d


def _same_value(got, want):
    if want is None:
        return got is None
    if isinstance(want, tuple) and isinstance(want[0], np.ndarray):
        return _same(got[0], want[0]) and _same(got[1], want[1])
    if isinstance(want, tuple):
        return tuple(got) == tuple(want)
    return _same(got, want)


def _step_exact(hip, d, ses, i, w):
    """call i of an integer session on the handle, then everything the model recorded after it"""
    op, at = ses["ops"][i], ss.describe(ses, i)
    status, value = _call(hip, d, op)
    assert status == w["status"] == (ss.INVALID if op.get("refused") else ss.OK), (at, status)
    assert _same_value(value, w["value"]), (at, value, w["value"])
    assert (d.pending, d.live, d.carry) == (w["pending"], w["live"], w["carry"]), (at, d.pending, d.live, w["pending"], w["live"])
    assert _same(d.state, w["state"]), (at, np.argwhere(d.state != w["state"])[:4].ravel())
    nis, S, flags, _ = d.score_sparse(*op["cand"], want_S=True)
    assert not flags.any() and _same(S, w["S"]) and _same(nis, w["nis"]), (at, S, w["S"], nis, w["nis"])
    if w["block"] is not None:
        got = d.sigma_block(op["rows"], op["cols_rd"])
        assert _same(got, w["block"]), (at, op["rows"], op["cols_rd"], got, w["block"])
    assert d.pending == w["pending"], at


@pytest.mark.parametrize("name,N,carry", GRID, ids=IDS)
def test_integer_session_is_the_model_after_every_call(hip, name, N, carry):
    ses = ss.session(name, N)
    want = ss.run(ses, carry)
    d = _begin(hip, ses, carry)
    for i, w in enumerate(want):
        _step_exact(hip, d, ses, i, w)
    got = d.sigma                                                      # all of [0, N)^2: the tail and both rectangles too
    assert d.pending == 0
    bad = ~((got == want[-1]["Sigma_cur"]) | (np.isnan(want[-1]["Sigma_cur"]) & (_bits(got) == _bits(want[-1]["Sigma_cur"]))))
    assert not bad.any(), (name, N, "the final Sigma", int(bad.sum()), np.argwhere(bad)[:4])
    top = ses["top"]
    if top < N and not any(o["op"] == "set" for o in ses["ops"]):
        out = np.ones((N, N), dtype=bool)
        out[:top, :top] = False
        assert np.array_equal(_bits(got)[out], _bits(ses["Sigma0"])[out]), (name, N, "the tail's bits")
    assert np.array_equal(_bits(d.state)[top:], _bits(ses["x0"])[top:])
    d.close()


def _rel(got, want):
    """the largest error relative to the block's own max-abs (parity._rel's rule)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not (np.isfinite(got).all() and np.isfinite(want).all()):
        return float("inf")
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-3)) if want.size else 0.0


def _read_all(d):
    N = d.N
    step = max(1, 65536 // N)
    return np.vstack([d.sigma_block(np.arange(k, min(N, k + step)), np.arange(N)) for k in range(0, N, step)])


@pytest.mark.parametrize("name,N,carry", GRID, ids=IDS)
def test_random_session_within_the_contract_at_every_step(hip, name, N, carry):
    """the plain float64 model is the reference; counts and live come from the integer session, whose op list this is"""
    ses, counts = ss.session(name, N, "random"), ss.run(ss.session(name, N), carry)
    want = ss.run(ses, carry, ss.PlainModel)
    d = _begin(hip, ses, carry)
    top, worst = ses["top"], 0.0
    for i, (op, w, c) in enumerate(zip(ses["ops"], want, counts)):
        at = ss.describe(ses, i)
        status, value = _call(hip, d, op)
        assert status == w["status"], at
        assert (d.pending, d.live, d.carry) == (c["pending"], c["live"], c["carry"]), at
        errs = {"state": _rel(d.state[:top], w["state"][:top])}
        if op["op"] in ("eager", "deferred", "dense_correct") and not op.get("refused"):
            errs["nis0"] = _rel(value, w["value"])
        nis, S, flags, _ = d.score_sparse(*op["cand"], want_S=True)
        assert not flags.any(), at
        errs["S"], errs["nis"] = _rel(S, w["S"]), _rel(nis, w["nis"])
        if ss.reads_block(c["carry"], c["pending"]):
            errs.update({"cov_" + k: v for k, v in cov_err(_read_all(d)[:top, :top], w["Sigma_cur"][:top, :top]).items()})
            assert d.pending == c["pending"], at
        worst = max(worst, max(errs.values()))
        assert max(errs.values()) <= FP64_TOL, (at, errs)
    got = d.sigma
    e = cov_err(got[:top, :top], want[-1]["Sigma_cur"][:top, :top])
    worst = max(worst, max(e.values()))
    print(f"measured {name} N={N} carry={int(carry)}: {worst:.3e}")
    assert max(e.values()) <= FP64_TOL, (name, N, e)
    if top < N:
        assert np.array_equal(_bits(got)[top:, top:], _bits(ses["Sigma0"])[top:, top:])
    d.close()


def test_two_handles_interleaved_do_not_disturb_each_other_and_a_fresh_one_is_zero(hip):
    """N = 67 (the corner grows to 35) and N = 131 (to 131) run their sessions op by op in turn, each equal to its own
    model after every call; then the first is closed, and a third handle is created -- all zero -- and run alone"""
    sa, sb, sc_ = (ss.session(name, N) for name, N, _ in ss.TWO_HANDLES)
    for carry in (True, False):
        wa, wb = ss.run(sa, carry), ss.run(sb, not carry)
        a, b = _begin(hip, sa, carry), _begin(hip, sb, not carry)
        for i in range(max(len(wa), len(wb))):
            if i < len(wa):
                _step_exact(hip, a, sa, i, wa[i])
            if i < len(wb):
                _step_exact(hip, b, sb, i, wb[i])
        assert _same(a.sigma, wa[-1]["Sigma_cur"]) and _same(b.sigma, wb[-1]["Sigma_cur"])
        a.close()
        c = hip.DensePropagator64(sc_["N"])
        assert (c.pending, c.live, c.carry) == (0, sc_["N"], False)
        assert not _bits(c.sigma).any() and not _bits(c.state).any()          # +0 everywhere
        assert _same(b.state, wb[-1]["state"])
        c.set(Sigma=sc_["Sigma0"])
        c.state = sc_["x0"]
        c.carry = carry
        wc = ss.run(sc_, carry)
        for i, w in enumerate(wc):
            _step_exact(hip, c, sc_, i, w)
        assert _same(c.sigma, wc[-1]["Sigma_cur"]) and _same(b.sigma, wb[-1]["Sigma_cur"])
        b.close()
        c.close()
