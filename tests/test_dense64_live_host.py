"""No GPU: the algebra behind the live dimension of the dense fp64 handle (ekf_dense64_set_live), on the numpy models the
other dense64 host files use (the eager sparse chain, DeferredModel, the carried model of tests/dense_carry_cases.py).
Every chain of tests/dense_live_cases.py -- the ones tests/test_gpu_dense64_live.py compares the device against bit for bit
-- is built on CarriedModel, which refuses (Inexact) any product whose terms are not integers over one power of two with
the sum of their absolute values below 2^52: every number below is exact in float64 in any order of summation.  On those
chains, embedded in N > Na with a decoupled tail that holds a dense block, the FULL-WIDTH model leaves the tail and both
rectangles exactly as they were and its corner equals the model run at dimension Na: the reason the policy is exact for a
growing map.  Also the symbols, and the refusals that need no device."""
import ctypes

import numpy as np
import pytest

import dense_carry_cases as cc
import dense_deferred_cases as dd
import dense_live_cases as lc
import dense_sparse_cases as sp


def test_the_grid():
    pairs = lc.pairs()
    assert len(pairs) == 6 + 11 + 11 and all(Na < N for N, Na in pairs)
    assert {Na for _, Na in pairs} == set(lc.GRID_NA) and {N for N, _ in pairs} == set(lc.GRID_N)
    assert lc.shapes(1) == [(1, 1)] and lc.shapes(5) == [(1, 1), (2, 5)] and lc.shapes(17) == lc.PAIRS[:4]
    assert lc.shapes(64) == lc.PAIRS == lc.shapes(191)


@pytest.mark.parametrize("Na", lc.GRID_NA)
def test_full_width_model_leaves_the_tail_and_equals_the_live_model(Na):
    """every chain of this Na, carried and flush-first: run at dimension Na and run at N = Na + 9 (and one at a larger N)
    on the embedding; the tail block, the tail state and both rectangles keep their values after every call -- also in the
    pending panels, whose rows are zero from Na on -- and everything in the corner is the same number"""
    for order in lc.ORDERS:
        for m, s in lc.shapes(Na):
            chain = lc.live_chain(Na, order, m, s)                     # raises Inexact when not exact in float64
            assert [op["op"] for op in chain["ops"]] == ["eager", "deferred", "propagate", "init", "deferred", "flush"]
            for N in ([Na + 9, 2 * Na + 70] if (order, (m, s)) == (lc.ORDERS[0], lc.shapes(Na)[-1]) else [Na + 9]):
                S0, x0 = lc.embed(chain, N, seed=Na)
                assert np.count_nonzero(S0[Na:, Na:]) == (N - Na) ** 2   # the tail is dense
                for carry in (True, False):
                    small, full = lc.run_model(chain, carry), lc.run_model(chain, carry, S0, x0)
                    for i, (a, b) in enumerate(zip(small, full)):
                        what = (Na, order, m, s, N, carry, i)
                        Sc = b["Sigma_cur"]
                        assert np.array_equal(Sc[Na:, Na:], S0[Na:, Na:]) and np.array_equal(b["state"][Na:], x0[Na:]), what
                        assert not Sc[:Na, Na:].any() and not Sc[Na:, :Na].any(), what
                        assert np.array_equal(Sc[:Na, :Na], a["Sigma_cur"]) and np.array_equal(b["state"][:Na], a["state"]), what
                        assert a["pending"] == b["pending"] and a["nis0"] == b["nis0"], what
                        assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["nis"], b["nis"]), what
            carried, flushed = lc.run_model(chain, True), lc.run_model(chain, False)
            assert carried[2]["pending"] == carried[3]["pending"] == m and flushed[2]["pending"] == 0
            assert carried[-1]["pending"] == 0 and np.array_equal(carried[-1]["Sigma_cur"], flushed[-1]["Sigma_cur"])


def test_pending_rows_of_the_full_width_model_are_zero_beyond_the_live_dimension():
    """what makes growing exact without a flush: K^T and T of a correction listed below Na on a decoupled Sigma are zero
    from Na on, and stay so through the carried maps"""
    Na, N = 17, 40
    chain = lc.live_chain(Na, "scattered", 2, 5)
    S0, x0 = lc.embed(chain, N)
    model = cc.CarriedModel(S0, x0)
    for op in chain["ops"][:-1]:
        lc.apply(model, op)
        assert not model.Kt[:, Na:].any() and not model.Tp[:, Na:].any()
    assert model.pending > 0


def test_the_eager_chain_and_the_deferred_model_agree_with_the_embedding():
    """the same statement on the two older models: sp.np_correct on an embedded integer chain, and DeferredModel"""
    Na, N = 65, 90
    chain = dd.integer_chain(Na, "scattered")
    B, xt = lc.tail_block(N - Na, 3)
    S = np.zeros((N, N))
    S[:Na, :Na], S[Na:, Na:] = chain["Sigma0"], B
    x = np.concatenate([chain["x0"], xt])
    model = dd.DeferredModel(S, x)
    for st in chain["steps"]:
        c, h, R, nu = st["cols"][0], st["Hc"][0], st["R"][0], st["nu"][0]
        x, S, nis = sp.np_correct(x, S, c, h, R, nu)
        assert nis == st["nis0"] == model.correct_deferred(c, h, R, nu)
        for got_x, got_S in ((x, S), (model.state, model.sigma_cur)):
            assert np.array_equal(got_S[:Na, :Na], st["Sigma"]) and np.array_equal(got_x[:Na], st["state"])
            assert np.array_equal(got_S[Na:, Na:], B) and np.array_equal(got_x[Na:], xt)
            assert not got_S[:Na, Na:].any() and not got_S[Na:, :Na].any()
    dd.exact_replay(chain)                                            # the chain itself stays inside float64


def test_symbols_and_refusals_without_a_device():
    from ekf_slam_ml_amd import capi
    lib = capi.load()
    for name in ("ekf_dense64_set_live", "ekf_dense64_get_live", "ekf_dense64_coupling"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
    assert isinstance(capi.DensePropagator64.live, property) and callable(capi.DensePropagator64.coupling)
    na, count, most = ctypes.c_int(7), ctypes.c_longlong(7), ctypes.c_double(7.0)
    assert lib.ekf_dense64_set_live(None, 3) == 1                     # EKF_ERR_INVALID, before any device is looked at
    assert lib.ekf_dense64_get_live(None, ctypes.byref(na)) == 1 and na.value == 7
    assert lib.ekf_dense64_coupling(None, 3, ctypes.byref(count), ctypes.byref(most), None) == 1
    assert count.value == 7 and most.value == 7.0
