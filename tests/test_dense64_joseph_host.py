"""CPU (not gpu): the ground under tests/test_gpu_dense64_joseph.py.  1. on the integer families the model's residual D is
exactly 0 and its result equals the short form's entry by entry; 2. with weights the model meets the long-double Joseph
expression at 1e-12 while the short form with the same weighted gain is farther than 1e-3 from it; 3. the committed
ill-conditioned family: the short form's result stops the Cholesky model, the Joseph model's completes, with the margins the
cases file promises; 4. the refusals that need no device; 5. the header's definition names every rule the model implements."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_factor_cases as fc
import dense_joseph_cases as jc
import dense_sparse_cases as sp
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
JOSEPH, INFO = "ekf_dense64_correct_sparse_joseph", "ekf_dense64_joseph_launch_info"
INVALID = 1


@pytest.mark.parametrize("N", jc.SIZES)
def test_integer_families_have_a_zero_residual_and_equal_the_short_form(N):
    for m, s, order in jc.shapes(N):
        c = jc.integer_case(N, m, s, order, 7000 + 31 * N + 7 * m + s)
        T, U, S, Si = jc.panels(c["Sigma"], c["cols"], c["Hc"], c["R"])
        K = jc.gain(U, Si, None)
        assert not jc.residual(U, K, S).any(), (N, m, s)                     # D = 0 exactly
        x, Sig, nis = jc.np_joseph(c["x"], c["Sigma"], c["cols"], c["Hc"], c["R"], c["nu"])
        wx, wS, wn = sp.np_correct(c["x"], c["Sigma"], c["cols"], c["Hc"], c["R"], c["nu"])
        assert (Sig == wS).all() and (x == wx).all() and nis == wn, (N, m, s)
        # quarters as weights keep every intermediate a dyadic rational: the long-double expression is met exactly
        w = jc.weights("quarters", N, N, 5 + N)
        _, Sw, _ = jc.np_joseph(c["x"], c["Sigma"], c["cols"], c["Hc"], c["R"], c["nu"], w)
        assert (Sw == np.asarray(jc.joseph_longdouble(c["Sigma"], c["cols"], c["Hc"], c["R"], w), dtype=np.float64)).all()


@pytest.mark.parametrize("kind", jc.WEIGHT_KINDS)
def test_weighted_model_meets_the_joseph_expression_and_the_short_form_does_not(kind):
    N = 129
    for m, s, order in [(2, 5, "asc"), (3, 64, "scattered"), (32, 5, "asc")]:
        c = jc.slam_case(N, m, s, order, 100 + m)
        w = jc.weights(kind, N, N, 40 + m)
        w[c["cols"][0]] = 0.5 if kind in ("random", "quarters") else w[c["cols"][0]]
        x, Sig, _ = jc.np_joseph(c["x"], c["Sigma"], c["cols"], c["Hc"], c["R"], c["nu"], w)
        want = jc.joseph_longdouble(c["Sigma"], c["cols"], c["Hc"], c["R"], w)
        err = jc.rel_cov_error(Sig, want, c["Sigma"])
        short = jc.rel_cov_error(jc.np_short_form(c["Sigma"], c["cols"], c["Hc"], c["R"], w), want, c["Sigma"])
        print(f"{kind} m={m} s={s}: model {err:.2e}, short form with the same gain {short:.2e}")
        assert err <= jc.TOL and short > 1e-3, (kind, m, s, err, short)
        off = w == 0.0
        assert jc.same_bits(Sig[np.ix_(off, off)], c["Sigma"][np.ix_(off, off)]) and jc.same_bits(x[off], c["x"][off])


def test_ill_conditioned_family_separates_the_two_forms():
    p = jc.ILL
    assert (p["Na"], p["m"], p["s"], p["prior"], p["r"]) == (13, 2, 5, 1e12, 1e-6)
    c = jc.ill_case()
    a = 3 + 2 * p["landmark"]
    assert c["Sigma"][a, a] == 1e12 and np.array_equal(c["R"], 1e-6 * np.eye(2)) and np.array_equal(c["Sigma"], c["Sigma"].T)
    assert fc.np_factor(c["Sigma"])[0]["ok"] == 1                            # the prior itself is positive definite
    truth = np.asarray(jc.joseph_longdouble(c["Sigma"], c["cols"], c["Hc"], c["R"]), dtype=np.float64)
    # ... and so is the posterior, two orders above an ulp of the prior, the scale at which the accumulator rounds
    assert np.linalg.eigvalsh(truth)[0] > 1e2 * np.spacing(1e12)
    short, jos = jc.ill_margins(c)
    print("short form: worst pivot / ulp", max(m for _, m in short), " Joseph: least pivot / ulp", min(m for _, m in jos))
    assert all(ok == 0 and margin <= -1e3 for ok, margin in short)
    assert all(ok == 1 and margin >= 1e3 for ok, margin in jos)
    _, Sj, _ = jc.np_joseph(c["x"], c["Sigma"], c["cols"], c["Hc"], c["R"], c["nu"])
    assert fc.np_factor(Sj)[0]["ok"] == 1
    assert fc.np_factor(jc.np_short_form(c["Sigma"], c["cols"], c["Hc"], c["R"]))[0]["ok"] == 0


def test_tile_count_model():
    w = np.ones(300)
    assert jc.tiles_skipped(300, None, 16, 128) == 0 and jc.tiles_skipped(300, w, 16, 128) == 0
    w[128:] = 0.0
    assert jc.tiles_skipped(300, w, 16, 128) == 11 * 2                       # row blocks 8 .. 18, strips 1 and 2
    w[299] = 0.5
    assert jc.tiles_skipped(300, w, 16, 128) == 10 * 1


def test_null_handle_and_bad_arguments_are_refused_without_a_device():
    lib = capi.load()
    cols = np.array([0, 1, 2, 7, 8], dtype=np.int32)
    Hc, R, nu, w = np.ones((2, 5)), np.eye(2), np.ones(2), np.ones(30)
    big = np.ones((33, 5))
    nis, skipped, ms = ctypes.c_double(7.0), ctypes.c_longlong(7), ctypes.c_double(7.0)
    ip = cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    for m, hc, weights in ((2, Hc, w), (2, Hc, None), (33, big, w), (2, Hc, np.full(30, np.nan))):
        st = lib.ekf_dense64_correct_sparse_joseph(None, m, 5, ip, capi._d(hc), capi._d(R), capi._d(nu),
                                                   capi._d(weights) if weights is not None else None, ctypes.byref(nis),
                                                   ctypes.byref(skipped), ctypes.byref(ms))
        assert st == INVALID and JOSEPH.encode() in lib.ekf_last_error()
    assert (nis.value, skipped.value, ms.value) == (7.0, 7, 7.0)
    a, b, c = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    assert lib.ekf_dense64_joseph_launch_info(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == INVALID
    assert (a.value, b.value, c.value) == (7, 7, 7)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_refuses_m_33_and_bad_weights_before_the_library():
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = 40, _NoLibrary(), None
    c5, Hc, R, nu = [0, 1, 2, 7, 8], np.ones((2, 5)), np.eye(2), np.ones(2)
    bad = [lambda: d.correct_sparse_joseph(c5, np.ones((33, 5)), np.eye(33)),
           lambda: d.correct_sparse_joseph(c5, Hc, R, nu, np.full(40, np.nan)),
           lambda: d.correct_sparse_joseph(c5, Hc, R, nu, np.full(40, -0.5)),
           lambda: d.correct_sparse_joseph(c5, Hc, R, nu, np.full(40, 1.5)),
           lambda: d.correct_sparse_joseph(c5, Hc, R, nu, np.full(40, np.inf)),
           lambda: d.correct_sparse_joseph(c5, Hc, R, nu, np.ones(39)),
           lambda: d.correct_sparse_joseph([0, 1, 2, 7, 7], Hc, R, nu),
           lambda: d.associate_landmarks(np.zeros((1, 2)), 0, 3, deferred=True, joseph=True),
           lambda: d.measure_landmarks(np.zeros((3, 2)), np.ones(3), True, deferred=True, joseph=True),
           lambda: d.merge_landmarks(0, 1, 0.1, 2, flags=d.LM_JOSEPH | d.LM_DEFERRED),
           d.joseph_launch_info]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError):
        capi.DenseEKFSLAM(3, deferred=True, joseph=True)
    d._lib = None


def test_calls_are_declared_bound_and_documented():
    lib = capi.load()
    for name in (JOSEPH, INFO):
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", HDR, re.M) and name in capi.SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define EKF_DENSE64_JOSEPH_MAX_M\s+32\b", HDR)
    assert capi.DensePropagator64.JOSEPH_MAX_M == 32 == jc.JOSEPH_MAX_M
    assert re.search(r"#define EKF_DENSE64_LM_JOSEPH\s+8u\b", HDR) and capi.DensePropagator64.LM_JOSEPH == 8 == jc.LM_JOSEPH
    text = " ".join(" ".join(re.sub(r"^\s*\*", " ", line) for line in HDR.splitlines()).split())   # (comment leaders dropped)
    for rule in ("SAME T, U, S, S^-1, nis", "THE GAIN: K[i][k] = +0.0 when w_i == 0, otherwise fl(w_i * G[i][k])",
                 "Rows i >= Na are zero", "THE STATE", "A state with w_i == 0 is NOT WRITTEN",
                 "THE RESIDUAL: D[i][k] = U[i][k] - sum_l K[i][l] S[l][k]", "one fused multiply-add per l, ascending",
                 "THE COVARIANCE", "the K T terms come first, then the D K^T terms", "a run repeats bit for bit",
                 "THE CONSIDER RULE", "enters no result and is not written", "takes the D K^T terms only, with D[i] = U[i]",
                 "takes the K T terms only", "*tiles_skipped (nullable) is the number of untouched tiles",
                 "must be finite and in [0, 1]", "values at indices >= Na are ignored", "FLUSHES THE PENDING ROWS FIRST",
                 "Nothing at a row or column >= Na is read or written", "returns EKF_ERR_STATE",
                 "1 <= m <= EKF_DENSE64_JOSEPH_MAX_M",
                 "together with EKF_DENSE64_LM_DEFERRED the call returns EKF_ERR_INVALID", "Without the flag every launch and every bit is as before"):
        assert rule in text, rule
    for doc, words in (("README.md", JOSEPH), ("DESIGN.md", "4.8.19"), ("DESIGN.md", "k_dj_update"),
                       ("INTEGRATION.md", "correct_sparse_joseph")):
        assert words in open(os.path.join(ROOT, doc)).read(), (doc, words)
