"""CPU (not gpu): the ground under tests/test_gpu_dense64_frame.py.  1. the op-by-op numpy model of dense_frame_cases equals
the exact int64 model of J Sigma J^T on every integer family, and its fused multiply-add is the correctly rounded one;
2. the slam_like family keeps its condition number and its 10 m; 3. the ROBOT Jacobian D + [C | 0] agrees with central
differences of the transform; 4. ROBOT twice is the identity in extended precision; 5. the NEES does not change under FIXED;
6. NULL handles and NULL arguments are refused through the built library; 7. the header states the rules the GPU test
holds."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dense_frame_cases as fr
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
GPU_SIZES = fr.sizes(64, 128)      # what the GPU test cuts from the tile the library reports today


@pytest.mark.parametrize("Na", [3, 5, 7, 13, 65, 131])
@pytest.mark.parametrize("family", sorted(fr.GS))
def test_model_equals_exact_arithmetic_on_the_integer_families(family, Na):
    S, G, C = fr.integer_corner(Na), fr.GS[family], fr.integer_C(Na)
    assert np.abs(S).max() <= 2 ** 10 and np.abs(C).max() <= 8 and not np.array_equal(S, S.T)
    for Cm in (None, C):
        want = fr.exact_congruence(S, G, Cm)
        assert fr.same_bits(fr.np_congruence(S, G, Cm), want)
        assert np.abs(want).max() < 2 ** 24                       # far below 2^53: exact in any order
        assert not fr.same_bits(fr.np_congruence(S.T.copy(), G, Cm), want)   # a transposed access shows


def test_the_models_fma_rounds_once():
    rng = np.random.default_rng(5)
    a, b, c = rng.standard_normal(200), rng.standard_normal(200), rng.standard_normal(200)
    c[:50] = -(a[:50] * b[:50])                                   # cancellation: the low half of the product is the result
    got = fr.fma(a, b, c)
    for x, y, z, r in zip(a, b, c, got):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        assert r == float(exact)
    assert np.any(got != a * b + c)                               # ... which two roundings miss
    assert fr.same_bits(fr.fma(0.0, 5.0, -0.0), 0.0) and fr.same_bits(fr.fma(-0.0, 5.0, -0.0), -0.0)
    assert fr.same_bits(fr.fma(3.0, 2.0, -6.0), 0.0) and math.isnan(fr.fma(1.0, math.nan, 0.0))


def test_identity_keeps_every_bit_and_step_one_alone_would_not():
    S = fr.integer_corner(7)
    S[2, 3], S[4, 4] = -0.0, fr.payload_nan(3)
    out = fr.np_congruence(S, np.eye(2), None)
    assert fr.same_bits(out, S)
    P = fr.np_D_congruence(S, np.eye(2))
    assert not fr.same_bits(P, S)                                 # -0.0 beside a positive entry, a NaN over its block


@pytest.mark.parametrize("Na", GPU_SIZES)
def test_slam_like_is_well_conditioned_and_not_symmetric(Na):
    S, x = fr.slam_like(Na), fr.slam_state(Na)
    assert fr.condition(S) <= fr.COND_MAX and not np.array_equal(S, S.T)
    r = np.hypot(x[3::2] - x[1], x[4::2] - x[2])
    assert r.size == (Na - 3) // 2 and (r.size == 0 or r.max() <= 10.0)


@pytest.mark.parametrize("Na", [3, 5, 13])
def test_robot_jacobian_agrees_with_central_differences(Na):
    x = fr.slam_state(Na)
    G, C = fr.robot_terms(x)
    J = fr.jacobian(Na, G, C)
    h = 1e-6
    num = np.empty((Na, Na))
    for j in range(Na):
        e = np.zeros(Na)
        e[j] = h
        num[:, j] = (fr.g_robot(x + e) - fr.g_robot(x - e)) / (2 * h)
    err = fr.row_scale_err(num, J)
    print(f"Na={Na}: ROBOT Jacobian against central differences {err:.3e}")
    assert err <= 1e-7


@pytest.mark.parametrize("Na", [3, 5, 13, 131])
def test_robot_twice_is_the_identity(Na):
    x = np.asarray(fr.slam_state(Na), dtype=np.longdouble)
    back = fr.g_robot(fr.g_robot(x, np.longdouble), np.longdouble)
    err = float(np.max(np.abs(back - x) / np.maximum(np.abs(x), 1)))
    assert err <= 1e-15, err
    G, C = fr.robot_terms(x.astype(np.float64))
    G2, C2 = fr.robot_terms(fr.g_robot(x.astype(np.float64)))
    JJ = fr.jacobian(Na, G2, C2) @ fr.jacobian(Na, G, C)          # the Jacobians compose to the identity too
    assert np.max(np.abs(JJ - np.eye(Na))) <= 1e-13


@pytest.mark.parametrize("Na", [5, 13, 65])
def test_nees_is_invariant_under_fixed(Na):
    S = fr.slam_like(Na)
    S = 0.5 * (S + S.T)
    x = fr.slam_state(Na)
    truth = x + 0.1 * np.random.default_rng(Na).standard_normal(Na) * np.sqrt(np.diagonal(S))
    dth, tx, ty = 0.7, 3.0, -2.0
    G = fr.fixed_terms(dth)
    S2 = fr.np_congruence(S, G, None)
    e, e2 = x - truth, fr.g_fixed(x, dth, tx, ty) - fr.g_fixed(truth, dth, tx, ty)
    nees, nees2 = e @ np.linalg.solve(S, e), e2 @ np.linalg.solve(S2, e2)
    assert abs(nees2 - nees) <= 1e-9 * nees, (nees, nees2)
    assert np.all(np.abs(fr.g_fixed(x, dth, tx, ty) - fr.g_fixed(x, dth, tx, ty, np.longdouble))
                  <= fr.fixed_state_bound(x, dth, tx, ty))


def test_null_handles_and_arguments_are_refused_without_a_device():
    lib = capi.load()
    a, b, c = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    buf = np.full(13, 7.0)
    assert lib.ekf_dense64_map_congruence(None, capi._d(buf), None, None) == 1
    assert b"null handle" in lib.ekf_last_error()
    assert lib.ekf_dense64_reframe_landmarks(None, 0, 0.0, 0.0, 0.0, capi._d(buf), None) == 1
    assert lib.ekf_dense64_frame_launch_info(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 1
    assert (a.value, b.value, c.value) == (7, 7, 7) and np.array_equal(buf, np.full(13, 7.0))


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with a closed handle")


def test_wrapper_checks_come_before_the_library():
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = 7, _NoLibrary(), None
    for call in (lambda: d.map_congruence(np.eye(2)), lambda: d.reframe(0), d.frame_launch_info):
        with pytest.raises(ValueError):
            call()
    d._lib = None
    assert callable(capi.DenseEKFSLAM.reframe) and callable(capi.DenseEKFSLAM.robot_frame)
    assert (capi.DensePropagator64.FRAME_FIXED, capi.DensePropagator64.FRAME_ROBOT) == (fr.FIXED, fr.ROBOT)


def test_calls_are_declared_bound_and_documented():
    for name in ("ekf_dense64_map_congruence", "ekf_dense64_reframe_landmarks", "ekf_dense64_frame_launch_info"):
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", HDR, re.M) and name in capi.SYMBOLS
    assert re.search(r"#define EKF_DENSE64_FRAME_FIXED\s+0\b", HDR) and re.search(r"#define EKF_DENSE64_FRAME_ROBOT\s+1\b", HDR)
    text = " ".join(HDR.split())
    for rule in ("NA MUST BE ODD AND >= 3", "ODD-ALIGNED, INDEX 0 STANDS ALONE", "FLUSHES THE PENDING ROWS FIRST, carry or not",
                 "IT DOES NOT TOUCH THE STATE VECTOR", "Y[r][c] = fma(G[r][1], B[1][c], fl(G[r][0] * B[0][c]))",
                 "the C A terms first, k ascending", "SKIPPED, not multiplied by zeros", "G = I IN BITS",
                 "SIGMA IS NEVER SYMMETRISED", "ORIGINS SIT ON ODD INDICES", "NO ATOMICS: A RUN REPEATS BIT FOR BIT",
                 "NOT WRAPPED", "ONCE ON THE HOST", "ON THE DEVICE", "its own inverse up to rounding",
                 "NOT THE PARAMETERISATION ekf_dense64_predict_landmarks ASSUMES", "call it again before filtering on",
                 "BIT FOR BIT, ekf_dense64_map_congruence WITH THOSE OPERANDS", "EKF_ERR_NOMEM"):
        assert rule in text, rule
    for doc, words in (("DESIGN.md", "4.8.20"), ("DESIGN.md", "k_fr_update"), ("README.md", "ekf_dense64_frame.hip"),
                       ("INTEGRATION.md", "world-frame truth")):
        assert words in open(os.path.join(ROOT, doc)).read(), (doc, words)
