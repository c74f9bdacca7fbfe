"""CPU (not gpu): the ground under tests/test_gpu_dense64_factor.py.  1. the numpy model of dense_factor_cases equals
Fraction arithmetic on the integer families; 2. at every size the GPU test can use (block sides 16 .. 128) the integer
corners stay far below 2^53 and numpy's own Cholesky returns L0 exactly; 3. the derived bounds hold for numpy's factor and
for the model's substitution on slam_like at those sizes; 4. the NULL-handle refusals through the built library; 5. the
header names the lower-triangle rule, the snapshot rule and the stop rule, and the wrapper mirrors the report."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dense_factor_cases as fc
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
ALL_SIZES = sorted({Na for nb in fc.BLOCK_SIDES for Na in fc.sizes(nb)})


def _fraction_factor(C):
    """Cholesky in exact arithmetic on the lower triangle; a pivot that is no square of a rational is an error ->
    (fail_index, pivots, L as Fractions)"""
    Na = C.shape[0]
    L = [[Fraction(0)] * Na for _ in range(Na)]
    pivots = []
    for j in range(Na):
        d = Fraction(C[j, j]) - sum(L[j][k] * L[j][k] for k in range(j))
        if not d > 0:
            return j, pivots + [d], L
        pivots.append(d)
        rn, rd = math.isqrt(d.numerator), math.isqrt(d.denominator)
        assert rn * rn == d.numerator and rd * rd == d.denominator
        L[j][j] = Fraction(rn, rd)
        for i in range(j + 1, Na):
            L[i][j] = (Fraction(C[i, j]) - sum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    return -1, pivots, L


@pytest.mark.parametrize("Na", [1, 2, 3, 15, 17, 33, 50])
def test_model_equals_exact_arithmetic_on_the_integer_families(Na):
    C, L0 = fc.integer_factor(Na)
    fail, piv, Lx = _fraction_factor(C)
    rep, L = fc.np_factor(C)
    assert fail == -1 and rep["ok"] == 1 and rep["fail_index"] == -1 and rep["Na"] == Na
    assert fc.same_bits(L, L0) and all(Fraction(L[i, j]) == Lx[i][j] for i in range(Na) for j in range(Na))
    assert Fraction(rep["min_pivot"]) == min(piv) and Fraction(rep["max_pivot"]) == max(piv)
    assert rep["min_pivot_i"] == piv.index(min(piv))
    assert fc.same_bits(rep["logdet"], fc.host_logdet(np.diagonal(L0)))
    for p in fc.fail_columns(16, Na):
        for c in (0, 3):
            Ci, _ = fc.integer_indefinite(Na, p, c)
            fail, piv, _ = _fraction_factor(Ci)
            rep, L = fc.np_factor(Ci)
            assert fail == p and piv[-1] == -c
            assert (rep["ok"], rep["fail_index"]) == (0, p) and fc.same_bits(rep["fail_pivot"], -float(c) if c else 0.0)
            assert fc.same_bits(L[:, :p], L0[:, :p]) and math.isnan(rep["logdet"])
            if p:
                assert Fraction(rep["min_pivot"]) == min(piv[:p]) and Fraction(rep["max_pivot"]) == max(piv[:p])
                assert rep["min_pivot_i"] == piv.index(min(piv[:p]))
            else:
                assert (rep["min_pivot"], rep["max_pivot"], rep["min_pivot_i"]) == (math.inf, 0.0, -1)
        if p >= 1:
            Cn, _ = fc.nan_entry(Na, p, p // 2)
            rep, L = fc.np_factor(Cn)
            assert (rep["ok"], rep["fail_index"]) == (0, p) and math.isnan(rep["fail_pivot"])
            assert fc.same_bits(L[:p, :p], L0[:p, :p])


@pytest.mark.parametrize("Na", ALL_SIZES)
def test_integer_corners_are_exact_at_every_gpu_size(Na):
    C, L0 = fc.integer_factor(Na)
    assert np.abs(C).max() <= 9 * Na + 16 < 2 ** 20 and np.array_equal(C, np.rint(C)) and np.array_equal(C, C.T)
    assert 9.0 * Na * 16 * 4 < 2 ** 53                      # the largest partial sum times the largest divisor
    assert fc.same_bits(np.linalg.cholesky(C), L0)          # numpy's own factor, its own order of summation
    Z = np.random.default_rng(Na).integers(-3, 4, size=(3, Na)).astype(np.float64)
    Y, d2 = fc.np_whiten(L0, Z @ L0.T)
    assert fc.same_bits(Y, Z) and fc.same_bits(d2, (Z * Z).sum(axis=1))


@pytest.mark.parametrize("Na", ALL_SIZES)
def test_derived_bounds_hold_for_numpy_on_slam_like(Na):
    A = fc.slam_like(Na)
    assert np.array_equal(A, A.T)
    L = np.linalg.cholesky(A)
    ratio = fc.factor_residual_ratio(A, L)
    logdet = fc.host_logdet(np.diagonal(L))
    err, bound = abs(logdet - np.linalg.slogdet(A)[1]), fc.logdet_bound(A, L)
    b = np.random.default_rng(Na + 5).standard_normal(Na)
    Y, d2 = fc.np_whiten(L, b)
    wr, nr = fc.whiten_residual_ratio(L, Y[0], b), fc.norm_ratio(Y[0], d2[0])
    print(f"Na={Na}: residual / bound {ratio:.3f}; logdet error {err:.2e} of {bound:.2e}; substitution {wr:.3f}; norm {nr:.3f}")
    assert ratio <= 1.0 and err <= bound and wr <= 1.0 and nr <= 1.0
    junk = fc.slam_like_input(Na)
    above = junk[np.triu(np.ones((Na, Na), dtype=bool), 1)]
    assert fc.same_bits(np.tril(junk), np.tril(A)) and (np.isnan(above) | (np.abs(above) > 1e200)).all()
    rep, Lm = fc.np_factor(junk)                            # the model reads the lower triangle only
    assert rep["ok"] == 1 and fc.factor_residual_ratio(A, Lm) <= 1.0


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_checks_come_before_the_library():
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = 30, _NoLibrary(), None   # a closed handle
    for call in (d.factor, d.get_factor, d.factor_launch_info, lambda: d.whiten(np.zeros(30))):
        with pytest.raises(ValueError):
            call()
    d._lib = None
    assert callable(capi.DenseEKFSLAM.factor) and callable(capi.DenseEKFSLAM.map_nees)


def test_null_handles_are_refused_without_a_device():
    lib = capi.load()
    rep, a, b = capi.FactorReport(), ctypes.c_int(7), ctypes.c_int(7)
    buf = np.full(4, 7.0)
    rep.Na = 7
    assert lib.ekf_dense64_factor(None, ctypes.byref(rep), None) == 1 and rep.Na == 7
    assert lib.ekf_dense64_factor_launch_info(None, ctypes.byref(a), ctypes.byref(b)) == 1 and (a.value, b.value) == (7, 7)
    assert lib.ekf_dense64_get_factor(None, capi._d(buf)) == 1
    assert lib.ekf_dense64_whiten(None, 1, capi._d(buf), capi._d(buf), capi._d(buf), None) == 1
    assert np.array_equal(buf, np.full(4, 7.0))
    assert b"null handle" in lib.ekf_last_error()


def test_calls_are_declared_bound_and_documented():
    for name in ("ekf_dense64_factor", "ekf_dense64_factor_launch_info", "ekf_dense64_get_factor", "ekf_dense64_whiten"):
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", HDR, re.M) and name in capi.SYMBOLS
    body = re.search(r"typedef struct ekf_dense64_factor_report \{(.*?)\} ekf_dense64_factor_report;", HDR, re.S).group(1)
    names = re.findall(r"^\s*(int|double)\s+([a-z_A-Z]+);", body, re.M)
    ctype = {ctypes.c_double: "double", ctypes.c_int: "int"}
    assert names == [(ctype[t], n) for n, t in capi.FactorReport._fields_]       # the same fields in the same order
    assert tuple(n for _, n in names) == fc.REPORT_FIELDS
    assert re.search(r"#define EKF_DENSE64_WHITEN_MAX_RHS\s+64\b", HDR) and capi.DensePropagator64.WHITEN_MAX_RHS == 64
    text = " ".join(HDR.split())
    for rule in ("THE LOWER TRIANGLE ONLY IS READ", "calls ekf_dense64_symmetrize first",      # the lower-triangle rule
                 "THE FACTOR IS A SNAPSHOT", "neither touch nor invalidate the snapshot",      # the snapshot rule
                 "THE STOP RULE", "not (finite and > 0) ends the factorisation",                # the stop rule
                 "FLUSHES THE PENDING ROWS FIRST", "does NOT flush the pending rows", "812.8 MB at Na = 10003"):
        assert rule in text, rule
    for doc, words in (("DESIGN.md", "ekf_dense64_factor"), ("INTEGRATION.md", "ekf_dense64_whiten"),
                       ("INTEGRATION.md", "map_nees")):
        assert words in open(os.path.join(ROOT, doc)).read(), (doc, words)
