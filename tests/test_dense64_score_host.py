"""CPU (not gpu): the batched candidate scoring of the fp64 dense handle (ekf_dense64_score) is exported, declared, bound,
checks its arguments before it looks for a device, and its recorded reference data meets numpy's literal spelling."""
import ctypes
import os
import re

import numpy as np
import pytest

from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ekf_dense64_score"


def _built():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_dense64_score_symbol_exported_and_declared():
    _built()
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert hasattr(lib, NAME)
    assert NAME in capi.SYMBOLS
    assert re.search(r"ekf_status\s+%s\s*\(" % NAME, header)
    m = re.search(r"#define\s+EKF_DENSE64_SCORE_MAX_ROWS\s+(\d+)", header)
    assert m and int(m.group(1)) == 2048 == capi.DensePropagator64.SCORE_MAX_ROWS
    assert callable(getattr(capi.DensePropagator64, "score"))


def test_dense64_score_bad_arguments_without_device():
    """every EKF_ERR_INVALID case that needs no live handle: a NULL handle with otherwise valid arguments, and with each
    bad argument -- answered before the device is looked at, the function named in ekf_last_error()"""
    _built()
    lib = capi.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    N, J, m = 5, 3, 2
    H = np.ones((J, m, N)); R = np.stack([np.eye(m)] * J); nu = np.ones((J, m))
    nis = np.zeros(J); S = np.zeros((J, m, m)); flags = np.zeros(J, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(dp)
    ms = ctypes.c_double()
    INVALID = 1
    ok = dict(J=J, m=m, H=p(H), R=p(R), shared=0, nu=p(nu), nis=p(nis), S=p(S), flags=flags.ctypes.data_as(ip))
    cases = [{}, {"shared": 1}, {"J": 0}, {"J": -1}, {"J": 1025, "m": 2}, {"J": 2049, "m": 1}, {"J": 1, "m": 2049},
             {"m": 0}, {"m": -1}, {"m": 65}, {"J": 1 << 20, "m": 1 << 20}, {"H": None}, {"R": None}, {"nu": None},
             {"nis": None, "S": None, "flags": None}, {"nu": None, "nis": None, "S": None, "flags": None}]
    for bad in cases:
        a = dict(ok, **bad)
        st = lib.ekf_dense64_score(None, a["J"], a["m"], a["H"], a["R"], a["shared"], a["nu"], a["nis"], a["S"],
                                   a["flags"], ctypes.byref(ms))
        assert st == INVALID, (bad, st)
        assert NAME.encode() in lib.ekf_last_error(), bad
    assert lib.ekf_dense64_score(None, J, m, p(H), p(R), 0, None, None, p(S), None, None) == INVALID


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the shapes were checked")


def test_score_shape_checks_raise_before_the_library():
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = 30, _NoLibrary(), None
    N, J, m = 30, 4, 2
    H, R, nu = np.ones((J, m, N)), np.eye(m), np.ones((J, m))
    bad = [lambda: d.score(np.ones((m, N)), R, nu),                 # not J x m x N
           lambda: d.score(np.ones((J, m, N + 1)), R, nu),
           lambda: d.score(np.ones((0, m, N)), R),
           lambda: d.score(np.ones((J, 0, N)), np.eye(0)),
           lambda: d.score(np.ones((1, N + 1, N)), np.eye(N + 1)),  # m > N
           lambda: d.score(np.ones((1025, 2, N)), R),               # J * m = 2050
           lambda: d.score(H, np.eye(3), nu),
           lambda: d.score(H, np.ones((J + 1, m, m)), nu),
           lambda: d.score(H, R, np.ones(J * m)),
           lambda: d.score(H, R, np.ones((J, m + 1)))]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    d65 = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d65.N, d65._lib, d65._h = 100, _NoLibrary(), None
    with pytest.raises(ValueError):
        d65.score(np.ones((1, 65, 100)), np.eye(65))


def test_score_fixture_meets_numpy_literal_spelling():
    """tests/golden/dense_score_ref.npz (the reference build's calculate_maha_dis at n = 20, 8 readings x 20 landmarks):
    numpy's literal spelling (H @ cov @ H.T + R, inv) meets every recorded score at FP64_TOL relative, so a failure of the
    GPU on the fixture is the kernel's; and the recording keeps the margins the GPU comparison of decisions relies on"""
    import dense_score_cases as ds
    from parity import FP64_TOL
    path = os.path.join(ROOT, "tests", "golden", "dense_score_ref.npz")
    assert os.path.getsize(path) <= 100 * 1024
    z = np.load(path)
    assert int(z["n"]) == 20 and z["maha"].shape == (8, 20) and z["readings"].shape == (8, 2)
    worst = 0.0
    for k, (sx, sy) in enumerate(z["readings"]):
        assert ds.margins_hold(z["maha"][k]), k
        H, R, nu = ds.candidate_terms(z["state"], sx, sy)
        nis = ds.np_scores(z["cov"], H, R, nu)[1]
        worst = max(worst, float((np.abs(nis - z["maha"][k]) / np.abs(z["maha"][k])).max()))
        assert ds.reference_rule(nis) == ds.reference_rule(z["maha"][k])
    print(f"numpy vs calculate_maha_dis on the fixture: worst relative {worst:.2e}")
    assert worst <= FP64_TOL
