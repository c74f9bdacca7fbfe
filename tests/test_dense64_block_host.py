"""CPU (not gpu): the block-structured prediction of the fp64 dense handle (ekf_dense64_propagate_block) is exported,
declared, bound, and checks its arguments before it looks for a device; the recorded reference prediction() meets numpy's
literal spelling."""
import ctypes
import os
import re

import numpy as np
import pytest

from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ekf_dense64_propagate_block"


def _built():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_dense64_block_symbol_exported_and_declared():
    _built()
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    assert hasattr(lib, NAME)
    assert NAME in capi.SYMBOLS
    assert re.search(r"ekf_status\s+%s\s*\(" % NAME, header)
    m = re.search(r"#define\s+EKF_DENSE64_MAX_R\s+(\d+)", header)
    assert m and int(m.group(1)) == 64 == capi.DensePropagator64.MAX_R


def test_dense64_block_bad_arguments_without_device():
    """every EKF_ERR_INVALID case that needs no live handle: a NULL handle with otherwise valid arguments, and with each
    bad argument -- answered before the device is looked at"""
    _built()
    lib = capi.load()
    dp = ctypes.POINTER(ctypes.c_double)
    r = 3
    Fr = np.eye(r); Qr = np.eye(r); dx = np.ones(r)
    p = lambda a: a.ctypes.data_as(dp)
    ms = ctypes.c_double()
    INVALID = 1
    ok = dict(first=0, r=r, Fr=p(Fr), Qr=p(Qr), dx=p(dx))
    cases = [{}, {"Fr": None}, {"Qr": None}, {"dx": None}, {"Qr": None, "dx": None}, {"r": 0}, {"r": -1}, {"r": 65},
             {"r": 1 << 20}, {"first": -1}, {"first": -(1 << 30)}, {"first": (1 << 31) - 1}, {"first": -1, "r": 0}]
    for bad in cases:
        a = dict(ok, **bad)
        st = lib.ekf_dense64_propagate_block(None, a["first"], a["r"], a["Fr"], a["Qr"], a["dx"], ctypes.byref(ms))
        assert st == INVALID, (bad, st)
        assert NAME.encode() in lib.ekf_last_error()
    assert lib.ekf_dense64_propagate_block(None, 0, r, p(Fr), None, None, None) == INVALID


def test_dense_propagator64_has_propagate_block():
    assert callable(getattr(capi.DensePropagator64, "propagate_block"))
    assert capi.DensePropagator64.MAX_R == 64


def test_propagate_block_value_errors_without_device():
    """the wrapper's shape and range checks come before the library is called: an object that never got a handle"""
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._h, d._lib = 30, None, None
    I3 = np.eye(3)
    bad = [lambda: d.propagate_block(0, np.ones((3, 4))), lambda: d.propagate_block(0, np.ones(3)),
           lambda: d.propagate_block(0, np.ones((0, 0))), lambda: d.propagate_block(0, np.eye(65)),
           lambda: d.propagate_block(0, np.eye(31)), lambda: d.propagate_block(-1, I3),
           lambda: d.propagate_block(28, I3), lambda: d.propagate_block(0, I3, Qr=np.eye(4)),
           lambda: d.propagate_block(0, I3, Qr=np.ones(3)), lambda: d.propagate_block(0, I3, dx=np.ones(4)),
           lambda: d.propagate_block(0, I3, dx=np.ones((3, 1)))]
    for f in bad:
        with pytest.raises(ValueError):
            f()


def test_fixture_meets_numpy_literal_spelling():
    """tests/golden/dense_predict_ref.npz (the reference build's prediction() at n = 20): numpy's literal spelling of the
    same predictions -- dense At and Q, and the three slice updates -- meets the recorded state and Sigma at FP64_TOL, so
    a failure of the GPU replay is the kernel's"""
    import dense_block_cases as bc
    from parity import FP64_TOL, worst
    path = os.path.join(ROOT, "tests", "golden", "dense_predict_ref.npz")
    assert os.path.getsize(path) <= 100 * 1024
    z = np.load(path)
    branches = set()
    for name, twists, _ in bc.CASES:
        case = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
        assert int(case["n"]) == 20 and case["cov0"].shape == (43, 43)
        assert np.array_equal(case["twists"], np.array(twists, dtype=np.float64))
        assert np.abs(case["cov0"] - case["cov0"].T).max() > 1e-5      # rows and columns differ
        branches |= {abs(t[0]) < 1e-6 for t in twists}
        for spell in (bc.np_predict_literal, bc.np_predict_slices):
            s, c = bc.replay_case(case, spell)
            w, e = worst(s, c, case["state1"], case["cov1"])
            assert w <= FP64_TOL, (name, spell.__name__, e)
    assert branches == {True, False}                                    # both branches of ekf_slam.cpp:79
    assert len(dict((c[0], c) for c in bc.CASES)["five"][1]) == 5
