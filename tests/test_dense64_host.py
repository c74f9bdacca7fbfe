"""CPU (not gpu): the fp64 dense propagation refuses to run without a device -- there is no CPU path -- and checks its
arguments before it looks for one."""
import ctypes
import os

import pytest

from ekf_slam_ml_amd import capi


def _built():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_dense64_bad_arguments_without_device():
    _built()
    lib = capi.load()
    h = ctypes.c_void_p()
    assert lib.ekf_dense64_create(0, -1, ctypes.byref(h)) == 1        # EKF_ERR_INVALID
    assert lib.ekf_dense64_create(-3, -1, ctypes.byref(h)) == 1
    assert lib.ekf_dense64_create(5, -1, None) == 1
    assert lib.ekf_dense64_destroy(None) == 0


def test_dense64_no_cpu_fallback():
    _built()
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    h = ctypes.c_void_p()
    assert capi.load().ekf_dense64_create(5, -1, ctypes.byref(h)) == 2   # EKF_ERR_NO_DEVICE
    assert not h.value
    with pytest.raises(capi.EkfError) as e:
        capi.DensePropagator64(5)
    assert e.value.status == 2
