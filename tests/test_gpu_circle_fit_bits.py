"""GPU: the two circle-fit kernels against their own recorded bytes.  tests/golden/circle_fit_bits.npz holds 29 scans and what
k_circles (circle_fit_scans at S = 1) and k_scan_circles (DensePropagator64.fit_scan) made of them when the fit was moved
into ekf_circle_fit.hpp (tests/golden/make_circle_fit_bits_golden.py, recorded on the commit before): the circle count, the
cluster count, the centres, the radii and every cluster's row.  Both kernels are compiled with -ffp-contract=off and every
sum has a fixed order, so the answer to a change of the shared source that is meant to keep the arithmetic is the same bytes,
not a tolerance.  The scan with NaN and inf ranges is held to the same NaN positions and the same bytes elsewhere (a NaN's
payload is not part of the contract); every other scan to the same bytes throughout."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MAX_OUT = 32
NONFINITE = "nan_inf"


@pytest.fixture(scope="module")
def rec():
    """the fixture cut back into scans: [(name, ranges, {kernel: (centres, radii, all)})]"""
    z = np.load(os.path.join(HERE, "golden", "circle_fit_bits.npz"))
    ranges = np.split(z["ranges"], np.cumsum(z["nb"])[:-1])
    want = {}
    for k in ("lane", "wave"):
        cnt, ncl = np.cumsum(z[k + "_count"])[:-1], np.cumsum(z[k + "_clusters"])[:-1]
        want[k] = list(zip(np.split(z[k + "_centres"], cnt), np.split(z[k + "_radii"], cnt), np.split(z[k + "_all"], ncl)))
    out = [(str(name), np.ascontiguousarray(r), {k: want[k][i] for k in want}) for i, (name, r) in enumerate(zip(z["names"], ranges))]
    assert len(out) == 29 and sum(name == NONFINITE for name, _, _ in out) == 1
    assert any(len(w["lane"][0]) for _, _, w in out) and any(len(w["wave"][2]) > 4 for _, _, w in out)
    return out


def _same(name, what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{name}: {what} has shape {got.shape}, recorded {want.shape}"   # the two counts
    assert got.dtype == want.dtype == np.float64
    if name == NONFINITE:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{name}: {what}: NaN positions"
        got, want = np.where(nan, 0.0, got), np.where(nan, 0.0, want)
    assert got.tobytes() == want.tobytes(), f"{name}: {what} differs at {np.argwhere(got.view(np.int64) != want.view(np.int64))[:4].tolist()}"


def _hold(name, got, want):
    for what, g, w in zip(("centres", "radii", "clusters"), got, want):
        _same(name, what, g, w)


def test_k_scan_circles(hip, rec):
    d = hip.DensePropagator64(23)
    for name, r, want in rec:
        _hold(name, d.fit_scan(r, max_out=MAX_OUT, want_all=True)[:3], want["wave"])
    d.close()


def test_k_circles_one_scan_a_launch(hip, rec):
    for name, r, want in rec:
        cen, rad, allc = hip.circle_fit_scans(r, max_out=MAX_OUT, want_all=True)
        _hold(name, (cen[0], rad[0], allc[0]), want["lane"])


def test_k_circles_in_a_batch(hip, rec):
    """all scans of 360 beams in one launch: blocks other than 0, and a scan's result does not depend on its neighbours"""
    batch = [(name, r, want) for name, r, want in rec if len(r) == 360]
    assert len(batch) == 19
    cen, rad, allc = hip.circle_fit_scans(np.stack([r for _, r, _ in batch]), max_out=MAX_OUT, want_all=True)
    for s, (name, _, want) in enumerate(batch):
        _hold(name, (cen[s], rad[s], allc[s]), want["lane"])
