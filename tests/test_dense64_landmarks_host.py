"""CPU (not gpu): the landmark front end of the fp64 dense handle (ekf_dense64_score_landmarks,
ekf_dense64_associate_landmarks) is exported, declared and bound; the decision rule as a function keeps the reference's
edges (first of equals, NaN never wins, an empty or all-NaN vector, the full map); the numpy model of the call equals the
spelled loop of dense_init_cases bit for bit and meets the reference's own data_association(), so a failure of the GPU
replay is the kernels'."""
import os
import re

import numpy as np
import pytest

import dense_block_cases as bc
import dense_init_cases as ic
import dense_landmark_cases as lc
import dense_score_cases as ds
import dense_sparse_cases as sp
from ekf_slam_ml_amd import capi
from parity import FP64_TOL, worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE, ASSOC = "ekf_dense64_score_landmarks", "ekf_dense64_associate_landmarks"


def _built():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_dense64_landmark_symbols_exported_and_declared():
    _built()
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in ((SCORE, 13), (ASSOC, 10)):
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
        m = re.search(r"ekf_status\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(getattr(lib, name).argtypes), (name, m.group(1))
    for flag, value in (("EKF_DENSE64_LM_DEFERRED", 1), ("EKF_DENSE64_LM_GROW_LIVE", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)u" % flag, header)
        assert m and int(m.group(1)) == value
    assert (capi.DensePropagator64.LM_DEFERRED, capi.DensePropagator64.LM_GROW_LIVE) == (1, 2)
    for name in ("score_landmarks", "associate_landmarks"):
        assert callable(getattr(capi.DensePropagator64, name))


def test_rule_edges():
    nan = float("nan")
    assert lc.rule([0.5, 0.25, 0.25, 3.0], 4, 9) == (1, "update", 0.25)              # the first of equals
    assert lc.rule([0.25, nan, 0.25], 3, 9)[0] == 0 and lc.rule([nan, 0.3, 0.2], 3, 9)[:2] == (2, "update")
    assert lc.rule([nan, nan], 2, 9) == (2, "new", 10.0) and lc.rule([], 0, 9) == (0, "new", 10.0)
    assert lc.rule([], 0, 0) == (-1, "drop", 10.0) and lc.rule([nan], 1, 1) == (-1, "drop", 10.0)
    assert lc.rule([5.0, 2.0], 2, 9) == (-1, "drop", 2.0)                            # between the gates
    assert lc.rule([12.0, 11.0], 2, 2) == (-1, "drop", 10.0)                         # the full map, nothing under the gate
    assert lc.rule([12.0, 0.5], 2, 2) == (1, "update", 0.5)
    assert lc.rule([-0.0, 0.0], 2, 2)[0] == 0                                         # equal as numbers: the first


def test_fixtures_in_numpy():
    """the tie fixture gives equal score bits that are the strict minimum of the others, the NaN candidate is NaN, the
    full-map fixture drops the far reading and corrects landmark 2"""
    for count, a, b in ((5, 0, 1), (70, 62, 65), (260, 254, 257)):
        nan_at = a + 1 if b != a + 1 else b + 1
        x, S, (sx, sy) = lc.tie_fixture(count, a, b, nan_at)
        cols, Hc, R, nu = sp.candidate_terms(x, sx, sy)
        with np.errstate(all="ignore"):
            nis = np.array([ds.np_scores(S[np.ix_(c, c)], h[None], R, n[None])[1][0] for c, h, n in zip(cols, Hc, nu)])
        assert nis[a].tobytes() == nis[b].tobytes() and np.isnan(nis[nan_at])
        rest = np.delete(nis, [a, b, nan_at])
        assert nis[a] < 1.0 and (rest > nis[a]).all()
        assert lc.rule(nis, count, count)[:2] == (a, "update")
    x, S, far, on = lc.full_map_fixture()
    d = ic.NumpyHandle(len(x))
    d.set(S)
    d.state = x.copy()
    known, assoc, best = lc.np_associate(d, None, [far, on], 4, 4)
    assert known == 4 and list(assoc) == [-1, 2] and best[0] == 10.0 and best[1] < 1.0


def test_model_equals_the_spelled_loop_bit_for_bit():
    """one tick of ic.association_step (propagate_block, then per reading the spelled loop) against propagate_block +
    np_associate on a twin: known, state and Sigma in bits, tick after tick"""
    n = 20
    N = 3 + 2 * n
    a, b = ic.NumpyHandle(N), ic.NumpyHandle(N)
    x0, S0 = ic.stale_start(n)
    for d in (a, b):
        d.set(S0)
        d.state = x0.copy()
    ka = kb = 0
    for dth, dx, readings in ic.discovery_scenario():
        ka = ic.association_step(a, n, ka, dth, dx, readings, "init_block")
        Fr, Qr, upd = bc.model_operands(b.state_block(0, 3), dth, dx)
        b.propagate_block(0, Fr, Qr, upd)
        kb, assoc, _ = lc.np_associate(b, None, readings, kb, n)
        assert ka == kb and (assoc >= 0).all()
        assert a.state.tobytes() == b.state.tobytes() and a.sigma.tobytes() == b.sigma.tobytes()
    assert ka == n


def test_model_against_the_reference_data_association(oracle):
    """np_associate against the reference's own data_association() on the discovery scenario at n = 20: the same `known`
    after every tick, state and Sigma within FP64_TOL, every scored vector with its margins"""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    n = 20
    ref = oracle.RefEKF(n)
    known_ref = np.zeros(n, dtype=np.uint8)
    d = ic.NumpyHandle(3 + 2 * n)
    x0, S0 = ic.prior_start(n)
    d.set(S0)
    d.state = x0
    known, scores = 0, []
    for dth, dx, readings in ic.discovery_scenario():
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        Fr, Qr, upd = bc.model_operands(d.state_block(0, 3), dth, dx)
        d.propagate_block(0, Fr, Qr, upd)
        known, _, _ = lc.np_associate(d, None, readings, known, n, scores=scores)
        assert known == int(known_ref.sum()) and known_ref[:known].all(), (known, known_ref)
    assert known == n and all(ds.margins_hold(s) for s in scores)
    w, e = worst(d.state, d.sigma, ref.state, ref.cov)
    assert w <= FP64_TOL, e
