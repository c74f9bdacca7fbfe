"""CPU (not gpu): the joint association of the fp64 dense handle (ekf_dense64_score_readings, ekf_dense64_joint_operands,
ekf_dense64_associate_joint, ekf_dense64_associate_scan_joint) is exported, declared and bound; the joint rule as a function
keeps its edges (a conflict, equal scores, a NaN candidate, a full map, more new readings than slots); with one reading per
call the numpy model is lc.np_associate bit for bit; on the scan fixture the joint and the sequential model decide alike with
every deciding score away from both gates; a NULL handle is refused before anything else, without a device."""
import ctypes as C
import os
import re

import numpy as np

import dense_block_cases as bc
import dense_init_cases as ic
import dense_joint_cases as jc
import dense_landmark_cases as lc
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = (("ekf_dense64_score_readings", 9), ("ekf_dense64_joint_operands", 9), ("ekf_dense64_associate_joint", 11),
           ("ekf_dense64_associate_scan_joint", 13))
INVALID = 1


def _built():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_dense64_joint_symbols_exported_and_declared():
    _built()
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in SYMBOLS:
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
        m = re.search(r"ekf_status\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(getattr(lib, name).argtypes), (name, m.group(1))
    for macro, value in (("EKF_DENSE64_JOINT_MAX_READINGS", 128), ("EKF_DENSE64_JOINT_MAX_PAIRS", 30)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, header)
        assert m and int(m.group(1)) == value, macro
    P = capi.DensePropagator64
    assert (P.JOINT_MAX_READINGS, P.JOINT_MAX_PAIRS) == (jc.MAX_READINGS, jc.MAX_PAIRS) == (128, 30)
    for name in ("score_readings", "joint_operands", "associate_joint", "associate_scan_joint"):
        assert callable(getattr(P, name)), name
    assert callable(capi.DenseEKFSLAM.joint_association)


def test_null_handle_is_refused_first():
    """a NULL handle comes first in every call's order: EKF_ERR_INVALID although every other argument is bad as well"""
    _built()
    lib = capi.load()
    assert lib.ekf_dense64_score_readings(None, None, 0, None, -1, 0, None, None, None) == INVALID
    assert lib.ekf_dense64_joint_operands(None, None, 0, None, None, None, None, None, None) == INVALID
    assert lib.ekf_dense64_associate_joint(None, None, 0, None, -1, None, 4, None, None, None, None) == INVALID
    assert lib.ekf_dense64_associate_scan_joint(None, None, None, 0, 0, -1, None, 4, None, None, None, None, None) == INVALID
    z, k = (C.c_double * 2)(1.0, 1.0), C.c_int(0)
    assert lib.ekf_dense64_associate_joint(None, None, 1, z, 1, C.byref(k), 0, None, None, None, None) == INVALID
    assert k.value == 0


def test_joint_rule_edges():
    nan = float("nan")
    # a conflict: both readings claim landmark 1, the lower score keeps it
    assert jc.joint_rule([[5.0, 0.5], [5.0, 0.25]], 2, 9)[:2] == (["drop", "match"], [-1, 1])
    # equal scores: the lower j keeps it
    assert jc.joint_rule([[0.25, 5.0], [0.25, 5.0]], 2, 9)[:2] == (["match", "drop"], [0, -1])
    # the loser is dropped although another landmark is under its gate too: one assignment, no second choice
    assert jc.joint_rule([[0.2, 0.3], [0.1, 0.9]], 2, 9)[:2] == (["drop", "match"], [-1, 0])
    # a NaN candidate never wins and disturbs nobody; the first of equal scores inside a row wins
    assert jc.joint_rule([[nan, 0.3, 0.3]], 3, 9)[:2] == (["match"], [1])
    kinds, lms, best = jc.joint_rule([[nan, nan]], 2, 9)
    assert (kinds, lms, best) == (["new"], [2], [10.0])
    # between the gates: dropped, best is the score; a full map with nothing under gate_new: dropped, best is the gate
    assert jc.joint_rule([[5.0, 2.0]], 2, 9) == (["drop"], [-1], [2.0])
    assert jc.joint_rule([[12.0, 11.0], [12.0, 0.5]], 2, 2) == (["drop", "match"], [-1, 1], [10.0, 0.5])
    # more new readings than slots: ascending j takes them, the rest drop; nothing known: every reading is new
    assert jc.joint_rule([[], [], []], 0, 2)[:2] == (["new", "new", "drop"], [0, 1, -1])
    assert jc.joint_rule([[20.0], [0.5], [30.0], [40.0]], 1, 3)[:2] == (["new", "match", "new", "drop"], [1, 0, 2, -1])
    # the pairs: MATCH and NEW in ascending j; MATCH only with a gate_update <= 0 (which then matches nothing)
    kinds, lms, _ = jc.joint_rule([[20.0], [0.5], [30.0]], 1, 3)
    assert jc.pairs_of(kinds, lms) == [(0, 1), (1, 0), (2, 2)]
    kinds, lms, _ = jc.joint_rule([[20.0], [0.5]], 1, 3, gate_update=0.0)
    assert kinds == ["new", "drop"] and jc.pairs_of(kinds, lms, 0.0) == []
    assert [len(g) for g in jc.groups_of(list(range(31)))] == [30, 1]


def test_joint_edges_on_a_numpy_handle():
    """the full map (a far reading dropped, one corrected) and a conflict through the whole model: the loser writes nothing"""
    x, S, far, on = lc.full_map_fixture()
    d = jc.numpy_handle(x, S)
    known, assoc, best, ng = jc.np_associate_joint(d, None, [far, on], 4, 4)
    assert known == 4 and list(assoc) == [-1, 2] and best[0] == 10.0 and best[1] < 1.0 and ng == 1
    x, S = lc.spiral_map(6)
    near, nearer = lc.reading_of(x, 3, (0.02, 0.0)), lc.reading_of(x, 3, (0.002, 0.0))
    d, one = jc.numpy_handle(x, S), jc.numpy_handle(x, S)
    known, assoc, best, _ = jc.np_associate_joint(d, None, [near, nearer], 6, 6)
    assert list(assoc) == [-1, 3] and best[1] < best[0] < 1.0
    jc.np_associate_joint(one, None, [nearer], 6, 6)
    assert d.state.tobytes() == one.state.tobytes() and d.sigma.tobytes() == one.sigma.tobytes()


def test_one_reading_per_call_is_the_sequential_model_bit_for_bit():
    """the discovery scenario, every reading its own joint call, against lc.np_associate with the tick's readings"""
    n = 20
    N = 3 + 2 * n
    a, b = ic.NumpyHandle(N), ic.NumpyHandle(N)
    x0, S0 = ic.stale_start(n)
    for d in (a, b):
        d.set(S0)
        d.state = x0.copy()
    ka = kb = 0
    for dth, dx, readings in ic.discovery_scenario():
        for d in (a, b):
            Fr, Qr, upd = bc.model_operands(d.state_block(0, 3), dth, dx)
            d.propagate_block(0, Fr, Qr, upd)
        ka, want, want_best = lc.np_associate(a, None, readings, ka, n)
        got, got_best = [], []
        for z in readings:
            kb, assoc, best, ng = jc.np_associate_joint(b, None, [z], kb, n)
            got.append(int(assoc[0]))
            got_best.append(float(best[0]))
            assert ng == (1 if assoc[0] >= 0 else 0)
        assert ka == kb and got == list(want) and np.array(got_best).tobytes() == want_best.tobytes()
        assert a.state.tobytes() == b.state.tobytes() and a.sigma.tobytes() == b.sigma.tobytes()
    assert ka == n


def joint_vs_sequential():
    """the scan fixture through both numpy models, tick after tick -> [(joint assoc, sequential assoc)], the joint model's
    score matrices with the decisions made on them, and the two handles"""
    x, S, known, steps = jc.scan_fixture()
    n_max = (len(x) - 3) // 2
    a, b = jc.numpy_handle(x, S), jc.numpy_handle(x, S)
    ka = kb = known
    decisions, scored, seq_scores = [], [], []
    for dth, dx, readings in steps:
        for d in (a, b):
            Fr, Qr, upd = bc.model_operands(d.state_block(0, 3), dth, dx)
            d.propagate_block(0, Fr, Qr, upd)
        scores = []
        k0 = ka
        ka, ja, best, _ = jc.np_associate_joint(a, None, readings, ka, n_max, scores=scores)
        kb, sa, _ = lc.np_associate(b, None, readings, kb, n_max, scores=seq_scores)
        assert ka == kb
        decisions.append((list(ja), list(sa)))
        scored.append((scores[0], jc.joint_rule(scores[0], k0, n_max)))
    return decisions, scored, seq_scores, a, b


def test_joint_and_sequential_decide_alike_away_from_the_gates():
    decisions, scored, seq_scores, a, b = joint_vs_sequential()
    assert len(decisions) >= 4
    for t, (ja, sa) in enumerate(decisions):
        assert ja == sa, (t, ja, sa)
        assert sorted(ja)[:8] == [0, 1, 2, 3, 5, 6, 8, 9] and ja[8] == 10 + t, (t, ja)   # 8 matches and one new landmark
    for nis, (kinds, _, best) in scored:
        assert jc.margins_ok(nis, kinds, best), np.sort(nis, axis=1)[:, :2]
    for row in seq_scores:                                  # the sequential rule's deciding scores keep the margin too
        m = float(np.nanmin(row))
        assert all(abs(m - g) >= jc.MARGIN * g for g in (10.0, 1.0)), m
    # the two are different filters: close, and not the same bits
    assert a.state.tobytes() != b.state.tobytes()
    assert np.abs(a.state - b.state).max() < 1e-2
