"""-m gpu: association decisions at ties and exact gates (tests/assoc_edge_cases.py) in every kernel form that implements
ekf_slam.cpp:293-330.  Per form x case: the decisions, the known list and the known count are the case's stated values
(by construction, not from a checker); state and Sigma agree with the CPU checker at parity.FP64_TOL; a dropped reading
leaves every bit alone; a tie's loser keeps its state entries and its rows and columns of Sigma bit for bit; and the form
under test is shown to be the one that ran.  Pools: B = 3, the edge filter is filter 1, filters 0 and 2 run an ordinary
synth.make_unknown_log world with the same parameters -- a tie in one filter leaves its neighbours' decisions alone."""
import math
from fractions import Fraction

import numpy as np
import pytest

import assoc_edge_cases as ec
from ekf_slam_ml_amd import synth
from parity import FP64_TOL, assert_parity

pytestmark = pytest.mark.gpu
WORST = {}        # per form: worst per-block parity, printed by test_zz_report
SMALL_MAX_DIM = 104   # ekf::small_max_dim()
CALL_CAPACITY = 448   # ekf::assoc_call_capacity()
CALL_V = 8            # ekf::kCallV
B, EDGE = 3, 1


def _checker(oracle, n):
    # (the DENSE checker multiplies full N x N matrices per landmark: minutes at n = 1040)
    return oracle.OracleEKF(n, oracle.DENSE if n <= 130 else oracle.STRUCTURED, params=ec.PARAMS)


def _same_bits(a, b):
    """bit-equal, NaN entries (whose payload is nobody's contract) at the same places"""
    (am, an), (bm, bn) = ec.masked(a), ec.masked(b)
    return np.array_equal(an, bn) and am.tobytes() == bm.tobytes()


def _parity(form, what, s, c, sr, cr):
    sm, nm = ec.masked(s)
    srm, nrm = ec.masked(sr)
    assert np.array_equal(nm, nrm), f"{what}: NaN entries of the state differ"
    w = assert_parity(sm, c, srm, cr, FP64_TOL, what)
    WORST[form] = max(WORST.get(form, 0.0), w)


def _check_stated(c, what, dec, kc, s0, c0, s1, c1):
    assert tuple(int(d) for d in dec) == tuple(c.decisions), f"{what}: decisions {list(dec)} vs stated {c.decisions}"
    assert kc == c.known_after, f"{what}: known count {kc} vs stated {c.known_after}"
    if c.dropped:
        assert s1.tobytes() == s0.tobytes() and c1.tobytes() == c0.tobytes(), f"{what}: a dropped reading changed something"
    for i in c.unchanged:
        r = ec.rows_of(i)
        assert s1[r].tobytes() == s0[r].tobytes() and c1[r].tobytes() == c0[r].tobytes() \
            and c1[:, r].tobytes() == c0[:, r].tobytes(), f"{what}: the loser {i} changed"
    if c.new_slot >= 0:
        assert tuple(s1[ec.rows_of(c.new_slot)]) == tuple(c.readings[-1]), f"{what}: new landmark not at the reading"


# ---- single filter -----------------------------------------------------------------------------------------------

SINGLE = [(form, cid) for form, cid in ec.all_case_ids() if not ec.FORMS[form]["pool"]]


def _single_setup(hip, form, n):
    f = hip.EKF_SLAM(n, params=hip.Params(*ec.PARAMS))
    if form in ("single_chain", "single_delayed"):
        f.set_small_map_path(False)
        f.set_call_fused(False)
        assert not f.forms & (hip.FORM_SMALL_MAP | hip.FORM_CALL_FUSED)
    else:
        assert f.forms & hip.FORM_SMALL_MAP and f.forms & hip.FORM_CALL_FUSED and f.forms & hip.FORM_ACTIVE_PREFIX
    if form == "single_delayed":
        f.set_update_mode(16)
    return f


def _single_form_ran(form, c, prof):
    """the dispatch of ekf_associate (ekf_capi.hip), from the case's own numbers, and the launch counts it leaves"""
    N, J = 3 + 2 * c.n, c.J
    carried = min(c.M + J, c.n)   # touched_hwm = 0: the map was initialised by a measurement() with nothing visible
    passes = math.ceil(J / CALL_V)
    if form == "single_inline":      # ekf_capi.hip:250
        assert N <= SMALL_MAX_DIM and J <= ec.STAGED_FILLERS
        assert prof["score_launches"] == 0 and prof["stream_launches"] == 0, prof
    elif form == "single_staged":    # :268 (and not :250)
        assert N <= SMALL_MAX_DIM and c.n <= 128 and J > ec.STAGED_FILLERS
        assert prof["score_launches"] == 0 and prof["stream_launches"] == 0, prof
    elif form == "single_prefix":    # :287
        assert N > SMALL_MAX_DIM and 3 + 2 * carried <= SMALL_MAX_DIM
        assert prof["score_launches"] == 0 and prof["stream_launches"] == 0, prof
    elif form == "single_call":      # :318: one k_assoc_call and one pass per 8 readings
        assert 3 + 2 * carried > SMALL_MAX_DIM and carried <= CALL_CAPACITY
        assert prof["score_launches"] == passes and prof["stream_launches"] == passes, prof
    elif form == "single_reading":   # :351: k_assoc_score per pass + k_assoc_reading per reading
        assert carried > CALL_CAPACITY
        assert prof["score_launches"] == passes + J and prof["stream_launches"] == passes, prof
    else:                            # :393: k_maha per reading (the call-fused and small forms are off)
        assert prof["score_launches"] == J, prof


@pytest.mark.parametrize("form,cid", SINGLE, ids=[f"{a}-{b}" for a, b in SINGLE])
def test_single_filter(hip, oracle, form, cid):
    c = ec.get_case(form, cid)
    what = f"{form} {cid}"
    f, o = _single_setup(hip, form, c.n), _checker(oracle, c.n)
    ec.init_by_measurement(f, c)
    ec.init_by_measurement(o, c)
    s0, c0 = f.state, f.cov
    assert _same_bits(s0, o.state) and c0.tobytes() == o.cov.tobytes(), f"{what}: the world is not exact"
    if form == "single_chain":   # the one place a device score is visible: its bits are the stated fractions
        m = c.readings[c.first]
        got = f.maha_scores(m, c.M)
        assert {i: Fraction(float(got[i])) for i in c.scores} == c.scores, f"{what}: device scores"
        if c.kind == "tie":
            lo, hi = sorted(c.scores)
            assert got[lo].tobytes() == got[hi].tobytes()
    f.set_profiling(True)
    known, known_o = ec.known_list(c), ec.known_list(c)
    dec = f.data_association(c.readings, known)
    prof = f.profile()
    dec_o = o.data_association(c.readings, known_o)
    s1, c1 = f.state, f.cov
    assert np.array_equal(known, known_o) and known[:c.known_after].all(), f"{what}: known list"
    assert np.array_equal(dec, dec_o), f"{what}: decisions {dec} vs the checker's {dec_o}"
    _check_stated(c, what, dec, int(known.sum()), s0, c0, s1, c1)
    _parity(form, what, s1, c1, o.state, o.cov)
    _single_form_ran(form, c, prof)
    f.close()


# ---- pools -------------------------------------------------------------------------------------------------------

POOL = [(form, cid) for form, cid in ec.all_case_ids() if ec.FORMS[form]["pool"]]
_ORDINARY = {}


def _ordinary(oracle, n):
    """filters 0 and 2, once per map size: a surveyed synth world, one step of shuffled readings, and what the checker
    makes of it -> (init[B, 2n], log, {b: (decisions, known count, state, cov)})"""
    if n not in _ORDINARY:
        half = 0.16 * math.sqrt(n) + 1.0
        cfg = synth.SimConfig(n=n, steps=1, filters=B, seed=909 + n, half_extent=half, min_spacing=0.2,
                              max_visible_dis=0.8, vmax=CALL_V)
        log = synth.make_unknown_log(cfg)
        init = (log.world[None] + np.random.default_rng(n).normal(0, 0.005, size=(B, n, 2))).reshape(B, 2 * n)
        res = {}
        for b in (0, 2):
            o = _checker(oracle, n)
            o.prediction(0.0, 0.0)
            o.measurement(init[b], np.zeros(n, dtype=np.uint8))
            known = np.ones(n, dtype=np.uint8)
            o.prediction(*log.twist[0, b])
            dec = o.data_association(log.meas_xy[0, b, :int(log.count[0, b])], known)
            res[b] = (dec.copy(), int(known.sum()), o.state, o.cov)
        assert sum(int(log.count[0, b]) for b in (0, 2)) > 0, "the ordinary filters see nothing"
        _ORDINARY[n] = (init, log, res)
    return _ORDINARY[n]


def _pool_setup(hip, form, n):
    bt = hip.BatchEKF(B, n, params=hip.Params(*ec.PARAMS))
    if form == "pool_small":
        assert bt.forms & hip.FORM_SMALL_MAP and bt.forms & hip.FORM_ACTIVE_PREFIX
        return bt
    bt.set_small_map_path(False)
    assert not bt.forms & hip.FORM_SMALL_MAP
    if form.startswith("pool_fused"):
        bt.set_step_fused({"pool_fused_off": 0, "pool_fused_auto": 1, "pool_fused_always": 2}[form])
    else:
        bt.set_update_mode(32)
        on = form == "pool_delayed_spec"
        bt.set_forms(bt.forms | hip.FORM_STEP_SPECULATE if on else bt.forms & ~hip.FORM_STEP_SPECULATE)
        assert bool(bt.forms & hip.FORM_STEP_SPECULATE) == on
    return bt


def _pool_form_ran(hip, form, c, bt, before, updates):
    """the dispatch of ekf_batch_run_unknown (ekf_capi_batch.hip) from the case's own numbers, and its counters"""
    fc = bt.form_counts()
    d = {k: fc[k] - before[k] for k in fc}
    N = 3 + 2 * c.n
    if form == "pool_small":           # ekf_capi_batch.hip:514: Nstep <= small_max_dim() whatever the counts
        assert N <= SMALL_MAX_DIM and d["step_split_passes"] == 0 and d["rank2_streams"] == 0, d
    elif form == "pool_fused_off":     # :589: four launches per slot
        assert not bt.forms & hip.FORM_STEP_FUSED and d["step_split_passes"] == 0, d
    elif form == "pool_fused_auto":    # :559: fresh counts, Nstep >= 603, >= 70 % real work -> the split pass
        real = 2 * N * N + (3 + 2 * min(c.M + c.J, c.n)) ** 2   # (filters 0 and 2 hold full maps)
        assert N >= 603 and real >= 0.7 * B * N * N
        assert bt.forms & hip.FORM_STEP_SPLIT_PASS and d["step_split_passes"] == 1, d
    elif form == "pool_fused_always":  # :578: one launch, the pass inside
        assert bt.forms & hip.FORM_STEP_FUSED and not bt.forms & hip.FORM_STEP_SPLIT_PASS and d["step_split_passes"] == 0, d
    else:                              # :525: the delayed step kernel, flushed at the end of the run (:617)
        assert c.J <= CALL_V and 2 * CALL_V <= 64
        assert d["step_split_passes"] == 1 and d["flush_plain"] + d["flush_strip"] + d["flush_mirrored"] >= 1, d
        eligible, hits = bt.spec_counts()
        if form == "pool_delayed_spec":
            assert eligible >= updates and hits <= eligible, (eligible, hits, updates)
        else:
            assert (eligible, hits) == (0, 0)


@pytest.mark.parametrize("form,cid", POOL, ids=[f"{a}-{b}" for a, b in POOL])
def test_pool(hip, oracle, form, cid):
    c = ec.get_case(form, cid)
    what = f"{form} {cid}"
    n = c.n
    init, log, ordinary = _ordinary(oracle, n)
    init = init.copy()
    init[EDGE] = c.world.reshape(-1)
    bt = _pool_setup(hip, form, n)
    # the pattern of test_pool_run_unknown_against_reference: a one-step known log that only initialises, then the counts
    bt.upload_known_log(np.zeros((1, B, 2)), np.full((1, B, 1), -1, dtype=np.int32), np.zeros((1, B, 1, 2)), init)
    bt.run_known()
    bt.set_known_counts([n, c.M, n])
    o = _checker(oracle, n)
    o.prediction(0.0, 0.0)
    ec.init_by_measurement(o, c)
    s0, c0 = bt.state(EDGE), bt.cov(EDGE)
    assert _same_bits(s0, o.state) and c0.tobytes() == o.cov.tobytes(), f"{what}: the world is not exact"
    twist, count, meas = log.twist.copy(), log.count.copy(), log.meas_xy.copy()
    twist[0, EDGE], count[0, EDGE] = 0.0, c.J
    meas[0, EDGE] = 0.0
    meas[0, EDGE, :c.J] = c.readings
    before = bt.form_counts()
    bt.upload_unknown_log(twist, count, meas)
    bt.run_unknown(0, 1)
    dec_all, kc = bt.decisions(), bt.known_counts()
    known_o = ec.known_list(c)
    o.prediction(0.0, 0.0)
    dec_o = o.data_association(c.readings, known_o)
    dec = dec_all[0, EDGE, :c.J]
    s1, c1 = bt.state(EDGE), bt.cov(EDGE)
    assert np.array_equal(dec, dec_o), f"{what}: decisions {dec} vs the checker's {dec_o}"
    assert int(kc[EDGE]) == int(known_o.sum()) and known_o[:int(kc[EDGE])].all()
    _check_stated(c, what, dec, int(kc[EDGE]), s0, c0, s1, c1)
    _parity(form, what, s1, c1, o.state, o.cov)
    updates = sum(1 for d in c.decisions if d >= 0 and d != c.new_slot)
    for b in (0, 2):   # the neighbours: the checker's decisions, untouched by the edge filter's tie
        d_b, kc_b, s_b, c_b = ordinary[b]
        assert np.array_equal(dec_all[0, b, :len(d_b)], d_b), f"{what}: filter {b} decisions"
        assert int(kc[b]) == kc_b
        _parity(form, f"{what} filter {b}", bt.state(b), bt.cov(b), s_b, c_b)
        updates += int((d_b >= 0).sum())
    _pool_form_ran(hip, form, c, bt, before, updates)
    bt.close()


def test_zz_report():
    """the worst per-block parity by form (printed with -s / in the log)"""
    for k in sorted(WORST):
        print(f"assoc edges worst parity {k}: {WORST[k]:.3e}")
    assert all(v <= FP64_TOL for v in WORST.values())
