"""-m gpu: every pool form through the motion model's branches and wraps (tests/pool_motion_cases.py; its inputs are proved on
the CPU by tests/test_pool_motion_cases_host.py).

A pool of B = 7 filters, one per motion family -- both sides of the 1e-6 gate of prediction() (ekf_slam.cpp:79), dtheta and dx
of both signs, turning in place (a10 = a20 = 0 exactly), zero twists (At = I), a heading several turns outside (-pi, pi],
readings from behind the robot whose raw bearing difference lies beyond +-pi (:187), runs of silent steps of mixed branches --
so ONE launch of k_predict and of every gain kernel holds all of them.  n = 50 (the LDS-resident paths), n = 130 (N = 263: the
mirrored flush and the column panel exist) and n = 300 (run_unknown beyond the small path from its first steps), T = 18.

Known association: every form, as one run and cut into (0, 4), (4, 5), (5, 11), (11, T) so that column panels, pending factors
and the accumulated prediction map of FORM_CURRENT_COLUMNS are handed across run boundaries -- one of them inside a silent run.
The chained pass exists only where one correction takes the tile queue, which no pool of B = 7 does: it runs on the n = 300
case with the seven families repeated to B = 112.  Unknown association: on the empty map and on a surveyed map.  Every filter of every run against OracleEKF(STRUCTURED) at
FP64_TOL per block (for unknown logs decisions and known counts first); where set_forms() promises the same bits for two forms
they are compared bit for bit over the same run boundaries, FORM_CURRENT_COLUMNS against its rebuilt form at the 1e-10 of
tests/test_gpu_delayed.py.  Every test shows through form_counts() / forms / rank2_kernel() / spec_counts() that the form it
names ran.  test_zz_report prints the worst error per (form, family): profiles/r35/pool_motion.txt."""
import hashlib

import numpy as np
import pytest

import pool_motion_cases as pm
from parity import FP64_TOL, assert_parity

pytestmark = pytest.mark.gpu

PLANS = {"one_run": ((0, pm.T),), "four_runs": pm.CUTS}
WORST = {}      # (kind, form, family) -> worst per-block error against the checker
NOTES = {}      # what ran, for the report
_KEEP_COV = ("delayed8", "delayed8_panel_on")   # the pair compared at 1e-10 needs the matrices, every other pair their digests


def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _note(key, w):
    WORST[key] = max(WORST.get(key, 0.0), w)


# ---- the checker, once per case ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def checker(oracle):
    """(kind, n) -> per filter (state, cov[, decisions, known count]); computed once, shared, left unchanged"""
    done = {}

    def get(kind, n):
        if (kind, n) not in done:
            c = pm.make_case(n)
            out = []
            for b in range(pm.B):
                o = oracle.OracleEKF(n, oracle.STRUCTURED)
                if kind == "known":
                    pm.replay_known(o, c, b)
                    out.append((o.state, o.cov))
                else:
                    known = pm.survey(o, c, b) if kind == "surveyed" else np.zeros(n, dtype=np.uint8)
                    dec = pm.replay_unknown(o, c, b, known)
                    kc = int(known.sum())
                    assert known[:kc].all()
                    out.append((o.state, o.cov, dec, kc))
            done[kind, n] = out
        return done[kind, n]
    return get


# ---- known association ---------------------------------------------------------------------------------------------------

def _delayed(k, pairing=True, sym=False, strip=False, forms=None):
    def configure(hip, bt):
        if forms is not None:
            bt.set_forms(forms(hip))
        if strip:
            bt.set_strip_flush("always")
        bt.set_update_mode(k, symmetric_gather=sym)
        bt.set_delayed_pairing(pairing)
    return configure


def _eager(call_fused=True, active=False, small=True):
    def configure(hip, bt):
        bt.set_call_fused(call_fused)
        if not small:
            bt.set_small_map_path(False)
        if active:
            bt.set_active_set(True)
    return configure


def _nocur(hip):
    return hip.FORMS_DEFAULT & ~hip.FORM_CURRENT_COLUMNS


KNOWN_FORMS = {
    "default": lambda hip, bt: None,
    "call_fused_off": _eager(call_fused=False),
    "per_correction": _eager(call_fused=False, small=False),      # k_gain + one rank-2 stream per landmark at every n
    "active_set": _eager(active=True),
    "delayed3_pair": _delayed(3, True),
    "delayed3_nopair": _delayed(3, False),
    "delayed32_pair": _delayed(32, True),
    "delayed32_nopair": _delayed(32, False),
    "delayed8_sym": _delayed(8, sym=True),
    "delayed8": _delayed(8),                                       # = column panel on, FORM_CURRENT_COLUMNS on (the default)
    "delayed8_strip": _delayed(8, strip=True),                     # FORM_STRIP_FLUSH_ALWAYS
    "delayed8_panel_on": _delayed(8, forms=_nocur),                # = FORM_CURRENT_COLUMNS off (the rebuilt form)
    "delayed8_panel_off": _delayed(8, forms=lambda hip: _nocur(hip) & ~hip.FORM_COLUMN_PANEL),
    "delayed8_one_slot": _delayed(8, forms=lambda hip: _nocur(hip) | hip.FORM_COLUMN_PANEL_ONE_SLOT),
}
# the same bits (set_forms()'s list), over the same run boundaries: form -> the form it must equal
KNOWN_SAME_BITS = {"call_fused_off": "default", "per_correction": "default", "active_set": "default",
                   "delayed8_strip": "delayed8", "delayed8_panel_on": "delayed8_panel_off", "delayed8_one_slot": "delayed8_panel_off"}
_known_runs = {}


def _known_run(hip, n, form, plan, fresh=False):
    """-> (what the tests compare, the covariances).  A test runs the form it names itself (fresh); the form it is compared
    with comes from an earlier run where there is one (its covariances kept as digests, in full only for _KEEP_COV)"""
    key = (n, form, plan)
    if fresh or key not in _known_runs:
        c = pm.make_case(n)
        bt = hip.BatchEKF(pm.B, n)
        KNOWN_FORMS[form](hip, bt)
        bt.upload_known_log(*c.known_log())
        corrections = sum(bt.run_known(t0, t1)["corrections"] for t0, t1 in PLANS[plan])
        assert corrections == int((c.lm_idx >= 0).sum())
        cov = [bt.cov(b) for b in range(pm.B)]
        _known_runs[key] = {"state": [bt.state(b) for b in range(pm.B)], "digest": [_digest(x) for x in cov],
                            "cov": cov if form in _KEEP_COV else None, "counts": bt.form_counts(), "forms": bt.forms,
                            "kernel": bt.rank2_kernel()[0], "chain": bt.chain_counts(), "touched": bt.touched()}
        bt.close()
        return _known_runs[key], cov
    return _known_runs[key], _known_runs[key]["cov"]


def _the_form_ran(hip, n, form, plan, r):
    """loud, never a skip"""
    N, fc, forms = 3 + 2 * n, r["counts"], r["forms"]
    flushes = fc["flush_plain"] + fc["flush_strip"] + fc["flush_mirrored"]
    small = N <= 104                                   # the LDS-resident run (k_pool_run_known) takes these pools whole
    if form == "default":
        assert forms == hip.FORMS_DEFAULT
        assert fc["rank2_streams"] == 0 and (fc["call_fused_passes"] == 0 if small else fc["call_fused_passes"] > 0), fc
    elif form == "call_fused_off":
        assert not forms & hip.FORM_CALL_FUSED
        assert small or (fc["rank2_streams"] > 0 and fc["call_fused_passes"] == 0), fc
    elif form == "per_correction":
        assert not forms & (hip.FORM_CALL_FUSED | hip.FORM_SMALL_MAP)
        assert fc["rank2_streams"] > 0 and fc["call_fused_passes"] == 0, fc
    elif form == "active_set":
        assert 0 < r["touched"].max() < n and fc["call_fused_passes"] == 0, (r["touched"], fc)
    else:
        assert flushes >= 2, fc
        assert (fc["gain_pairs"] == 0) == (form.endswith("_nopair")), fc
        if form == "delayed8_sym":
            assert (fc["flush_mirrored"] == flushes) if N >= 256 else fc["flush_mirrored"] == 0, fc
        if form == "delayed8_strip":
            assert forms & hip.FORM_STRIP_FLUSH_ALWAYS and fc["flush_strip"] == flushes, fc
        elif form.startswith("delayed8") and form != "delayed8_sym":   # (16 pending vectors: never the strip form by itself)
            assert fc["flush_strip"] == 0 and fc["flush_plain"] == flushes, fc
        panel = N >= 256 and form not in ("delayed8_sym", "delayed8_panel_off")     # (no panel below N = 256, none with the symmetric option)
        assert (fc["gain_from_panel"] > 0) == panel, (form, fc)
        if form.startswith("delayed8_panel") or form == "delayed8_one_slot":
            assert not forms & hip.FORM_CURRENT_COLUMNS
            assert bool(forms & hip.FORM_COLUMN_PANEL) == (form != "delayed8_panel_off")
            assert bool(forms & hip.FORM_COLUMN_PANEL_ONE_SLOT) == (form == "delayed8_one_slot")
        if form == "delayed8":
            assert forms & hip.FORM_CURRENT_COLUMNS and forms & hip.FORM_COLUMN_PANEL


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("form", list(KNOWN_FORMS))
@pytest.mark.parametrize("n", pm.SHAPES)
def test_known_forms_on_the_motion_families(hip, checker, n, form, plan):
    r, cov = _known_run(hip, n, form, plan, fresh=True)
    _the_form_ran(hip, n, form, plan, r)
    ref = checker("known", n)
    for b, fam in enumerate(pm.FAMILIES):
        w = assert_parity(r["state"][b], cov[b], ref[b][0], ref[b][1], FP64_TOL, f"n={n} {form} {plan}, filter {b} ({fam}) vs checker")
        _note(("known", form, fam), w)
    spin = pm.FAMILIES.index("spin")
    assert abs(r["state"][spin][0]) > 3 * np.pi       # the heading handed back is the unwrapped one (:99)
    NOTES["known", n, form, plan] = f"{r['counts']} chain {r['chain']} {r['kernel']}"
    if form in KNOWN_SAME_BITS:
        other, _ = _known_run(hip, n, KNOWN_SAME_BITS[form], plan)
        for b, fam in enumerate(pm.FAMILIES):
            assert np.array_equal(r["state"][b], other["state"][b]), f"n={n} {form} vs {KNOWN_SAME_BITS[form]} {plan}: state of filter {b} ({fam})"
            assert r["digest"][b] == other["digest"][b], f"n={n} {form} vs {KNOWN_SAME_BITS[form]} {plan}: Sigma of filter {b} ({fam})"
    if form == "delayed8":          # FORM_CURRENT_COLUMNS against its rebuilt form: another association of the same sums
        other, ocov = _known_run(hip, n, "delayed8_panel_on", plan)
        for b, fam in enumerate(pm.FAMILIES):
            ds = np.abs(r["state"][b] - other["state"][b]).max()
            dc = np.abs(cov[b] - ocov[b]).max() / np.abs(ocov[b]).max()
            _note(("known", "current_columns_vs_rebuilt", fam), max(ds, dc))
            assert ds < 1e-10 and dc < 1e-10, f"n={n} {plan}: current columns vs rebuilt, filter {b} ({fam}): {ds:.2e} {dc:.2e}"


# The chained pass (k_rank2_chain, FORM_STEP_CHAIN) is the tile queue's: a pool chains only where ONE correction takes
# k_rank2_queue -- 256-lane workgroups (N >= 385) and at least 16 tiles per CU (csrc/ekf_rank2_plan.hpp).  No pool of B = 7
# reaches that, and no pool of n = 50 or 130 at any B, so the form runs here on the n = 300 case with its seven families
# repeated CHAIN_TILES times: B = 112, 2 x 19 tiles per filter.
CHAIN_TILES = 16


@pytest.mark.parametrize("plan", list(PLANS))
def test_chained_pass_on_the_motion_families(hip, checker, plan):
    """set_step_chain / set_chain as tests/test_gpu_rank2_chain.py's _run sets them: the chained launches are the log's
    (chain_counts()), the single correction is k_rank2_queue; the first and the last repetition of the seven families against
    the checker at FP64_TOL, and bit for bit against the same pool with the chain off and against the call-fused form"""
    n, R = pm.SHAPES[2], CHAIN_TILES
    c = pm.make_case(n)
    B = pm.B * R
    log = [np.tile(c.twist, (1, R, 1)), np.tile(c.lm_idx, (1, R, 1)), np.tile(c.z_xy, (1, R, 1, 1)), np.tile(c.init_xy, (R, 1))]
    slots = [int((c.lm_idx[t] >= 0).any(axis=0).sum()) for t in range(pm.T)]
    expected = (sum(a >= 2 for a in slots), sum(a for a in slots if a >= 2))      # (vmax = 4 <= 8 slots: one launch per step)
    pick = list(range(pm.B)) + list(range(B - pm.B, B))
    res = {}
    for name, chain, call_fused in (("chain", True, False), ("off", False, False), ("fused", True, True)):
        bt = hip.BatchEKF(B, n)
        bt.set_row_packing(False)
        bt.set_call_fused(call_fused)
        bt.set_step_chain(chain)
        if chain and not call_fused:
            bt.set_chain(2, hip.CHAIN_POLICY_EXPLICIT | 5)
        bt.upload_known_log(*log)
        for t0, t1 in PLANS[plan]:
            bt.run_known(t0, t1)
        res[name] = {"state": [bt.state(b) for b in pick], "cov": [bt.cov(b) for b in pick], "chain": bt.chain_counts(),
                     "counts": bt.form_counts(), "kernel": bt.rank2_kernel()[0]}
        bt.close()
    on, off, cf = res["chain"], res["off"], res["fused"]
    assert "k_rank2_queue<" in on["kernel"], f"the pool does not take the tile queue ({on['kernel']})"
    assert expected[0] >= 10 and on["chain"] == expected, (on["chain"], expected)
    assert off["chain"] == (0, 0) and cf["chain"] == (0, 0)
    assert on["counts"]["rank2_streams"] == off["counts"]["rank2_streams"] == sum(slots)
    assert cf["counts"]["call_fused_passes"] > 0 and cf["counts"]["rank2_streams"] == 0
    ref = checker("known", n)
    for i, b in enumerate(pick):
        fam = pm.FAMILIES[b % pm.B]
        w = assert_parity(on["state"][i], on["cov"][i], ref[b % pm.B][0], ref[b % pm.B][1], FP64_TOL, f"chained {plan}, filter {b} ({fam}) vs checker")
        _note(("known", "chain (B = 112)", fam), w)
        for name, other in (("chain off", off), ("call-fused", cf)):
            assert np.array_equal(on["state"][i], other["state"][i]) and np.array_equal(on["cov"][i], other["cov"][i]), \
                f"chained vs {name} {plan}: filter {b} ({fam})"
    NOTES["known", n, "chain (B = 112)", plan] = f"{on['counts']} chain {on['chain']} {on['kernel']}"


def test_single_filter_pool_equals_the_single_filter_api_on_spin(hip):
    """B = 1 on the `spin` log against EKF_SLAM, call by call the same kernels: the same bits (as
    test_gpu_parity.py::test_batch_equals_single_filters_bitwise), at n = 50 and beyond the small path"""
    spin = pm.FAMILIES.index("spin")
    for n in pm.SHAPES[:2]:
        c = pm.make_case(n)
        bt = hip.BatchEKF(1, n)
        bt.upload_known_log(c.twist[:, spin:spin + 1], c.lm_idx[:, spin:spin + 1], c.z_xy[:, spin:spin + 1], c.init_xy[spin:spin + 1])
        bt.run_known(0, 5)
        bt.run_known(5, pm.T)
        f = hip.EKF_SLAM(n)
        for t in range(pm.T):
            f.prediction(c.twist[t, spin])
            f.measurement(*c.expand_step(t, spin))
        assert abs(f.state[0]) > 3 * np.pi
        assert np.array_equal(bt.state(0), f.state) and np.array_equal(bt.cov(0), f.cov), f"n={n}"
        f.close()
        bt.close()


# ---- unknown association -------------------------------------------------------------------------------------------------

def _step_fused(mode):
    def configure(hip, bt):
        bt.set_small_map_path(False)       # step fusion is the form beyond the LDS-resident path
        bt.set_step_fused(mode)
    return configure


def _delayed_unknown(speculate=True, sym=False):
    def configure(hip, bt):
        bt.set_small_map_path(False)
        bt.set_update_mode(32, symmetric_gather=sym)
        bt.set_forms(bt.forms | hip.FORM_STEP_SPECULATE if speculate else bt.forms & ~hip.FORM_STEP_SPECULATE)
    return configure


UNKNOWN_FORMS = {"default": lambda hip, bt: None, "fused_off": _step_fused(0), "fused_auto": _step_fused(1),
                 "fused_always": _step_fused(2), "delayed32_speculate": _delayed_unknown(True),
                 "delayed32_nospeculate": _delayed_unknown(False), "delayed32_sym": _delayed_unknown(True, sym=True)}
UNKNOWN_SAME_BITS = {"default": "fused_off", "fused_auto": "fused_off", "fused_always": "fused_off",
                     "delayed32_speculate": "delayed32_nospeculate"}
_unknown_runs = {}


def _unknown_run(hip, n, surveyed, form, fresh=False):
    key = (n, surveyed, form)
    if fresh or key not in _unknown_runs:
        c = pm.make_case(n)
        B = pm.B
        bt = hip.BatchEKF(B, n)
        configure = UNKNOWN_FORMS[form]
        if surveyed:   # a map built by a first known-association call at the start pose, then every reading scored against all n
            bt.upload_known_log(np.zeros((1, B, 2)), np.full((1, B, 1), -1, dtype=np.int32), np.zeros((1, B, 1, 2)), c.survey_xy)
            bt.run_known()
            bt.set_known_counts(n)
        configure(hip, bt)
        bt.upload_unknown_log(*c.unknown_log())
        st = bt.run_unknown(0, pm.T, time_kernels=True)
        cov = [bt.cov(b) for b in range(B)]
        _unknown_runs[key] = {"state": [bt.state(b) for b in range(B)], "digest": [_digest(x) for x in cov],
                              "decisions": bt.decisions().copy(), "known": bt.known_counts().copy(), "counts": bt.form_counts(),
                              "forms": bt.forms, "spec": bt.spec_counts(), "stats": st}
        bt.close()
        return _unknown_runs[key], cov
    return _unknown_runs[key], None


@pytest.mark.parametrize("form", list(UNKNOWN_FORMS))
@pytest.mark.parametrize("surveyed", [False, True])
@pytest.mark.parametrize("n", pm.SHAPES)
def test_unknown_forms_on_the_motion_families(hip, checker, n, surveyed, form):
    c = pm.make_case(n)
    r, cov = _unknown_run(hip, n, surveyed, form, fresh=True)
    ref = checker("surveyed" if surveyed else "empty", n)
    applied = 0
    for b, fam in enumerate(pm.FAMILIES):
        state, rcov, dec, kc = ref[b]
        J = c.count[:, b]
        for t in range(pm.T):
            assert np.array_equal(r["decisions"][t, b, :J[t]], dec[t, :J[t]]), f"n={n} {form}: decisions of filter {b} ({fam}) at step {t}"
        assert r["known"][b] == kc, f"n={n} {form}: known count of filter {b} ({fam})"
        w = assert_parity(r["state"][b], cov[b], state, rcov, FP64_TOL, f"n={n} surveyed={surveyed} {form}, filter {b} ({fam}) vs checker")
        _note(("surveyed" if surveyed else "empty", form, fam), w)
        applied += int((dec >= 0).sum())
    assert r["stats"]["corrections"] == applied > 100
    # the form ran
    fc, forms, launches = r["counts"], r["forms"], r["stats"]["rank2_launches"]
    flushes = fc["flush_plain"] + fc["flush_strip"] + fc["flush_mirrored"]
    steps, slots = int((c.count.max(axis=1) > 0).sum()), int(c.count.max(axis=1).sum())
    if form == "default":
        assert forms == hip.FORMS_DEFAULT
    elif form == "fused_off":
        assert not forms & (hip.FORM_STEP_FUSED | hip.FORM_SMALL_MAP) and launches == slots, (launches, slots)
    elif form == "fused_auto":
        assert forms & hip.FORM_STEP_FUSED and forms & hip.FORM_STEP_SPLIT_PASS and steps <= launches <= 2 * steps, (launches, steps)
        # the separate streaming pass is taken from a launch bound of N >= 603 with fresh known counts: the surveyed map of
        # n = 300 (on the empty map no prefix of these logs gets there)
        assert (fc["step_split_passes"] > 0) == (surveyed and 3 + 2 * n >= 603), fc
    elif form == "fused_always":
        assert forms & hip.FORM_STEP_FUSED and not forms & hip.FORM_STEP_SPLIT_PASS and launches == steps, (launches, steps)
    else:
        assert flushes >= 2, fc
        if form == "delayed32_sym":
            assert (fc["flush_mirrored"] == flushes) if 3 + 2 * n >= 256 else fc["flush_mirrored"] == 0, fc
        eligible, hits = r["spec"]
        if form == "delayed32_nospeculate":
            assert not forms & hip.FORM_STEP_SPECULATE and (eligible, hits) == (0, 0)
        else:
            assert forms & hip.FORM_STEP_SPECULATE and 0 < hits <= eligible, (eligible, hits)
    NOTES["unknown", n, surveyed, form] = f"{fc} spec {r['spec']} launches {launches} (steps {steps}, slots {slots})"
    if form in UNKNOWN_SAME_BITS:
        other, _ = _unknown_run(hip, n, surveyed, UNKNOWN_SAME_BITS[form])
        assert np.array_equal(r["decisions"], other["decisions"]) and np.array_equal(r["known"], other["known"])
        for b, fam in enumerate(pm.FAMILIES):
            assert np.array_equal(r["state"][b], other["state"][b]), f"n={n} {form} vs {UNKNOWN_SAME_BITS[form]}: state of filter {b} ({fam})"
            assert r["digest"][b] == other["digest"][b], f"n={n} {form} vs {UNKNOWN_SAME_BITS[form]}: Sigma of filter {b} ({fam})"


def test_zz_report():
    """worst per-block error against the checker per (log, form, family), what each form launched, and what the families
    reach (printed with -s)"""
    for n in pm.SHAPES:
        r = pm.reach(n)
        print(f"pool motion n={n}: wraps {r['wraps']} of corrections {r['corrections']}; final theta of spin "
              f"{r['final_theta']['spin']:+.3f}; steps with both branches {r['mixed_steps']}/{pm.T}")
    forms = sorted({(k, f) for k, f, _ in WORST})
    for kind, form in forms:
        print(f"pool motion worst {kind:9s} {form:28s} " + "  ".join(f"{fam} {WORST.get((kind, form, fam), 0.0):.2e}" for fam in pm.FAMILIES))
    for k in sorted(NOTES, key=str):
        print(f"pool motion ran {k}: {NOTES[k]}")
    assert all(v <= FP64_TOL for (k, f, _), v in WORST.items() if f != "current_columns_vs_rebuilt")
