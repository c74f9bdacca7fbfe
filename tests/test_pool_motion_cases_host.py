"""CPU: tests/pool_motion_cases.py proved before the GPU sees it (tests/test_gpu_pool_motion.py).

1. each motion family reaches what it names (branches on both sides of the gate in one step, headings beyond 3 pi, raw bearing
   differences beyond +-pi, silent runs of mixed branches), counted on the restated filter's own trajectory;
2. the checker is right on these logs: OracleEKF(STRUCTURED) against the reference's own class (RefEKF; skipped where
   oracle/_ref was not built) within FP64_TOL / 10 on every filter of every case, so the GPU comparison at FP64_TOL keeps a
   margin of ten; the restatement that takes the mutants (MotionEKF) is held against the checker the same way;
3. the cases can see the bugs they are for: every mutant moves the filter of each family meant for it by more than
   1000 x FP64_TOL in some block of state or covariance.
`-s` prints the figures (the report of profiles/r35/pool_motion.txt)."""
import numpy as np
import pytest

import pool_motion_cases as pm
import ref_scenarios as rs
from parity import FP64_TOL, worst

SEEN = 1000 * FP64_TOL     # a mutant counts as seen above this per-block error
REPORT = {}


@pytest.fixture(scope="module")
def ref(oracle):
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    return oracle.RefEKF


@pytest.mark.parametrize("n", pm.SHAPES)
def test_logs_are_what_the_pool_takes(n):
    """shapes and conventions of upload_known_log / upload_unknown_log; one world for the pool with its minimum spacing and
    clearance; ragged counts, steps with VMAX readings, a blind tail, filters that sit steps out beside filters that read"""
    c = pm.make_case(n)
    B, T = pm.B, pm.T
    assert c.twist.shape == (T, B, 2) and c.lm_idx.shape == (T, B, pm.VMAX) and c.lm_idx.dtype == np.int32
    assert c.z_xy.shape == (T, B, pm.VMAX, 2) and c.init_xy.shape == (B, 2 * n)
    assert c.count.shape == (T, B) and c.count.dtype == np.int32 and c.meas_xy.shape == (T, B, pm.JMAX, 2)
    assert (c.lm_idx[0] == -1).all()                          # the first call only initialises
    for t in range(T):
        for b in range(B):
            idx = c.lm_idx[t, b]
            k = int((idx >= 0).sum())
            assert (idx[k:] == -1).all() and np.all(np.diff(idx[:k]) > 0) and (idx[:k] < n).all()
            assert k == 0 or c.reads[t, b]
            assert 0 <= c.count[t, b] <= pm.JMAX and (c.count[t, b] == 0 or c.reads[t, b])
            J = int(c.count[t, b])
            tr = c.truth_idx[t, b, :J]
            assert len(set(tr.tolist())) == J                 # one reading per landmark
            d = np.hypot(*(c.world[tr] - c.pose[t, b, 1:]).T)
            assert (d <= pm.R_VISIBLE).all()
    d = np.hypot(c.world[:, None, 0] - c.world[None, :, 0], c.world[:, None, 1] - c.world[None, :, 1])
    assert d[~np.eye(n, dtype=bool)].min() >= pm.MIN_SPACING
    flat = c.pose.reshape(-1, 3)
    assert np.hypot(c.world[:, None, 0] - flat[None, :, 1], c.world[:, None, 1] - flat[None, :, 2]).min() >= pm.CLEARANCE
    counts = (c.lm_idx >= 0).sum(axis=2)
    assert (counts == pm.VMAX).any() and len(set(counts[1:].reshape(-1).tolist())) >= 3     # full steps, ragged slots
    spin = pm.FAMILIES.index("spin")
    assert (counts[-4:, spin] == 0).all() and (counts[-4:].sum(axis=1) > 0).all()           # a blind tail beside readers
    assert (counts[1:].sum(axis=1) > 0).all()                 # every step of the pool corrects somewhere
    assert counts[1:].sum() > 32 * 2 and int((counts[1:] > 0).any(axis=1).sum()) == T - 1
    slots = sum(int((c.lm_idx[t] >= 0).any(axis=0).sum()) for t in range(T))
    assert slots > 2 * 32                                    # more pool-wide slots than k = 32 holds: a flush in mid-run
    REPORT[f"case n={n}"] = (f"corrections per filter {counts.sum(axis=0).tolist()}, pool-wide slots {slots}, "
                             f"unknown readings per filter {c.count.sum(axis=0).tolist()}")


@pytest.mark.parametrize("n", pm.SHAPES)
def test_each_family_reaches_what_it_names(n):
    c = pm.make_case(n)
    r = pm.reach(n)
    # the twists themselves
    tw = {f: pm.family_twists(f)[0] for f in pm.FAMILIES}
    assert {pm.branch(a) for a in tw["gate"][:, 0]} == {"straight", "arc"} and (tw["gate"][:, 1] == 0.2).all()
    assert set(rs.straight_threshold()) <= set(tw["gate"][:, 0].tolist())
    assert (tw["straight"][:, 0] == 0).all() and np.signbit(tw["straight"][:, 0]).any() and not np.signbit(tw["straight"][:, 0]).all()
    assert (tw["straight"][:, 1] > 0).any() and (tw["straight"][:, 1] < 0).any()
    assert (tw["in_place"][:, 1] == 0).all() and {0.3, -0.3, 0.0} == set(tw["in_place"][:, 0].tolist())
    assert (tw["reverse"] < 0).all()
    assert {1.4, -1.4, 3.1, -3.1} == set(tw["spin"][:, 0].tolist())
    # both branches among the filters of one step (of every step, here)
    assert r["mixed_steps"] == pm.T
    # spin: the true heading leaves (-pi, pi] within three steps, the filter's own ends beyond 3 pi, and it was read from
    # beyond 3 pi in both directions
    spin = pm.FAMILIES.index("spin")
    assert abs(c.pose[2, spin, 0]) > rs.PI
    assert abs(r["final_theta"]["spin"]) > 3 * rs.PI
    f = pm.MotionEKF(n)
    seen = []
    for t in range(pm.T):
        f.prediction(*c.twist[t, spin])
        if c.reads[t, spin] and t > 0:
            seen.append(f.state[0])
        f.measurement(*c.expand_step(t, spin))
    assert max(seen) > 3 * rs.PI and min(seen) < -3 * rs.PI, seen
    # behind and spin: corrections whose raw bearing difference lies beyond +-pi
    assert r["wraps"]["behind"] > 0 and r["wraps"]["spin"] > 0, r["wraps"]
    # silent_mix: a run of >= 2 predictions of different branches in front of a correction
    sm = pm.FAMILIES.index("silent_mix")
    runs, cur = [], []
    for t in range(1, pm.T):
        cur.append(pm.branch(c.twist[t, sm, 0]))
        if (c.lm_idx[t, sm] >= 0).any():
            runs.append(cur)
            cur = []
    mixed = [x for x in runs if len(x) >= 3 and len(set(x[:-1])) == 2]     # (the last prediction is the reading step's own)
    assert len(mixed) >= 3 and {len(x) - 1 for x in mixed} >= {2, 3, 4}, runs
    # in_place: a10 = a20 = 0 exactly on the arc branch
    th = 0.7
    dth, dx = 0.3, 0.0
    assert -(dx / dth) * np.cos(th) + (dx / dth) * np.cos(th + dth) == 0.0 and -(dx / dth) * np.sin(th) + (dx / dth) * np.sin(th + dth) == 0.0
    REPORT[f"reach n={n}"] = (f"wraps (|raw bearing difference| > pi) {r['wraps']} of corrections {r['corrections']}; "
                              f"final theta spin {r['final_theta']['spin']:+.3f}; spin read at theta {[round(float(s), 2) for s in seen]}; "
                              f"steps with both branches {r['mixed_steps']}/{pm.T}")


def _worst(a, b):
    return worst(a.state, a.cov, b.state, b.cov)[0]


@pytest.mark.parametrize("n", pm.SHAPES)
def test_checker_against_the_reference_on_the_known_logs(oracle, ref, n):
    c = pm.make_case(n)
    for b, fam in enumerate(pm.FAMILIES):
        o = pm.replay_known(oracle.OracleEKF(n, oracle.STRUCTURED), c, b)
        r = pm.replay_known(ref(n), c, b)
        w = _worst(o, r)
        REPORT[f"checker vs reference, known n={n} {fam}"] = f"{w:.3e}"
        assert w <= FP64_TOL / 10, (fam, w)


@pytest.mark.parametrize("surveyed", [False, True])
@pytest.mark.parametrize("n", pm.SHAPES)
def test_checker_against_the_reference_on_the_unknown_logs(oracle, ref, n, surveyed):
    """... and no decision of the checker sits within 1e-6 (relative) of a gate or of its runner-up: a GPU result within
    FP64_TOL decides the same way.  (On a surveyed map the reference scores every reading against all n landmarks with
    dense products, minutes at n = 300: there the reference runs at n = 50 and 130; the surveyed map of n = 300 replays the
    same readings through the same code, and only its decision margins are taken -- reported as "not run".)"""
    c = pm.make_case(n)
    live = not surveyed or n <= pm.SHAPES[1]
    for b, fam in enumerate(pm.FAMILIES):
        o = oracle.OracleEKF(n, oracle.STRUCTURED)
        ko = pm.survey(o, c, b) if surveyed else np.zeros(n, dtype=np.uint8)
        mg = oracle.new_margins()
        dec = pm.replay_unknown(o, c, b, ko, mg)
        w = None
        if live:
            r = ref(n)
            kr = pm.survey(r, c, b) if surveyed else np.zeros(n, dtype=np.uint8)
            pm.replay_unknown(r, c, b, kr)
            assert np.array_equal(ko, kr), fam
            w = _worst(o, r)
            assert w <= FP64_TOL / 10, (fam, w)
        REPORT[f"checker vs reference, unknown n={n} surveyed={int(surveyed)} {fam}"] = \
            f"{'not run' if w is None else format(w, '.3e')}  corrections {int((dec >= 0).sum())}, dropped {int((dec == -1).sum())}, decision margin {mg[4]:.2e}"
        assert mg[4] > 1e-6, (fam, mg)
        assert (dec >= 0).sum() > 0


@pytest.mark.parametrize("n", pm.SHAPES)
def test_the_restatement_that_takes_the_mutants_is_the_checker(oracle, n):
    """MotionEKF without a mutant against OracleEKF(STRUCTURED): known log, and unknown log on the empty map with the
    decisions identical"""
    c = pm.make_case(n)
    for b, fam in enumerate(pm.FAMILIES):
        w = _worst(pm.replay_known(pm.MotionEKF(n), c, b), pm.replay_known(oracle.OracleEKF(n, oracle.STRUCTURED), c, b))
        assert w <= FP64_TOL / 10, (fam, w)
        if n == pm.SHAPES[0]:
            m, o = pm.MotionEKF(n), oracle.OracleEKF(n, oracle.STRUCTURED)
            dm = pm.replay_unknown(m, c, b, np.zeros(n, dtype=np.uint8))
            do = pm.replay_unknown(o, c, b, np.zeros(n, dtype=np.uint8))
            assert np.array_equal(dm, do), fam
            assert _worst(m, o) <= FP64_TOL / 10, fam


@pytest.mark.parametrize("n", pm.SHAPES)
@pytest.mark.parametrize("mutant", sorted(pm.MUTANTS))
def test_each_mutant_is_seen_by_the_family_meant_for_it(n, mutant):
    """gate `<=` for `<` | straight branch dropped | sign of a10 on the straight branch | the wrap of :187 dropped | an
    accumulated prediction map that forgets a silent step.  The cap: no family meant for a mutant may be blind to it -- each
    family is one filter of the pool, and that filter must move by more than 1000 x FP64_TOL in some block."""
    c = pm.make_case(n)
    moved = {}
    for b, fam in enumerate(pm.FAMILIES):
        good = pm.replay_known(pm.MotionEKF(n), c, b)
        bad = pm.replay_known(pm.MotionEKF(n, mutant), c, b)
        moved[fam] = _worst(bad, good)
    REPORT[f"mutant {mutant} n={n}"] = "  ".join(f"{f} {moved[f]:.1e}" for f in pm.FAMILIES)
    for fam in pm.MUTANTS[mutant]:
        assert moved[fam] > SEEN, (mutant, fam, moved)


def test_zz_report():
    for k, v in REPORT.items():
        print(f"pool motion host: {k}: {v}")
