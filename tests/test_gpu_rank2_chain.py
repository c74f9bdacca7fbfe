"""-m gpu: the chained pass of eager pools (k_rank2_chain, EKF_FORM_STEP_CHAIN) -- all corrections of a step in one launch,
tile batch by tile batch -- against the one-launch-per-correction stream and the call-fused form, through the C ABI.

The same operations on every element in the same order: every comparison between forms is bit for bit; one shape also runs
against OracleEKF(STRUCTURED) under tests/test_gpu_dense_sigma.py's entrywise metric and its 1e-9.  chain_counts() shows
which form ran.

The first eight tests run the benchmark's own log family (config5: "untouched stays untouched" -- such a log corrects at
most four landmarks per filter, all in the filter's first tile).  The tests behind them run tests/rank2_chain_cases.py's
survey logs, on which every step corrects every tile of every filter: the table's edge shapes (one column chunk, ld off the
2-KB boundary, a one-row last tile, three chunks with packing off, nine slots = two launches per step), every batch size,
all sixteen cache policies, uneven activity, run boundaries and a change of form between runs of one pool."""
import dataclasses

import numpy as np
import pytest

import dense_sigma_cases as cases
import rank2_chain_cases as chain_cases
from ekf_slam_ml_amd import synth
from parity import FP64_TOL

pytestmark = pytest.mark.gpu

# (n, B): the tile-queue test's two shapes, and N = 1005 -- the last column chunk partly valid, the last double2 half
# valid, 1005 = 62 * 16 + 13 rows: a last tile of fewer than 16 rows
SHAPES = [(1000, 24), (500, 80), (501, 70)]


FORMS = {"chain": (True, False), "off": (False, False), "fused": (True, True)}   # name -> (set_step_chain, set_call_fused)


def _run(hip, log, chain=True, call_fused=False, m=0, policy=0, cuts=None, configure=None, time_kernels=False, packing=True,
         plan=None, snap=()):
    """one pool over the whole log (in runs that end at `cuts`); returns a dict of what the tests compare.  plan: runs as
    [(t1, form name)] instead -- the form is switched on the same pool between runs; snap: filters whose state and Sigma
    are also taken after every run"""
    B, n = log.cfg.filters, log.cfg.n
    bt = hip.BatchEKF(B, n)
    if not packing:
        bt.set_row_packing(False)
    bt.set_call_fused(call_fused)
    bt.set_step_chain(chain)
    assert bool(bt.forms & hip.FORM_STEP_CHAIN) == chain
    if m or policy:
        bt.set_chain(m, policy)
    if configure:
        configure(bt)
    bt.upload_known_log(log.twist, log.lm_idx, log.z_xy, log.init_xy)
    T = log.twist.shape[0]
    stats, after, snaps, t0 = [], [], [], 0
    for t1, form in plan or [(t, None) for t in list(cuts or []) + [T]]:
        if form is not None:
            bt.set_step_chain(FORMS[form][0])
            bt.set_call_fused(FORMS[form][1])
        stats.append(bt.run_known(t0, t1, time_kernels=time_kernels))
        after.append(bt.chain_counts())
        snaps.append({b: (bt.state(b), bt.cov(b)) for b in snap})
        t0 = t1
    assert t0 == T
    pick = sorted({0, B // 2, B - 1})
    out = {"state": [bt.state(b) for b in pick], "cov": [bt.cov(b) for b in pick], "checksum": bt.checksum(),
           "chain": bt.chain_counts(), "forms": bt.form_counts(), "stats": stats, "kernel": bt.rank2_kernel()[0],
           "chain_after": after, "snaps": snaps}
    bt.close()
    return out


def _expected(log):
    """(chained launches, corrections they apply, correction passes of the whole log): a step chains when two or more of
    its slots hold a correction in some filter, in ceil(slots / 8) launches (rank2_chain_cases.expected_counts)"""
    return chain_cases.expected_counts(log)


def _same(a, b, what):
    for x, y in zip(a["state"] + a["cov"], b["state"] + b["cov"]):
        assert np.array_equal(x, y), f"{what}: {int((x != y).sum())} entries differ"
    assert np.allclose(a["checksum"], b["checksum"], rtol=1e-12)   # (the pool checksum is summed in no fixed order)


@pytest.fixture(scope="module")
def log_1000():
    return synth.make_known_log(synth.config5(filters=24, steps=5, n=1000))


@pytest.fixture(scope="module")
def off_1000(hip, log_1000):
    return _run(hip, log_1000, chain=False, time_kernels=True)


@pytest.mark.parametrize("n,B", SHAPES)
def test_chain_is_bit_identical(hip, n, B, log_1000, off_1000):
    """chain on, chain off and the call-fused form: the same bits in state and all of Sigma (first, middle, last filter),
    pool checksums to 1e-12; the chained form ran with the bit on (every step has V = 2 corrections) and not with it off"""
    log = log_1000 if (n, B) == (1000, 24) else synth.make_known_log(synth.config5(filters=B, steps=5, n=n))
    on = _run(hip, log, chain=True)
    off = off_1000 if (n, B) == (1000, 24) else _run(hip, log, chain=False)
    cf = _run(hip, log, chain=True, call_fused=True)
    assert "k_rank2_queue<" in on["kernel"], on["kernel"]   # (the single-correction plan of these pools: the tile queue)
    steps, corr, passes = _expected(log)
    assert steps >= 3 and on["chain"] == (steps, corr), on["chain"]
    assert off["chain"] == (0, 0) and cf["chain"] == (0, 0), (off["chain"], cf["chain"])
    assert on["forms"]["rank2_streams"] == off["forms"]["rank2_streams"] == passes
    assert cf["forms"]["call_fused_passes"] > 0 and cf["forms"]["rank2_streams"] == 0
    _same(on, off, f"n={n} B={B}: chain on vs off")
    _same(on, cf, f"n={n} B={B}: chain on vs call-fused")


def test_chain_against_the_structured_checker(hip, oracle):
    """tests/test_gpu_dense_sigma.py's test_pool_tile_queue case at n = 500 (a survey, then steps on a full Sigma) with the
    chain on: filters 0 and B - 1 against the checker, entry_err <= 1e-9, and bit for bit the chain-off run"""
    n, B = 500, 80
    log = cases.survey_log(n, cases.POOL_QUEUE_VMAX, B=B, seed=600 + n)
    filters = [0, B - 1]
    traces, _ = cases.checker_pool(oracle, log, filters)
    for b in filters:
        cases.require_preconditions([c for _, c in traces[b]], f"filter {b}")
    res = {}
    for chain in (True, False):
        bt = hip.BatchEKF(B, n)
        bt.set_call_fused(False)
        bt.set_step_chain(chain)
        bt.upload_known_log(log.twist, log.lm_idx, log.z_xy, log.init_xy)
        bt.run_known(0, log.steps)
        res[chain] = {b: (bt.state(b), bt.cov(b)) for b in filters}
        assert (bt.chain_counts()[0] > 0) == chain
        bt.close()
    worst = 0.0
    for b in filters:
        assert np.array_equal(res[True][b][0], res[False][b][0]) and np.array_equal(res[True][b][1], res[False][b][1])
        worst = max(worst, cases.assert_entrywise(*res[True][b], *traces[b][-1], FP64_TOL, f"chained, filter {b}", "k_rank2_chain"))
    print(f"measured chained pass n={n} B={B}: {worst:.3e}")


@pytest.mark.parametrize("m", [1, 2, 5, 8])
def test_chain_batch_sizes(hip, m, log_1000, off_1000):
    """m tiles per queue item through set_chain: a filter has 4 x 126 = 504 tiles, which neither 5 nor 8 divides, so every
    filter's last batch is short; an explicit cache policy on top (all plain for odd m, all non-temporal for even m)"""
    policy = hip.CHAIN_POLICY_EXPLICIT | (0 if m % 2 else 15)
    on = _run(hip, log_1000, chain=True, m=m, policy=policy)
    assert on["chain"][0] > 0
    _same(on, off_1000, f"m={m}")


def test_chain_uneven_activity(hip):
    """vmax = 3; within one step filters have 0, 1, 2 and 3 corrections (a known log is -1 padded, so a filter's corrections
    are its leading slots: "active only in the last slot" cannot be uploaded, a filter with fewer corrections than the step
    has slots is what skips the later sweeps), and one step has a single active slot pool-wide: that step does not chain"""
    B, n, T = 24, 1000, 5
    log = synth.make_known_log(dataclasses.replace(synth.config5(filters=B, steps=T, n=n), vmax=3))
    lm = log.lm_idx.copy()
    assert (lm[0] < 0).all() and (lm[1:] >= 0).all()   # (the first call only initialises the landmarks)
    keep = np.zeros((T, B), dtype=int)
    keep[1] = 3
    keep[2] = np.arange(B) % 4                   # 0, 1, 2, 3 corrections side by side
    keep[3] = (np.arange(B) % 3 == 0)            # one active slot pool-wide: no chain
    keep[4] = 3 - np.arange(B) % 4
    for t in range(T):
        for b in range(B):
            lm[t, b, keep[t, b]:] = -1
    masked = dataclasses.replace(log, lm_idx=lm)
    slots = [int((lm[t] >= 0).any(axis=0).sum()) for t in range(T)]
    assert slots == [0, 3, 3, 1, 3], slots
    steps, corr, passes = _expected(masked)
    on, off = _run(hip, masked, chain=True), _run(hip, masked, chain=False)
    assert on["chain"] == (steps, corr) and passes == corr + 1, on["chain"]   # step 3 takes the single launch
    assert on["forms"]["rank2_streams"] == off["forms"]["rank2_streams"] == passes
    _same(on, off, "uneven activity")


def test_chain_run_boundaries(hip, log_1000, off_1000):
    """run_known(0, 3) then run_known(3, 5) equals one run of five steps"""
    cut = _run(hip, log_1000, chain=True, cuts=[3])
    assert cut["chain"] == _expected(log_1000)[:2]
    _same(cut, off_1000, "run boundary")


def test_chain_reporters(hip, log_1000, off_1000):
    """run statistics keep their meaning (passes over Sigma and bytes per pass as in the chain-off run), and delayed,
    active-set, call-fused and small pools report no chained launch"""
    on = _run(hip, log_1000, chain=True, time_kernels=True)
    s_on, s_off = on["stats"][0], off_1000["stats"][0]
    assert s_on["rank2_launches"] == s_off["rank2_launches"] == _expected(log_1000)[2]
    assert s_on["rank2_bytes_per_launch"] == s_off["rank2_bytes_per_launch"]
    assert s_on["rank2_ms"] > 0 and s_on["corrections"] == s_off["corrections"]
    assert on["kernel"] == off_1000["kernel"]
    for name, configure in (("delayed", lambda bt: bt.set_update_mode(8)), ("active set", lambda bt: bt.set_active_set(True))):
        r = _run(hip, log_1000, chain=True, configure=configure)
        assert r["chain"] == (0, 0), (name, r["chain"])
    assert _run(hip, log_1000, chain=True, call_fused=True)["chain"] == (0, 0)
    small = synth.make_known_log(synth.config5(filters=2, steps=3, n=60))
    assert _run(hip, small, chain=True)["chain"] == (0, 0)


# ---- on a FULL covariance (tests/rank2_chain_cases.py; tests/test_rank2_chain_cases_host.py checks the inputs on the CPU) ----
# A config5 log corrects at most four landmarks per filter: all it can change lies in a filter's first tile.  Behind a
# survey every step corrects every tile of every filter, so a skipped tile, a dropped short batch, a wrong factor row in a
# ragged tile or in a later column chunk, or a second launch that does nothing changes the bits compared below.

@pytest.fixture(scope="module")
def off_full(hip):
    """name -> the chain-off run of that shape's log (one single run; computed once, shared, left unchanged)"""
    done = {}

    def get(name):
        if name not in done:
            s = chain_cases.BY_NAME[name]
            done[name] = _run(hip, s.log(), chain=False, packing=s.packing)
        return done[name]
    return get


def _takes_the_queue_and_chains(res, log, what):
    """loud, never a skip: the pool's single correction is the tile queue and the chained launches are the log's"""
    assert "k_rank2_queue<" in res["kernel"], f"{what}: the pool does not take the tile queue ({res['kernel']})"
    launches, corr, _ = chain_cases.expected_counts(log)
    assert launches > 0 and res["chain"] == (launches, corr), f"{what}: chain_counts {res['chain']}, the log implies {(launches, corr)}"


@pytest.mark.parametrize("name", [s.name for s in chain_cases.SHAPES])
def test_chain_shapes_on_a_full_sigma(hip, name, off_full):
    """every shape of the case table: chain on, chain off and call-fused give the same bits in state and all of Sigma
    (filters 0, B // 2, B - 1) after the survey and three steps that correct every tile; the queue kernel and the chained
    launch count are what the log implies"""
    s = chain_cases.BY_NAME[name]
    log = s.log()
    on = _run(hip, log, chain=True, packing=s.packing)
    off = off_full(name)
    cf = _run(hip, log, chain=True, call_fused=True, packing=s.packing)
    _takes_the_queue_and_chains(on, log, name)
    passes = chain_cases.expected_counts(log)[2]
    assert off["chain"] == (0, 0) and cf["chain"] == (0, 0), (off["chain"], cf["chain"])
    assert on["forms"]["rank2_streams"] == off["forms"]["rank2_streams"] == passes
    assert cf["forms"]["call_fused_passes"] > 0 and cf["forms"]["rank2_streams"] == 0
    assert on["kernel"] == off["kernel"]
    _same(on, off, f"{name}: chain on vs off")
    _same(on, cf, f"{name}: chain on vs call-fused")


@pytest.mark.parametrize("name", chain_cases.CHECKER_SHAPES)
def test_chain_on_a_full_sigma_against_the_checker(hip, oracle, name):
    """the chained run's filters 0 and B - 1 against OracleEKF(STRUCTURED) under the entrywise metric and FP64_TOL, after
    the survey and after every step under test (one run_known each)"""
    s = chain_cases.BY_NAME[name]
    log = s.log()
    S, filters = log.survey_steps, [0, s.B - 1]
    traces, _ = cases.checker_pool(oracle, log, filters)
    for b in filters:
        cases.require_preconditions([c for _, c in traces[b]], f"{name} filter {b}")
    on = _run(hip, log, chain=True, packing=s.packing, plan=[(t, "chain") for t in range(S, log.steps + 1)], snap=filters)
    _takes_the_queue_and_chains(on, log, name)
    assert len(on["snaps"]) == log.steps - S + 1 == len(traces[0])
    worst = 0.0
    for i, snap in enumerate(on["snaps"]):
        for b in filters:
            worst = max(worst, cases.assert_entrywise(*snap[b], *traces[b][i], FP64_TOL,
                                                      f"{name} chained, filter {b}, after step {S - 1 + i}", "k_rank2_chain"))
    print(f"measured chained pass {name} n={s.n} B={s.B}: {worst:.3e}")


@pytest.mark.parametrize("m", ["1", "2", "5", "8", "63", "tiles", "tiles+1"])
@pytest.mark.parametrize("name", chain_cases.BATCH_SHAPES)
def test_chain_batch_sizes_on_a_full_sigma(hip, name, m, off_full):
    """m tiles per queue item where every tile is corrected: short last batches (m = 5, 63), one item per filter
    (m = tiles) and the clamp (m = tiles + 1), on the one-row last tile and on the one-chunk shape"""
    s = chain_cases.BY_NAME[name]
    mm = dict(zip(("1", "2", "5", "8", "63", "tiles", "tiles+1"), chain_cases.batch_sizes(s)))[m]
    on = _run(hip, s.log(), chain=True, m=mm, packing=s.packing)
    _takes_the_queue_and_chains(on, s.log(), f"{name} m={mm}")
    _same(on, off_full(name), f"{name} m={mm}")


@pytest.mark.parametrize("p", range(16))
def test_chain_all_sixteen_policies(hip, p, off_full):
    """every instantiation k_rank2_chain<16, POL>: the four access sets plain or non-temporal in every mix (non-temporal
    stores followed by plain re-loads of the same lines among them), at m = 2 on the one-chunk shape"""
    s = chain_cases.BY_NAME["one-chunk"]
    on = _run(hip, s.log(), chain=True, m=2, policy=hip.CHAIN_POLICY_EXPLICIT | p, packing=s.packing)
    _takes_the_queue_and_chains(on, s.log(), f"policy {p}")
    _same(on, off_full("one-chunk"), f"policy {p}")


@pytest.mark.parametrize("which", ["uneven", "long-uneven"])
def test_chain_uneven_activity_on_a_full_sigma(hip, which):
    """test_chain_uneven_activity's masks behind a survey (0 .. 3 corrections side by side, one step with a single active
    slot pool-wide that must not chain), and the long call with 0, 1, 5, 8 and 9 corrections side by side: in its C = 1
    launch some filters have cnt = 1 and the others cnt = 0"""
    log, keep = chain_cases.uneven_log() if which == "uneven" else chain_cases.long_uneven_log()
    S = log.survey_steps
    on, off = _run(hip, log, chain=True), _run(hip, log, chain=False)
    _takes_the_queue_and_chains(on, log, which)
    launches, corr, passes = chain_cases.expected_counts(log)
    tail = chain_cases.expected_counts(log, S)
    if which == "uneven":
        assert [chain_cases.active_slots(log, t) for t in range(S, log.steps)] == [3, 3, 1, 3]
        assert tail == (3, 9, 10) and passes == corr + 1      # the one-slot step takes the single launch
    else:
        assert tail == (2 * keep.shape[0], 9 * keep.shape[0], 9 * keep.shape[0]) and passes == corr
    assert on["forms"]["rank2_streams"] == off["forms"]["rank2_streams"] == passes
    _same(on, off, which)


def test_chain_long_call(hip, off_full):
    """nine active slots: every step under test is a launch of C = 8 and one of C = 1 (first and last sweep at once);
    passes over Sigma and bytes per pass are reported as in the chain-off run"""
    s = chain_cases.BY_NAME["long-call"]
    log = s.log()
    S, steps = log.survey_steps, log.steps - log.survey_steps
    assert all(chain_cases.active_slots(log, t) == 9 for t in range(S, log.steps))
    on = _run(hip, log, chain=True, cuts=[S])
    off = _run(hip, log, chain=False, cuts=[S])
    _takes_the_queue_and_chains(on, log, "long call")
    before, after = on["chain_after"]
    assert (after[0] - before[0], after[1] - before[1]) == (2 * steps, 9 * steps), (before, after)
    assert before == chain_cases.expected_counts(log, 0, S)[:2]
    for run in (0, 1):
        assert on["stats"][run]["rank2_launches"] == off["stats"][run]["rank2_launches"] == chain_cases.expected_counts(log, *((0, S), (S, None))[run])[2]
        assert on["stats"][run]["rank2_bytes_per_launch"] == off["stats"][run]["rank2_bytes_per_launch"]
        assert on["stats"][run]["corrections"] == off["stats"][run]["corrections"]
    _same(on, off, "long call")
    _same(on, off_full("long-call"), "long call against the single chain-off run")


def test_chain_form_switching_on_one_pool(hip):
    """one pool: the survey chained, then one run_known per step under test -- chained, per-correction, call-fused, chained
    again (the forms share the factor buffers and the state swap) -- equals a pool that never chained, bit for bit;
    chain_counts moves in the chained steps only"""
    log = chain_cases.switch_log()
    S = log.survey_steps
    assert log.steps == S + 4
    sw = _run(hip, log, plan=[(S, "chain"), (S + 1, "chain"), (S + 2, "off"), (S + 3, "fused"), (S + 4, "chain")])
    off = _run(hip, log, chain=False)
    assert "k_rank2_queue<" in sw["kernel"], sw["kernel"]
    a = sw["chain_after"]
    assert a[0] == chain_cases.expected_counts(log, 0, S)[:2] and a[0][0] > 0
    assert a[1] == (a[0][0] + 1, a[0][1] + 2) and a[2] == a[1] and a[3] == a[1] and a[4] == (a[1][0] + 1, a[1][1] + 2), a
    assert sw["forms"]["call_fused_passes"] == 1 and off["chain"] == (0, 0)
    assert sw["forms"]["rank2_streams"] == off["forms"]["rank2_streams"] - 2
    _same(sw, off, "chained / per-correction / call-fused / chained on one pool")


def test_chain_run_boundary_on_a_full_sigma(hip, off_full):
    """a run boundary inside the steps under test (after the survey and one step) equals one run"""
    s = chain_cases.BY_NAME["one-row"]
    log = s.log()
    cut = _run(hip, log, chain=True, cuts=[log.survey_steps + 1])
    _takes_the_queue_and_chains(cut, log, "run boundary")
    _same(cut, off_full("one-row"), "run boundary on a full Sigma")
