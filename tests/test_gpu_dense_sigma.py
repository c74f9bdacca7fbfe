"""-m gpu: the kernels that read and write all N^2 entries of Sigma -- k_rank2 in its shapes, k_rank2_queue, k_rank2_packed,
k_rank2_active, the call-fused k_rank2v, the delayed k_flush / k_flush_strip / k_flush_sym, the column-panel and
current-columns forms, the separate streaming pass behind k_pool_step_unknown, k_maha -- on a FULL covariance matrix.

Every case replays a survey (tests/dense_sigma_cases.py: every landmark shown once, after which Sigma has no zero entry)
and then steps under test whose first one corrects landmark n - 1 and landmark 0, against OracleEKF(STRUCTURED):
state and all of Sigma under entry_err <= 1e-9 (every entry against sqrt(S_ii S_jj)), the per-block parity of the
neighbouring existing test as well, the bit-identity relations between forms that the existing tests state, and the
library's own reporters for the kernel / form the case is named for.  tests/test_dense_sigma_host.py shows on the CPU
that a single dropped 64 x 64 tile is three orders beyond this tolerance."""
import numpy as np
import pytest

import dense_sigma_cases as cases
from parity import FP64_TOL, assert_parity

pytestmark = pytest.mark.gpu


def _replay(f, log, t0, t1, b=0):
    for t in range(t0, t1):
        sensor, vis = log.expand_step(t, b)
        f.prediction(log.twist[t, b])
        f.measurement(sensor, vis)


def _same_bits(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: state differs"
    if not np.array_equal(a[1], b[1]):
        r, c = np.argwhere(a[1] != b[1])[0]
        raise AssertionError(f"{what}: covariance differs, first at ({r}, {c}) [64 x 64 tile ({r // 64}, {c // 64})], "
                             f"{int((a[1] != b[1]).sum())} entries in all")


def _single_vs_checker(hip, oracle, log, configure, kernel, parity_tol, name, delayed_k=0, compare_at=None):
    """one single filter through survey + steps under test; compared after the survey and after every step under test
    (compare_at: only behind these steps); returns (worst entry_err, final (state, cov))"""
    n, S = log.cfg.n, log.survey_steps
    tr = cases.checker_trace(oracle, log, 0)
    cases.require_preconditions([c for _, c in tr], name)
    f = hip.EKF_SLAM(n)
    configure(f)
    _replay(f, log, 0, S)
    worst = cases.assert_entrywise(f.state, f.cov, *tr[0], FP64_TOL, f"{name}: after the survey", kernel)
    assert_parity(f.state, f.cov, *tr[0], parity_tol, f"{name}: after the survey")
    if delayed_k:
        f.set_update_mode(delayed_k)
    for t in range(S, log.steps):
        _replay(f, log, t, t + 1)
        if compare_at is not None and t + 1 not in compare_at:
            continue
        s, c = f.state, f.cov
        worst = max(worst, cases.assert_entrywise(s, c, *tr[t + 1 - S], FP64_TOL, f"{name}: step under test {t - S}", kernel))
        assert_parity(s, c, *tr[t + 1 - S], parity_tol, f"{name}: step under test {t - S}")
    out = (f.state, f.cov)
    f.close()
    return worst, out


@pytest.mark.parametrize("n", cases.SINGLE_EAGER_N)
def test_single_filter_eager(hip, oracle, n):
    """EKF_SLAM beyond the LDS-resident path (forced off for n = 2, 31, which it would otherwise take): k_rank2 per landmark
    (set_call_fused(False)), k_rank2v per call (default), k_rank2_active, full-width association prefix -- bit-identical
    to each other, 1e-9 entrywise and 1e-11 per block (test_all_rank2_tile_shapes' tolerance) against the checker.
    EKF_SLAM has neither rank2_kernel() nor form_counts(): the k_rank2 instantiation is asked of a BatchEKF(1, n) (the same
    selection, ekf_kernels.hip rank2_variant) and the runs assert their form bits; that k_rank2_active ran is shown through
    touched() for pools only (test_pool_active_set)."""
    log = cases.survey_log(n, cases.SINGLE_VMAX, seed=100 + n)
    u, tpb = cases.SINGLE_EAGER_KERNEL[n]
    probe = hip.BatchEKF(1, n)
    probe.set_call_fused(False)
    kname, _ = probe.rank2_kernel()
    probe.close()
    assert kname == f"ekf::k_rank2<{u},false,{tpb}>", kname

    def variant(call_fused, active_set=False, prefix=True, tuning=None):
        def configure(f):
            f.set_small_map_path(False)
            f.set_call_fused(call_fused)
            f.set_active_set(active_set)
            f.set_active_prefix(prefix)
            if tuning:
                f.set_tuning(*tuning)
            assert bool(f.forms & hip.FORM_CALL_FUSED) == call_fused and not f.forms & hip.FORM_SMALL_MAP
            assert bool(f.forms & hip.FORM_ACTIVE_PREFIX) == prefix
        return configure

    runs = {"per landmark": (variant(False), kname), "call-fused": (variant(True), "k_rank2v"),
            "active set": (variant(False, active_set=True), "k_rank2_active"), "prefix off": (variant(True, prefix=False), "k_rank2v")}
    if n == cases.SINGLE_TUNING_N:
        for rows, nt in cases.SINGLE_TUNING:
            runs[f"tuning ({rows}, {nt})"] = (variant(False, tuning=(rows, nt)), f"k_rank2 rows_per_block={rows} nontemporal={nt}")
    outs, worst = {}, 0.0
    for name, (configure, kernel) in runs.items():
        w, outs[name] = _single_vs_checker(hip, oracle, log, configure, kernel, 1e-11, f"n={n} {name}")
        worst = max(worst, w)
    for name in outs:
        _same_bits(outs[name], outs["per landmark"], f"n={n}: {name} vs per landmark")
    print(f"measured single eager n={n}: {worst:.3e}")


@pytest.mark.parametrize("n", cases.SMALL_MAP_N)
def test_single_filter_small_map_path(hip, oracle, n):
    """measurement() as one LDS-resident launch (N <= 104) and as the gain + streaming pair, on a full Sigma: bit-identical
    (test_small_map_path_is_bit_identical) and against the checker"""
    log = cases.survey_log(n, cases.SINGLE_VMAX, seed=200 + n)
    outs, worst = [], 0.0
    for enable in (True, False):
        def configure(f):
            f.set_small_map_path(enable)
            assert bool(f.forms & hip.FORM_SMALL_MAP) == enable
        w, o = _single_vs_checker(hip, oracle, log, configure, "k_small_measure" if enable else "k_rank2v", FP64_TOL, f"small map n={n} {'on' if enable else 'off'}")
        outs.append(o)
        worst = max(worst, w)
    _same_bits(outs[0], outs[1], f"small map n={n}: on vs off")
    print(f"measured small map n={n}: {worst:.3e}")


@pytest.mark.parametrize("k", cases.DELAYED_SINGLE_K)
def test_single_filter_delayed(hip, oracle, k):
    """set_update_mode(k) on a surveyed filter: the survey runs eagerly, 18 steps x 8 corrections run delayed (two flushes and
    more at every k); test_single_filter_delayed_vs_oracle's tolerance.  Departure from "compare after each step under
    test": reading state or Sigma forces a flush, so a comparison per step would turn every k into "flush every step";
    the filter is compared behind the survey, behind step 10 (a read in the middle of a pending window, as the existing
    test does) and at the end, while the checker's preconditions are still checked for every step.  EKF_SLAM has no
    form_counts(): that a flush ran is shown for pools only (test_pool_delayed_plain_and_strip_flush)"""
    n = cases.DELAYED_SINGLE_N
    log = cases.survey_log(n, cases.SINGLE_VMAX, seed=300, extra_steps=cases.DELAYED_SINGLE_STEPS)
    S = log.survey_steps
    assert (log.steps - S) * cases.SINGLE_VMAX >= 2 * k + 8
    w, _ = _single_vs_checker(hip, oracle, log, lambda f: None, "k_flush", FP64_TOL, f"single delayed k={k}", delayed_k=k,
                              compare_at=(S + 10, log.steps))
    print(f"measured single delayed k={k}: {w:.3e}")


# ---- pools ----------------------------------------------------------------------------------------------------------------

def _pool(hip, log, configure=None):
    bt = hip.BatchEKF(log.cfg.filters, log.cfg.n)
    if configure:
        configure(bt)
    bt.upload_known_log(log.twist, log.lm_idx, log.z_xy, log.init_xy)
    return bt


def _pool_vs_checker(bt, traces, idx, filters, name, kernel, parity_tol=FP64_TOL):
    worst = 0.0
    for b in filters:
        s, c = bt.state(b), bt.cov(b)
        worst = max(worst, cases.assert_entrywise(s, c, *traces[b][idx], FP64_TOL, f"{name}, filter {b}", kernel))
        assert_parity(s, c, *traces[b][idx], parity_tol, f"{name}, filter {b}")
    return worst


def _eager_pool_run(hip, log, configure, traces, filters, name, kernel):
    """survey, compare, every step under test, compare; returns (worst, {b: final (state, cov)}, checksum, form counts, touched())"""
    S = log.survey_steps
    bt = _pool(hip, log, configure)
    bt.run_known(0, S)
    worst = _pool_vs_checker(bt, traces, 0, filters, f"{name}: after the survey", kernel)
    for t in range(S, log.steps):
        bt.run_known(t, t + 1)
        worst = max(worst, _pool_vs_checker(bt, traces, t + 1 - S, filters, f"{name}: step under test {t - S}", kernel))
    out = {b: (bt.state(b), bt.cov(b)) for b in filters}
    cs, fc, touched = bt.checksum(), bt.form_counts(), bt.touched()
    bt.close()
    return worst, out, cs, fc, touched


def _traces(oracle, log, filters, want_sums=False, fast=False):
    traces, sums = cases.checker_pool(oracle, log, filters, fast=fast, want_sums=want_sums)
    for b in filters:
        cases.require_preconditions([c for _, c in traces[b]], f"filter {b}")
    return traces, sums


@pytest.mark.parametrize("B,n,vmax", cases.POOL_CALLFUSED)
def test_pool_eager_and_call_fused(hip, oracle, B, n, vmax):
    """test_call_fused_pool_bitwise_and_vs_checker's shapes on a full Sigma: k_rank2v (one pass per call) and the
    per-landmark k_rank2 stream, bit-identical, every filter against the checker (n = 1000: filters 0, B // 2, B - 1 and
    the pool checksum against the sum of all filters' checker results)"""
    log = cases.survey_log(n, vmax, B=B, seed=400 + n)
    every = B * (3 + 2 * n) ** 2 <= 8e6
    filters = list(range(B)) if every else [0, B // 2, B - 1]
    traces, sums = _traces(oracle, log, filters, want_sums=not every)
    res = {}
    for cf in (True, False):
        def configure(bt):
            bt.set_call_fused(cf)
            if n in (401, 640):
                bt.set_tuning(rows_per_block=64 if n == 401 else 32)   # the big-pool form of the pass: K values staged in LDS
        res[cf] = _eager_pool_run(hip, log, configure, traces, filters, f"pool B={B} n={n} call_fused={cf}",
                                  "k_rank2v" if cf else "k_rank2")
        fc = res[cf][3]
        assert (fc["call_fused_passes"] > 0, fc["rank2_streams"] > 0) == (cf, not cf), fc
    for b in filters:
        _same_bits(res[True][1][b], res[False][1][b], f"pool B={B} n={n} filter {b}: call-fused vs per landmark")
    if sums is not None:
        for cf in (True, False):
            assert np.abs(res[cf][2] - sums).max() / np.abs(sums).max() < 1e-9, (res[cf][2], sums)
    print(f"measured pool call-fused B={B} n={n}: {max(res[True][0], res[False][0]):.3e}")


def _assert_packing(bt, packed, P=None, plain="ekf::k_rank2<"):
    """the plan the launcher launches from (BatchEKF.rank2_packing / rank2_kernel): the packed kernel with P > 1 rows per
    virtual row, or P = 1 and the plain kernel"""
    got, kname = bt.rank2_packing(), bt.rank2_kernel()[0]
    if packed:
        assert got > 1 and "k_rank2_packed" in kname and "k_rank2_queue" not in kname, (got, kname)
        assert P is None or got == P, (got, P)
    else:
        assert got == 1 and kname.startswith(plain), (got, kname)


@pytest.mark.parametrize("n,B", cases.POOL_PACKED)
def test_pool_row_packed(hip, oracle, n, B):
    """k_rank2_packed (test_row_packed_rank2_is_bit_identical's shapes) against the plain kernel bit for bit and against the
    checker: filters 0, B // 2, B - 1 entrywise, the pool checksum against the sum over all filters' checker results"""
    log = cases.survey_log(n, cases.POOL_PACKED_VMAX, B=B, seed=500 + n)
    filters = [0, B // 2, B - 1]
    traces, sums = _traces(oracle, log, filters, want_sums=True)
    res = {}
    for packed in (True, False):
        def configure(bt):
            bt.set_call_fused(False)   # the per-landmark rank-2 stream is what packs rows
            bt.set_row_packing(packed)
            assert bool(bt.forms & hip.FORM_ROW_PACKING) == packed and not bt.forms & hip.FORM_CALL_FUSED
            _assert_packing(bt, packed)
        res[packed] = _eager_pool_run(hip, log, configure, traces, filters, f"row packing {packed} n={n} B={B}",
                                      "k_rank2_packed" if packed else "k_rank2")
        assert res[packed][3]["rank2_streams"] > 0 and res[packed][3]["call_fused_passes"] == 0
        assert np.abs(res[packed][2] - sums).max() / np.abs(sums).max() < 1e-9, (res[packed][2], sums)
    for b in filters:
        _same_bits(res[True][1][b], res[False][1][b], f"n={n} B={B} filter {b}: packed vs plain")
    assert np.allclose(res[True][2], res[False][2], rtol=1e-12)
    print(f"measured pool row-packed n={n} B={B}: {max(res[True][0], res[False][0]):.3e}")


def _packed_run(hip, log, traces, filters, name, packed, P=None, tuning=None, plain="ekf::k_rank2<", want_name=None):
    def configure(bt):
        bt.set_call_fused(False)   # the per-landmark rank-2 stream is what packs rows
        bt.set_row_packing(packed)
        if tuning:
            bt.set_tuning(*tuning)
        _assert_packing(bt, packed, P, plain)
        if want_name:
            assert bt.rank2_kernel() == want_name, (bt.rank2_kernel(), want_name)
    res = _eager_pool_run(hip, log, configure, traces, filters, name, "k_rank2_packed" if packed else "k_rank2")
    assert res[3]["rank2_streams"] > 0 and res[3]["call_fused_passes"] == 0
    return res


@pytest.mark.parametrize("n,B,P", cases.POOL_PACKED_PLAN)
def test_pool_row_packed_at_the_work_floor(hip, oracle, n, B, P):
    """k_rank2_packed on the smallest pools that take it (cases.POOL_PACKED_PLAN says what each shape is there for), with the
    P the plan reports asserted: against the plain kernel bit for bit, filters 0, B // 2, B - 1 against the checker, the pool
    checksum against the sum over all filters' checker results"""
    log = cases.packed_plan_log(n, B)
    filters = [0, B // 2, B - 1]
    traces, sums = _traces(oracle, log, filters, want_sums=True)
    res = {packed: _packed_run(hip, log, traces, filters, f"row packing {packed} n={n} B={B} P={P}", packed, P) for packed in (True, False)}
    for packed in (True, False):
        assert np.abs(res[packed][2] - sums).max() / np.abs(sums).max() < 1e-9, (res[packed][2], sums)
    for b in filters:
        _same_bits(res[True][1][b], res[False][1][b], f"n={n} B={B} P={P} filter {b}: packed vs plain")
    assert np.allclose(res[True][2], res[False][2], rtol=1e-12)
    print(f"measured pool row-packed at the work floor n={n} B={B} P={P}: {max(res[True][0], res[False][0]):.3e}")


def test_pool_row_packed_instantiations(hip, oracle):
    """k_rank2_packed<8|16, false|true> on one shape, each named by the plan hook, with 40 virtual rows per workgroup (a short
    last block; several row groups per block): all bit-identical to the plain kernel and against the checker"""
    n = cases.POOL_PACKED_TUNING_N
    _, B, P = next(c for c in cases.POOL_PACKED_PLAN if c[0] == n)
    log = cases.packed_plan_log(n, B)
    filters = [0, B // 2, B - 1]
    traces, _ = _traces(oracle, log, filters)
    plain = _packed_run(hip, log, traces, filters, f"plain n={n} B={B}", False)
    worst = plain[0]
    for rows, nt, group in cases.POOL_PACKED_TUNING:
        want = (f"ekf::k_rank2_packed<{group},{'true' if nt else 'false'}>", rows)
        res = _packed_run(hip, log, traces, filters, f"{want[0]} rows_per_block={rows} n={n} B={B}", True, P,
                          tuning=(rows, nt, group), want_name=want)
        for b in filters:
            _same_bits(res[1][b], plain[1][b], f"n={n} B={B} filter {b}: {want[0]} vs plain")
        worst = max(worst, res[0])
    print(f"measured pool row-packed instantiations n={n} B={B}: {worst:.3e}")


def test_pool_under_the_work_floor_stays_plain(hip, oracle):
    """one filter fewer than the smallest pool that packs: P = 1 and the plain kernel with packing allowed, and still the
    checker's result"""
    n, B = cases.POOL_PACKED_BELOW
    log = cases.packed_plan_log(n, B)
    filters = [0, B // 2, B - 1]
    traces, sums = _traces(oracle, log, filters, want_sums=True)

    def configure(bt):
        bt.set_call_fused(False)
        assert bt.forms & hip.FORM_ROW_PACKING
        _assert_packing(bt, False)
    res = _eager_pool_run(hip, log, configure, traces, filters, f"under the work floor n={n} B={B}", "k_rank2")
    assert res[3]["rank2_streams"] > 0
    assert np.abs(res[2] - sums).max() / np.abs(sums).max() < 1e-9, (res[2], sums)
    print(f"measured pool under the work floor n={n} B={B}: {res[0]:.3e}")


def test_pool_row_packed_where_the_tile_queue_would_run(hip, oracle):
    """a pool big enough for the tile queue whose rows do not fill their strips: with packing on the launch is packed and the
    hooks say so (ekf_batch_rank2_resident used to say queue), with packing off it is k_rank2_queue; bit-identical, filters
    0, B // 2, B - 1 against the checker"""
    n, B, P = cases.POOL_PACKED_QUEUE
    log = cases.packed_plan_log(n, B)
    filters = [0, B // 2, B - 1]
    traces, _ = _traces(oracle, log, filters)
    res = {packed: _packed_run(hip, log, traces, filters, f"row packing {packed} n={n} B={B}", packed, P, plain="ekf::k_rank2_queue<")
           for packed in (True, False)}
    for b in filters:
        _same_bits(res[True][1][b], res[False][1][b], f"n={n} B={B} filter {b}: packed vs queue")
    assert np.allclose(res[True][2], res[False][2], rtol=1e-12)
    print(f"measured pool row-packed against the tile queue n={n} B={B}: {max(res[True][0], res[False][0]):.3e}")


@pytest.mark.parametrize("n,B", cases.POOL_QUEUE)
def test_pool_tile_queue(hip, oracle, n, B):
    """k_rank2_queue (test_rank2_tile_queue_is_bit_identical's shapes) against the grid form bit for bit and against the
    checker (n = 500: three filters + the checksum over all 80; n = 1000: filters 0 and B - 1)"""
    log = cases.survey_log(n, cases.POOL_QUEUE_VMAX, B=B, seed=600 + n)
    filters = [0, B // 2, B - 1] if n == 500 else [0, B - 1]
    traces, sums = _traces(oracle, log, filters, want_sums=n == 500)
    res = {}
    for queue in (True, False):
        def configure(bt):
            bt.set_call_fused(False)   # the per-landmark rank-2 stream
            bt.set_forms((bt.forms | hip.FORM_TILE_QUEUE) if queue else (bt.forms & ~hip.FORM_TILE_QUEUE))
            name, _ = bt.rank2_kernel()
            assert ("k_rank2_queue<" in name) == queue, name
        res[queue] = _eager_pool_run(hip, log, configure, traces, filters, f"tile queue {queue} n={n} B={B}",
                                     "k_rank2_queue" if queue else "k_rank2")
        if sums is not None:
            assert np.abs(res[queue][2] - sums).max() / np.abs(sums).max() < 1e-9, (res[queue][2], sums)
    for b in filters:
        _same_bits(res[True][1][b], res[False][1][b], f"n={n} B={B} filter {b}: queue vs grid")
    assert np.allclose(res[True][2], res[False][2], rtol=1e-12)   # (the pool checksum is summed in no fixed order)
    print(f"measured pool tile queue n={n} B={B}: {max(res[True][0], res[False][0]):.3e}")


def test_pool_active_set(hip, oracle):
    """k_rank2_active with every landmark touched (touched() == n behind the survey): all rows streamed, bit-identical to
    the dense stream (tests/test_gpu_active_set.py) and against the checker"""
    B, n, vmax = cases.POOL_ACTIVE
    log = cases.survey_log(n, vmax, B=B, seed=650)
    filters = list(range(B))
    traces, _ = _traces(oracle, log, filters)
    res = {}
    for on in (True, False):
        def configure(bt):
            bt.set_call_fused(False)   # the per-landmark stream is what the touched set narrows
            bt.set_active_set(on)
        res[on] = _eager_pool_run(hip, log, configure, traces, filters, f"active set {on}", "k_rank2_active" if on else "k_rank2")
    assert (res[True][4] == n).all(), res[True][4]          # touched() of the run with the active set on: every row is streamed
    assert res[True][3]["rank2_streams"] > 0 and res[True][3]["call_fused_passes"] == 0, res[True][3]
    for b in filters:
        _same_bits(res[True][1][b], res[False][1][b], f"active set filter {b}")
    print(f"measured pool active set: {max(res[True][0], res[False][0]):.3e}")


def _delayed_pool_run(hip, log, k, configure, cuts, symmetric=False):
    """the survey eagerly, then set_update_mode(k) and the steps under test in runs that end at `cuts`; returns the pool"""
    S = log.survey_steps
    bt = _pool(hip, log, configure)
    bt.run_known(0, S)
    bt.set_update_mode(k, symmetric_gather=symmetric)
    launches, t0 = 0, S
    for t1 in cuts:
        launches += bt.run_known(t0, t1, time_kernels=True)["rank2_launches"]
        t0 = t1
    return bt, launches


@pytest.mark.parametrize("B,n,k,vmax", cases.POOL_FLUSH)
def test_pool_delayed_plain_and_strip_flush(hip, oracle, B, n, k, vmax):
    """k_flush and k_flush_strip (forced: set_strip_flush("always")) on a full Sigma: bit-identical
    (test_strip_form_flush_is_bit_identical_to_the_plain_flush), a run boundary inside the steps under test, every filter
    against the checker at the boundary and at the end"""
    log = cases.survey_log(n, vmax, B=B, seed=700 + n, extra_steps=cases.flush_steps(k, vmax))
    S, T = log.survey_steps, log.steps
    mid = S + (T - S) // 2
    filters = list(range(B))
    traces, _ = _traces(oracle, log, filters)
    res, worst = [], 0.0
    for strip, rows in (("always", 0), ("never", 0), ("never", 16)):
        def configure(bt):
            bt.set_strip_flush(strip)
            bt.set_tuning(rows_per_block=rows)
        kernel = "k_flush_strip" if strip == "always" else "k_flush"
        bt, launches = _delayed_pool_run(hip, log, k, configure, (mid,))
        worst = max(worst, _pool_vs_checker(bt, traces, mid - S, filters, f"{kernel} B={B} n={n} k={k}: at the run boundary", kernel))
        launches += bt.run_known(mid, T, time_kernels=True)["rank2_launches"]
        worst = max(worst, _pool_vs_checker(bt, traces, T - S, filters, f"{kernel} B={B} n={n} k={k}: at the end", kernel))
        fc = bt.form_counts()
        assert launches >= 2
        assert (fc["flush_strip"], fc["flush_plain"]) == ((launches, 0) if strip == "always" else (0, launches)), fc
        res.append({b: (bt.state(b), bt.cov(b)) for b in filters})
        bt.close()
    for other in (1, 2):
        for b in filters:
            _same_bits(res[0][b], res[other][b], f"B={B} n={n} k={k} filter {b}: strip vs plain ({other})")
    print(f"measured pool delayed flush B={B} n={n} k={k}: {worst:.3e}")


@pytest.mark.parametrize("B,n,k,vmax", cases.POOL_MIRRORED)
def test_pool_delayed_mirrored_flush(hip, oracle, B, n, k, vmax):
    """k_flush_sym + k_sym_repair (symmetric_gather=True, N >= 256) on a full Sigma.  First run: at most k corrections, so
    its only flush is the closing one -- from the same base bit-identical to the plain flush on and above the diagonal
    tiles and the exact mirror image below (test_mirrored_flush_of_the_symmetric_option).  Then two more runs (a run
    boundary inside the steps under test, two flushes and more): mirror image again, 1e-9 against the checker at every
    run boundary"""
    log = cases.survey_log(n, vmax, B=B, seed=800 + n, extra_steps=cases.flush_steps(k, vmax))
    S, T = log.survey_steps, log.steps
    one = S + max(1, k // vmax)
    mid = one + (T - one) // 2
    assert one < mid < T
    filters = list(range(B))
    traces, _ = _traces(oracle, log, filters)
    tile = np.arange(3 + 2 * n) // 32
    above = tile[:, None] < tile[None, :]
    on_or_above = tile[:, None] <= tile[None, :]
    res, worst = [], 0.0
    for rows in (0, 16):                      # rows_per_block != 0 pins the plain row-block flush
        bt, launches = _delayed_pool_run(hip, log, k, lambda bt: bt.set_tuning(rows_per_block=rows), (one,), symmetric=True)
        fc = bt.form_counts()
        assert launches == 1
        assert (fc["flush_mirrored"], fc["flush_plain"] + fc["flush_strip"]) == ((1, 0) if rows == 0 else (0, 1)), fc
        res.append({b: (bt.state(b), bt.cov(b)) for b in filters})
        if rows == 0:
            worst = _pool_vs_checker(bt, traces, one - S, filters, f"k_flush_sym B={B} n={n} k={k}: first flush", "k_flush_sym")
            for t0, t1 in ((one, mid), (mid, T)):
                bt.run_known(t0, t1)
                worst = max(worst, _pool_vs_checker(bt, traces, t1 - S, filters, f"k_flush_sym B={B} n={n} k={k}: run to step {t1 - S}", "k_flush_sym"))
                for b in filters:
                    m = bt.cov(b)
                    assert np.array_equal(m.T[above], m[above]), f"filter {b}: mirror image behind step {t1 - S}"
            fc = bt.form_counts()
            assert fc["flush_mirrored"] >= 3 and fc["flush_plain"] + fc["flush_strip"] == 0, fc
        bt.close()
    for b in filters:
        m, p = res[0][b][1], res[1][b][1]
        assert np.array_equal(res[0][b][0], res[1][b][0]), f"filter {b} state"
        assert np.array_equal(m[on_or_above], p[on_or_above]), f"filter {b}: tiles on and above the diagonal"
        assert np.array_equal(m.T[above], m[above]), f"filter {b}: mirror image"
    print(f"measured pool mirrored flush B={B} n={n} k={k}: {worst:.3e}")


@pytest.mark.parametrize("B,n,k,vmax,strip", cases.POOL_PANEL)
def test_pool_delayed_column_panel_and_current_columns(hip, oracle, B, n, k, vmax, strip):
    """EKF_FORM_COLUMN_PANEL on / off / one-slot and EKF_FORM_CURRENT_COLUMNS on / off on a full Sigma, in one run and in
    four runs that hand the panel over: the panel forms bit-identical to the run without the panel, the current-columns
    forms within 1e-10 of it (test_column_panel_is_bit_identical's relations), all against the checker"""
    log = cases.survey_log(n, vmax, B=B, seed=900 + n, extra_steps=cases.POOL_PANEL_STEPS)
    S, T = log.survey_steps, log.steps
    filters = list(range(B))
    traces, _ = _traces(oracle, log, filters)
    base = hip.FORMS_DEFAULT | (hip.FORM_STRIP_FLUSH_ALWAYS if strip else 0)
    nocur = base & ~hip.FORM_CURRENT_COLUMNS
    variants = {"panel": nocur, "one_slot": nocur | hip.FORM_COLUMN_PANEL_ONE_SLOT, "off": base & ~hip.FORM_COLUMN_PANEL,
                "current": base, "current_one_slot": base | hip.FORM_COLUMN_PANEL_ONE_SLOT}
    outs, counts, worst = {}, {}, 0.0
    for name, forms in variants.items():
        for cuts in ((T,), (S + 3, S + 4, S + 9, T)):
            bt, _ = _delayed_pool_run(hip, log, k, lambda bt: bt.set_forms(forms), cuts)
            assert bt.forms == forms
            worst = max(worst, _pool_vs_checker(bt, traces, T - S, filters, f"column panel '{name}' {cuts} B={B} n={n} k={k}",
                                                f"k_flush{'_strip' if strip else ''} + gain kernels, forms {forms:#x}"))
            counts[name, cuts] = bt.form_counts()
            outs[name, cuts] = {b: (bt.state(b), bt.cov(b)) for b in filters}
            bt.close()
    for (name, cuts), got in outs.items():
        ref = outs["off", cuts]
        for b in filters:
            if name.startswith("current"):
                assert np.abs(got[b][0] - ref[b][0]).max() < 1e-10, f"{name} {cuts}, filter {b}"
                assert np.abs(got[b][1] - ref[b][1]).max() / np.abs(ref[b][1]).max() < 1e-10, f"{name} {cuts}, filter {b}"
            else:
                _same_bits(got[b], ref[b], f"{name} {cuts}, filter {b}")
    assert counts["off", (T,)]["gain_from_panel"] == 0
    for name in ("panel", "one_slot", "current"):
        c1, c4 = counts[name, (T,)], counts[name, (S + 3, S + 4, S + 9, T)]
        assert c4["gain_from_panel"] > 0, c4
        if c1["flush_plain"] + c1["flush_strip"] >= 2:
            assert c1["gain_from_panel"] > 0, c1
    print(f"measured pool column panel B={B} n={n} k={k}: {worst:.3e}")


@pytest.mark.parametrize("B,n", cases.POOL_UNKNOWN)
def test_pool_unknown_association_on_a_surveyed_map(hip, oracle, B, n):
    """run_known over the survey, then run_unknown over 4 steps of readings of the same world: four launches per slot,
    one launch per step, the separate streaming pass (n = 300: k_pool_step_unknown + k_rank2v, every step a run of its
    own so that the known counts are fresh), delayed k = 32 with EKF_FORM_STEP_SPECULATE on and off.  Decisions equal the
    checker's data_association(); the eager forms bit-identical (test_step_fused_beyond_the_small_path,
    test_step_with_a_separate_streaming_pass), the two delayed forms bit-identical
    (test_speculative_old_part_is_bit_identical) and within 1e-9 of the eager run; Sigma entrywise against the checker"""
    log = cases.unknown_case_log(B, n)
    S, T = log.survey_steps, log.steps
    tw, count, meas, truth = log.unknown_tail()
    filters = list(range(B))
    traces, _ = cases.checker_pool(oracle, log, filters, unknown=True)
    for b in filters:
        cases.require_preconditions([c for _, c in traces[b][0]], f"unknown n={n} filter {b}")
    want_dec = np.stack([traces[b][1] for b in filters], axis=1)          # [steps, B, J]
    snap, worst = {}, 0.0
    runs = {"four launches": (0, 0, None), "step-fused": (1, 0, None), "one launch": (2, 0, None),
            "delayed speculate": (1, cases.POOL_UNKNOWN_DELAYED_K, hip.FORMS_DEFAULT),
            "delayed": (1, cases.POOL_UNKNOWN_DELAYED_K, hip.FORMS_DEFAULT & ~hip.FORM_STEP_SPECULATE)}
    for name, (fused, k, forms) in runs.items():
        bt = _pool(hip, log)
        if forms is not None:
            bt.set_forms(forms)
        bt.set_step_fused(fused)
        bt.run_known(0, S)
        bt.set_known_counts(n)
        bt.set_update_mode(k)
        bt.upload_unknown_log(tw, count, meas)
        kernel = f"unknown association '{name}'"
        if k:    # (a run boundary flushes: two runs)
            bt.run_unknown(0, 2); bt.run_unknown(2, T - S)
        else:
            for t in range(T - S):
                bt.run_unknown(t, t + 1)
                for b in filters:
                    worst = max(worst, cases.assert_entrywise(bt.state(b), bt.cov(b), *traces[b][0][t + 1], FP64_TOL,
                                                              f"{kernel} n={n} step {t} filter {b}", kernel))
        dec = bt.decisions()
        assert np.array_equal(dec, want_dec), f"{kernel}: decisions differ from the checker's"
        assert np.array_equal(bt.known_counts(), np.full(B, n))
        for b in filters:
            s, c = bt.state(b), bt.cov(b)
            worst = max(worst, cases.assert_entrywise(s, c, *traces[b][0][-1], FP64_TOL, f"{kernel} n={n} filter {b}", kernel))
            assert_parity(s, c, *traces[b][0][-1], FP64_TOL, f"{kernel} n={n} filter {b}")
        fc = bt.form_counts()
        if k:   # the delayed forms really flushed (a run boundary and the end of the run at the least)
            assert fc["flush_plain"] + fc["flush_strip"] >= 2, fc
        if name == "step-fused":
            assert (fc["step_split_passes"] > 0) == (n >= 300), fc      # the separate streaming pass: N >= 603 only
        if name in ("four launches", "one launch"):
            assert fc["step_split_passes"] == 0, fc
        snap[name] = {b: (bt.state(b), bt.cov(b)) for b in filters}
        bt.close()
    for b in filters:
        _same_bits(snap["step-fused"][b], snap["four launches"][b], f"n={n} filter {b}: step-fused vs four launches")
        _same_bits(snap["one launch"][b], snap["four launches"][b], f"n={n} filter {b}: one launch vs four launches")
        _same_bits(snap["delayed speculate"][b], snap["delayed"][b], f"n={n} filter {b}: speculation on vs off")
        assert_parity(*snap["delayed"][b], *snap["four launches"][b], FP64_TOL, f"n={n} filter {b}: delayed vs eager")
    print(f"measured pool unknown B={B} n={n}: {worst:.3e}")


def test_maha_scores_on_a_surveyed_map(hip, oracle):
    """k_maha (calculate_maha_dis, ekf_slam.cpp:217-276) for every landmark of a surveyed n = 260 filter: every score reads
    a full 5 x 5 neighbourhood of Sigma; test_golden_maha's tolerances"""
    n = cases.MAHA_N
    log = cases.survey_log(n, cases.SINGLE_VMAX, seed=100 + n)
    S = log.survey_steps
    f, o = hip.EKF_SLAM(n), oracle.OracleEKF(n, oracle.STRUCTURED)
    for t in range(S):
        sensor, vis = log.expand_step(t)
        f.prediction(log.twist[t, 0]); o.prediction(*log.twist[t, 0])
        f.measurement(sensor, vis); o.measurement(sensor, vis)
    cases.require_preconditions([o.cov, cases.checker_trace(oracle, log, 0)[1][1]], "maha")
    f.prediction(log.twist[S, 0]); o.prediction(*log.twist[S, 0])     # the readings of step S are taken from its pose
    worst = 0.0
    for v in range(3):
        m = log.z_xy[S, 0, v]
        got = f.maha_scores(m, n)
        want = np.array([o.maha(m[0], m[1], i) for i in range(n)])
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
        assert np.abs(got - want).max() / np.abs(want).max() < FP64_TOL
        assert np.abs((got - want) / want).max() < 1e-7  # each score individually, too
        assert int(np.argmin(got)) == int(log.lm_idx[S, 0, v])
    f.close()
    print(f"measured maha n={n}: {worst:.3e}")
