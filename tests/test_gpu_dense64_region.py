"""-m gpu: a local region of the fp64 dense handle (ekf_dense64_region_begin .. ekf_dense64_region_end), on the chains and the
numpy model of tests/dense_region_cases.py, always on a COUPLED tail.  1. inside a region the corner, x_a, S, nis and the flags
are bit for bit those of a handle created with N = Na (the chains of dense_live_cases, every (m, s)); 2. after region_end the
whole Sigma and x equal the numpy model bit for bit on the exact integer chains, a second run repeats the bits, the padding
holds nothing that a product over it would show; 3. on general SPD chains -- eager, and deferred with the carry on and off --
the whole Sigma and x agree with a full-width twin within FP64_TOL; 4. an empty region keeps every bit; 5. NaNs and -0.0 in a
tail landmark reach nothing they did not reach on the twin; 6. every kind of call outside a region's terms ends it, counts,
restores live and returns what the twin returns; 7. refusals change nothing; 8. N = 10003, Na = 403: 64 corrections with a
prediction every eighth and region_end take less time than the same calls full-width.
tests/test_dense64_region_host.py proves the exact chains exact in float64."""
import time

import numpy as np
import pytest

import dense_block_cases as bc
import dense_landmark_cases as ll
import dense_live_cases as lc
import dense_region_cases as rc
import dense_scan_cases as sc
from parity import FP64_TOL, worst
from test_gpu_dense64_live import _call
from test_gpu_dense64_sparse import _full_size_sigma, _same_bits

pytestmark = pytest.mark.gpu
PAIR_IDS = [f"N{N}-Na{Na}" for N, Na in rc.pairs()]


def _corner(d, Na):
    """Sigma_aa through the block readout, in blocks, and x_a: neither leaves the region"""
    idx, step = np.arange(Na), max(1, 65536 // Na)
    return np.vstack([d.sigma_block(idx[k:k + step], idx) for k in range(0, Na, step)]), d.state_block(0, Na)


# ---- 1. the live contract inside a region ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Na", rc.pairs(), ids=PAIR_IDS)
def test_corner_bits_are_those_of_a_handle_of_dimension_na(hip, N, Na):
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(Na)
    for order in lc.ORDERS:
        for m, s in lc.shapes(Na):
            chain = rc.live_ops(Na, order, m, s)
            for carry in (True, False):
                S0, x0 = rc.coupled(chain["Sigma0"], chain["x0"], N, 11 * N + Na, integer=True)
                d.carry = twin.carry = carry
                d.set(Sigma=S0)
                d.state = x0
                twin.set(Sigma=chain["Sigma0"])
                twin.state = chain["x0"]
                d.region_begin(Na)
                assert d.live == Na and d.region_info()["active"]
                for i, op in enumerate(chain["ops"]):
                    at = (N, Na, order, m, s, carry, i, op["op"])
                    assert _call(d, op) == _call(twin, op), at
                    assert d.pending == twin.pending, at
                    cols, Hc, R, nu = op["cand"]
                    na, Sa, fa, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
                    nb, Sb, fb, _ = twin.score_sparse(cols, Hc, R, nu, want_S=True)
                    assert _same_bits(Sa, Sb) and _same_bits(na, nb) and np.array_equal(fa, fb), at
                    if carry or d.pending == 0:   # (without the carry a readout would flush: the corner behind a deferred
                        # correction is then compared only after the flush that the chain itself brings)
                        got, gx = _corner(d, Na)
                        assert _same_bits(got, twin.sigma_block(np.arange(Na), np.arange(Na))) and _same_bits(gx, twin.state), at
                info = d.region_info()
                assert info["active"] and info["ended_by_other_call"] == 0 and info["row_maps"] == 2
                assert info["corrections"] == 3
                rep = d.region_end()
                assert (rep["Na"], rep["Nb"], rep["corrections"], rep["row_maps"]) == (Na, N - Na, 3, 2)
                assert rep["group_bytes"] >= rc.plan(Na, N, d.launch_info()["ld"])["group_bytes"]
                assert d.live == N and not d.region_info()["active"]
                assert _same_bits(d.sigma[:Na, :Na], twin.sigma) and _same_bits(d.state[:Na], twin.state)
    d.close()
    twin.close()


# ---- 2. the model's bits on the exact chains --------------------------------------------------------------------------------------

def _run_region(d, ch, kinds=None):
    d.set(Sigma=ch["Sigma0"])
    d.state = ch["x0"]
    d.region_begin(ch["Na"])
    for op in ch["ops"]:
        _call(d, op if kinds is None else {**op, "op": kinds.get(op["op"], op["op"])})
    rep = d.region_end()
    return d.sigma, d.state, rep


@pytest.mark.parametrize("N,Na", rc.pairs(), ids=PAIR_IDS)
def test_after_region_end_sigma_and_state_are_the_models_bits(hip, N, Na):
    ch = rc.exact_chain(N, Na)
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)
    S, x, rep = _run_region(d, ch)
    bad = S != ch["Sigma"]
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4])
    assert np.array_equal(x, ch["x"])
    # Bit for bit.  Every number is exact, so a non-zero entry that is equal has the model's bits; what is left is the sign
    # of the zeros.  Outside the corner the device's order fixes it: Sigma_ab and Sigma_ba are fma chains from +0 (a chain
    # from +0 never ends at -0.0: +0 + -0 = +0, and an exact cancellation rounds to +0), Sigma_bb is the stored entry plus an
    # accumulator that starts at +0 -- so -(Psi Sigma0_ab) = -0.0 in Y can only add a -0 product to a +0 sum -- and x_b
    # starts at an integer of the chain, never -0.0.  Every zero there is therefore +0.0, which is what the model's value
    # plus +0.0 spells.  In the corner the order is the live call's: the bits are those of the twin of dimension Na.
    out = np.ones((N, N), dtype=bool)
    out[:Na, :Na] = False
    assert _same_bits(S[out], (ch["Sigma"] + 0.0)[out]) and _same_bits(x[Na:], ch["x"][Na:] + 0.0)
    small = hip.DensePropagator64(Na)
    small.set(Sigma=ch["Sigma0"][:Na, :Na])
    small.state = ch["x0"][:Na]
    for op in ch["ops"]:
        _call(small, op)
    assert _same_bits(S[:Na, :Na], small.sigma) and _same_bits(x[:Na], small.state)
    small.close()
    # the padding, read as it sits in memory: every bit zero
    Sp, xp = d.padded()
    assert _same_bits(Sp[:N, :N], S) and _same_bits(xp[:N], x)
    assert not Sp[N:, :].view(np.uint64).any() and not Sp[:, N:].view(np.uint64).any() and not xp[N:].view(np.uint64).any()
    assert rep["corrections"] == 2 and rep["row_maps"] == len(ch["ops"]) - 2
    twin.set(Sigma=ch["Sigma0"])                                       # the same calls at live = N
    twin.state = ch["x0"]
    for op in ch["ops"]:
        _call(twin, op)
    w, e = worst(x, S, twin.state, twin.sigma)
    print(f"region against the full-width twin, exact chain N = {N}, Na = {Na}: {w:.3e}")
    assert w <= FP64_TOL, e
    # the padding: I Sigma I^T + 0 on the matrix cores returns the same numbers unless a NaN or an Inf sits beyond column N
    d.set(F=np.eye(N), Q=np.zeros((N, N)))
    d.propagate(1)
    assert np.array_equal(d.sigma, ch["Sigma"])
    S2, x2, _ = _run_region(d, ch)                                     # a second run: the same bits
    assert _same_bits(S2, S) and _same_bits(x2, x)
    S3, x3, _ = _run_region(d, ch, {"eager": "deferred"})              # deferred: one correction per flush, the same bits
    assert _same_bits(S3, S) and _same_bits(x3, x)
    d.close()
    twin.close()


# ---- 3. general chains against a full-width twin ---------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Na", rc.pairs(), ids=PAIR_IDS)
def test_general_chains_agree_with_a_full_width_twin(hip, N, Na):
    ch = rc.float_chain(N, Na)
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)
    twin.set(Sigma=ch["Sigma0"])
    twin.state = ch["x0"]
    for op in ch["ops"]:
        _call(twin, {**op, "op": "eager"} if op["op"] == "deferred" else op)
    xt, St = twin.state, twin.sigma
    xm, Sm = rc.run_full(ch["Sigma0"], ch["x0"], ch["ops"])
    worst_of = 0.0
    for carry, kinds in ((False, {"deferred": "eager"}), (False, None), (True, None), (True, {"eager": "deferred"})):
        d.carry = carry
        S, x, rep = _run_region(d, ch, kinds)
        assert rep["corrections"] == len(lc.shapes(Na))
        for ref_x, ref_S in ((xt, St), (xm, Sm)):
            w, e = worst(x, S, ref_x, ref_S)
            worst_of = max(worst_of, w)
            assert w <= FP64_TOL, (carry, kinds, e)
    print(f"region against the full-width twin and numpy, N = {N}, Na = {Na}: worst per-block relative error {worst_of:.3e}")
    d.close()
    twin.close()


# ---- 4. an empty region ------------------------------------------------------------------------------------------------------------

def test_an_empty_region_keeps_every_bit(hip):
    N, Na = 200, 65
    rng = np.random.default_rng(4)
    S0 = rng.normal(size=(N, N))
    S0[3, 7], S0[100, 5], S0[150, 160] = -0.0, -0.0, -0.0
    x0 = rng.normal(size=N)
    d = hip.DensePropagator64(N)
    d.set(Sigma=S0)
    d.state = x0
    with d.region(Na) as reg:
        assert d.live == Na
    assert reg.report["corrections"] == 0 and reg.report["row_maps"] == 0 and d.live == N
    assert _same_bits(d.sigma, S0) and _same_bits(d.state, x0)
    d.close()


# ---- 5. NaN containment --------------------------------------------------------------------------------------------------------------

def test_nans_in_a_tail_landmark_reach_nothing_they_did_not_reach_on_the_twin(hip):
    N, Na = 200, 65                                                     # K of the product: 80, so columns 65 .. 79 are padding of K
    ch = rc.float_chain(N, Na, seed=9, shapes=[(2, 5), (1, 1), (2, 5)])
    S0, x0 = ch["Sigma0"].copy(), ch["x0"].copy()
    t = [Na + 10, Na + 11]                                              # inside the padded K range of the A operand
    S0[t, :Na], S0[:Na, t] = 0.0, 0.0                                   # Sigma_ab = 0 for that landmark
    S0[0, t[0]], S0[t[1], 1] = -0.0, -0.0
    pay = (np.uint64(0x7FF8000000000000) + np.arange(1, 2 * (N - Na) + 1, dtype=np.uint64)).view(np.float64)
    S0[t, Na:] = pay.reshape(2, -1)
    S0[Na:, t] = pay.reshape(2, -1).T
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)
    ops = [op for op in ch["ops"] if op["op"] != "init"]
    twin.set(Sigma=S0)
    twin.state = x0
    for op in ops:
        _call(twin, {**op, "op": "eager"} if op["op"] == "deferred" else op)
    S, x, _ = _run_region(d, {**ch, "Sigma0": S0, "x0": x0, "ops": ops})
    St, xt = twin.sigma, twin.state
    assert np.isnan(St).any() and not (np.isnan(S) & ~np.isnan(St)).any() and not (np.isnan(x) & ~np.isnan(xt)).any()
    ok = ~np.isnan(St)
    assert np.abs(S[ok] - St[ok]).max() <= FP64_TOL * max(1.0, np.abs(St[ok]).max())
    assert np.isfinite(x).all() and np.abs(x - xt).max() <= FP64_TOL * max(1.0, np.abs(xt).max())
    d.close()
    twin.close()


# ---- 6. calls outside a region's terms ---------------------------------------------------------------------------------------------

def _outside_calls(N, Na):
    H = np.zeros((1, N))
    H[0, [1, Na + 2]] = 1.0
    every = np.arange(N)
    return {
        "sigma": lambda h: h.sigma,
        "state": lambda h: h.state,
        "set_state": lambda h: setattr(h, "state", np.arange(N, dtype=np.float64)),
        "set": lambda h: h.set(F=np.eye(N)),
        "propagate": lambda h: h.propagate(0) and None,
        "correct": lambda h: h.correct(H, np.eye(1), np.ones(1))[0],
        "score": lambda h: h.score(H[None], np.eye(1), np.ones((1, 1)))[0],
        "swap_blocks": lambda h: h.swap_blocks(3, Na + 1, 2) and None,
        "health": lambda h: h.health()["n_nonfinite"],
        "symmetrize": lambda h: None if h.symmetrize() else None,
        "factor": lambda h: h.factor()["ok"],
        "coupling": lambda h: h.coupling(Na)[0],
        "set_live": lambda h: setattr(h, "live", N),
        "joseph": lambda h: h.correct_sparse_joseph(np.array([0, 4], dtype=np.int32), np.ones((1, 2)), np.eye(1), np.ones(1))[0],
        "sigma_block": lambda h: h.sigma_block(np.array([0, Na]), every[:8]),
        "state_block": lambda h: h.state_block(Na - 1, 2),
        "set_state_block": lambda h: h.set_state_block(Na - 1, np.array([1.5, -2.5])),
        "landmark_pairs": lambda h: h.landmark_pairs(4, 0.1, 5.0)[1],
    }


@pytest.mark.parametrize("name", sorted(_outside_calls(200, 65)))
def test_a_call_outside_the_terms_ends_the_region_first(hip, name):
    N, Na = 200, 65
    ch = rc.float_chain(N, Na, seed=2, shapes=[(2, 5), (1, 1)])
    call = _outside_calls(N, Na)[name]
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)
    for h in (d, twin):
        h.set(Sigma=ch["Sigma0"])
        h.state = ch["x0"]
    d.region_begin(Na)
    for op in ch["ops"]:
        _call(d, op)
        _call(twin, {**op, "op": "eager"} if op["op"] == "deferred" else op)
    assert d.region_info()["ended_by_other_call"] == 0
    a, b = call(d), call(twin)
    info = d.region_info()
    assert not info["active"] and info["ended_by_other_call"] == 1 and d.live == N
    if a is not None:
        assert np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=FP64_TOL, atol=FP64_TOL), name
    w, e = worst(d.state, d.sigma, twin.state, twin.sigma)
    assert w <= FP64_TOL, (name, e)
    with pytest.raises(hip.EkfError):
        d.region_end()                                                  # nothing is open any more
    d.close()
    twin.close()


# the calls of the landmark front end, the frame, the pairs, the joint association and the scans: on a map of landmarks
def _map_fixture():
    n, k = 10, 4                                                        # N = 23, the region holds the pose and 4 landmarks
    x, S = ll.spiral_map(n)
    v = np.random.default_rng(8).normal(size=3 + 2 * n)
    S = 0.5 * (S + S.T) + 1e-5 * np.outer(v, v)                         # symmetric, SPD, every landmark coupled with every other
    return n, k, x, S


def _map_calls(hip, n, x):
    rd = np.array([ll.reading_of(x, 1), ll.reading_of(x, 6)])
    c, s_ = np.cos(0.3), np.sin(0.3)
    vis = np.zeros(n, dtype=np.uint8)
    vis[[1, 6]] = 1
    sensor = np.array([ll.reading_of(x, i) for i in range(n)])
    scan = sc.circles_scan(3)
    return {
        "map_congruence": lambda h: h.map_congruence(np.array([[c, -s_], [s_, c]])) and None,
        "reframe": lambda h: h.reframe(hip.DensePropagator64.FRAME_FIXED, 0.2, 0.5, -0.25) and None,
        "merge_landmarks": lambda h: h.merge_landmarks(2, 7, 0.5, n)[2],
        "score_readings": lambda h: h.score_readings(rd, count=n)[0],
        "joint_operands": lambda h: h.joint_operands([1, 6], rd)[1],
        "associate_joint": lambda h: h.associate_joint(rd, n, n)[1],
        "associate_scan": lambda h: h.associate_scan(scan, n, n)[2],
        "associate_scan_joint": lambda h: h.associate_scan_joint(scan, n, n)[2],
        "measure_joseph": lambda h: h.measure_landmarks(sensor, vis, True, joseph=True)[1],
        "associate_joseph": lambda h: h.associate_landmarks(rd, n, n, joseph=True)[1],
    }


MAP_CALLS = ["map_congruence", "reframe", "merge_landmarks", "score_readings", "joint_operands", "associate_joint",
             "associate_scan", "associate_scan_joint", "measure_joseph", "associate_joseph"]


@pytest.mark.parametrize("name", MAP_CALLS)
def test_a_map_call_outside_the_terms_ends_the_region_first(hip, name):
    n, k, x, S = _map_fixture()
    calls = _map_calls(hip, n, x)
    assert sorted(calls) == sorted(MAP_CALLS)
    d, twin = hip.DensePropagator64(3 + 2 * n), hip.DensePropagator64(3 + 2 * n)
    for h in (d, twin):
        h.set(Sigma=S)
        h.state = x
    d.region_begin(3 + 2 * k)
    for h in (d, twin):
        h.predict_landmarks(0.05, 0.1)
        h.associate_landmarks([ll.reading_of(x, 1)], k if h is d else n, k if h is d else n)
    info = d.region_info()
    assert info["active"] and info["corrections"] == 1 and info["row_maps"] == 1 and info["ended_by_other_call"] == 0
    a, b = calls[name](d), calls[name](twin)
    info = d.region_info()
    assert not info["active"] and info["ended_by_other_call"] == 1 and d.live == twin.live
    if a is not None:
        assert np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=FP64_TOL, atol=FP64_TOL), (name, a, b)
    w, e = worst(d.state, d.sigma, twin.state, twin.sigma)
    assert w <= FP64_TOL, (name, e)
    d.close()
    twin.close()


def test_a_refused_call_outside_the_terms_leaves_the_region_open(hip):
    n, k, x, S = _map_fixture()
    d = hip.DensePropagator64(3 + 2 * n)
    d.set(Sigma=S)
    d.state = x
    d.region_begin(3 + 2 * k)
    d.predict_landmarks(0.05, 0.1)
    for bad in (lambda: d.swap_blocks(3, 4, 2), lambda: d.coupling(0), lambda: setattr(d, "live", 0),
                lambda: d.landmark_pairs(n + 1, 0.1), lambda: d.score_readings(np.zeros((1, 2)), count=n + 1)):
        with pytest.raises((hip.EkfError, ValueError)):
            bad()
        info = d.region_info()
        assert info["active"] and info["ended_by_other_call"] == 0 and d.live == 3 + 2 * k
    d.region_end()
    d.close()


# ---- 6b. the reference's data_association() inside a region ------------------------------------------------------------------

def test_data_association_with_the_known_landmarks_split_into_a_region_and_a_coupled_tail(hip):
    """n = 10 known landmarks on a coupled map, the robot sees the first k = 4 for three ticks.  `full`: predict_landmarks and
    ONE associate_landmarks per tick at known = n.  `one`: the same two calls inside a region over the pose and the k
    landmarks (known = n_max = k there).  `loop`: the prediction spelled and dense_landmark_cases.np_associate -- the
    reference's loop through state_block, score_sparse, correct_sparse and set_state_block -- inside a region.  `probe`:
    score_landmarks and measure_landmarks inside a region against the full-width calls.  The decisions are identical; after
    region_end Sigma and x agree with the full-width run within FP64_TOL."""
    n, k, x, S = _map_fixture()
    N, Na = 3 + 2 * n, 3 + 2 * k
    full, one, loop, probe, probe_full = (hip.DensePropagator64(N) for _ in range(5))
    for h in (full, one, loop, probe, probe_full):
        h.set(Sigma=S)
        h.state = x
    for h in (one, loop, probe):
        h.region_begin(Na)
    total = 0
    for t, (dth, dx) in enumerate([(0.05, 0.1), (-0.02, 0.08), (0.0, 0.05)]):
        readings = np.array([ll.reading_of(full.state_block(0, N), i, off=(0.004 * (t + 1), -0.003)) for i in ((0, 2, 3), (1, 3), (2, 0, 1))[t]])
        Fr, Qr, upd = bc.model_operands(loop.state_block(0, 3), dth, dx)
        loop.propagate_block(0, Fr, Qr, upd)
        kl, a_loop, best_loop = ll.np_associate(loop, None, readings, k, k)
        full.predict_landmarks(dth, dx)
        one.predict_landmarks(dth, dx)
        nis_full = full.score_landmarks(readings[0][0], readings[0][1], count=n)[0]
        nis_one = one.score_landmarks(readings[0][0], readings[0][1], count=k)[0]
        assert np.allclose(nis_one, nis_full[:k], rtol=1e-9, atol=0.0) and int(np.argmin(nis_full)) < k
        kf, a_full, best_full, _ = full.associate_landmarks(readings, n, n)
        ko, a_one, best_one, _ = one.associate_landmarks(readings, k, k)
        assert list(a_one) == list(a_full) == list(a_loop) and (a_full >= 0).all(), (t, a_one, a_full, a_loop)
        assert kf == n and ko == kl == k
        assert np.allclose(best_one, best_full, rtol=1e-9, atol=0.0) and np.allclose(best_loop, best_full, rtol=1e-9, atol=0.0)
        total += len(readings)
    sensor = np.array([ll.reading_of(x, i) for i in range(n)])
    vis = np.zeros(n, dtype=np.uint8)
    vis[[0, 3]] = 1
    probe.predict_landmarks(0.01, 0.02)
    probe_full.predict_landmarks(0.01, 0.02)
    assert probe.measure_landmarks(sensor[:k], vis[:k], True)[1] == probe_full.measure_landmarks(sensor, vis, True)[1] == 2
    for h, corr, maps in ((one, total, 3), (loop, total, 3), (probe, 2, 1)):
        info = h.region_info()
        assert info["active"] and info["ended_by_other_call"] == 0 and (info["corrections"], info["row_maps"]) == (corr, maps)
        h.region_end()
    for h, ref in ((one, full), (loop, full), (probe, probe_full)):
        w, e = worst(h.state, h.sigma, ref.state, ref.sigma)
        print(f"data_association in a region against the full-width run: {w:.3e}")
        assert w <= FP64_TOL, e
    assert not np.array_equal(full.sigma[Na:, Na:], S[Na:, Na:])       # the tail did owe something
    for h in (full, one, loop, probe, probe_full):
        h.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(hip):
    N, Na = 65, 5
    ch = rc.exact_chain(N, Na)
    d = hip.DensePropagator64(N)
    d.set(Sigma=ch["Sigma0"])
    d.state = ch["x0"]
    for bad in (2, 0, -1, N, N + 1):
        with pytest.raises(hip.EkfError):
            d.region_begin(bad)
    with pytest.raises(hip.EkfError):
        d.region_end()
    assert not d.region_info()["active"] and d.live == N
    d.region_begin(Na)
    _call(d, ch["ops"][0])
    before = _corner(d, Na)
    with pytest.raises(hip.EkfError):
        d.region_begin(Na)                                              # nested
    one = ch["ops"][0]
    with pytest.raises(hip.EkfError):
        d.correct_sparse(np.array([0, Na], dtype=np.int32), np.ones((1, 2)), one["R"], one["nu"])
    with pytest.raises(hip.EkfError):
        d.propagate_block(Na - 1, np.eye(2))
    with pytest.raises(hip.EkfError):
        d.init_block(Na - 1, r=2, W=np.eye(2))
    info = d.region_info()
    assert info["active"] and info["Na"] == Na and info["corrections"] == 1 and info["ended_by_other_call"] == 0
    after = _corner(d, Na)
    assert _same_bits(before[0], after[0]) and _same_bits(before[1], after[1])
    for op in ch["ops"][1:]:
        _call(d, op)
    d.region_end()
    assert np.array_equal(d.sigma, ch["Sigma"]) and np.array_equal(d.state, ch["x"])
    d.close()


def test_plan_through_the_library(hip):
    d = hip.DensePropagator64(403)
    ld = d.launch_info()["ld"]
    for Na in (3, 64, 129, 191, 402):
        got, want = d.region_launch_info(Na), rc.plan(Na, 403, ld)
        assert all(got[k] == want[k] for k in got), (Na, got, want)
    d.close()


# ---- 8. the size the handle was made for -------------------------------------------------------------------------------------------

def test_region_full_size_n10003_and_time(hip):
    """64 correct_sparse(2, 5) with a propagate_block(r = 3) every eighth call inside a region of Na = 403, plus region_end,
    against the same calls full-width on a twin in the same process (the path without regions): the sums of the calls' own
    HIP-event times, after one untimed pass of both.  Condition: the region's sum is the smaller one.  The states agree
    within FP64_TOL on sampled rows and columns."""
    N, Na = 10003, 403
    rng = np.random.default_rng(27)
    S0 = _full_size_sigma(N, rng)
    S0 = 0.5 * (S0 + S0.T)                                              # surveyed: coupled everywhere, symmetric
    x0 = rng.normal(size=N)
    ops = []
    for i in range(64):
        lm = 3 + 2 * int(rng.integers(0, (Na - 3) // 2))
        ops.append(("c", np.array([0, 1, 2, lm, lm + 1], dtype=np.int32), rng.normal(size=(2, 5)), 0.5 * np.eye(2), 0.1 * rng.normal(size=2)))
        if i % 8 == 7:
            ops.append(("p", np.eye(3) + 0.01 * rng.normal(size=(3, 3)), 1e-3 * np.eye(3), 0.01 * rng.normal(size=3)))
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)

    def run(h, region):
        h.set(Sigma=S0)
        h.state = x0
        ms, t0 = 0.0, time.perf_counter()
        if region:
            ms += h.region_begin(Na)
        for op in ops:
            ms += h.correct_sparse(*op[1:])[1] if op[0] == "c" else h.propagate_block(0, op[1], op[2], op[3])
        in_region = ms
        end = h.region_end() if region else None
        if region:
            ms += end["elapsed_ms"]
        return ms, in_region, end, time.perf_counter() - t0

    run(d, True), run(twin, False)                                      # untimed: allocations, first launches
    t_reg, t_in, end, wall_reg = run(d, True)
    t_full, _, _, wall_full = run(twin, False)
    flop = 2.0 * Na * (N - Na) ** 2
    print(f"N = {N}, Na = {Na}: region {t_reg:.3f} ms (in-region {t_in:.3f} ms = {t_in / 64:.4f} ms per correction, region_end "
          f"{end['elapsed_ms']:.3f} ms, {flop / end['elapsed_ms'] / 1e9:.1f} TF if it were the Sigma_bb product alone), "
          f"full width {t_full:.3f} ms ({t_full / 64:.4f} ms per correction); wall {wall_reg * 1e3:.1f} / {wall_full * 1e3:.1f} ms")
    rows = np.sort(rng.permutation(N)[:6])
    rows[0], rows[1] = 5, Na                                            # the region, the tile that straddles Na, the tail
    every = np.arange(N)
    a = np.vstack([d.sigma_block(rows[k:k + 6], every) for k in range(0, len(rows), 6)])
    b = np.vstack([twin.sigma_block(rows[k:k + 6], every) for k in range(0, len(rows), 6)])
    err = max(np.abs(a - b).max() / np.abs(b).max(), np.abs(d.state - twin.state).max() / np.abs(twin.state).max())
    print(f"sampled rows and the state against the full-width twin: {err:.3e}")
    assert err <= FP64_TOL
    assert t_reg < t_full, (t_reg, t_full)
    d.close()
    twin.close()
