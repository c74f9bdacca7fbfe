"""-m gpu: ekf_dense64_join_congruence and ekf_dense64_join_map (ekf_dense64_join.hip) against the models of dense_join_cases.
Sizes around both tile sides the library reports (the odd numbers nearest {3, 5, 7, T - 1, T, T + 1, 2 T + 1, 3 T + 2}): Nb over
all of them against Na in {3, 7, T_c + 1}, Na over all of them against Nb in {3, 5}.  The destination is created once with
N = Na' and once with N = Na' + 5, the source with N = Nb and with N = Nb + 5; everything outside both live corners is poisoned
with payload NaNs.  1. the integer families, bit for bit; 2. floats against the componentwise bound; 3. no symmetrisation, and
b = 0; 4. join_map; 5. pending rows and regions; 6. refusals; 7. DenseEKFSLAM end to end; 8. N = 10003 and the time."""
import ctypes
import math
import time

import numpy as np
import pytest

import dense_join_cases as jn
import dense_model_cases as dm
from parity import FP64_TOL, worst
from test_gpu_dense64_live import _poison
from test_gpu_dense64_sparse import _full_size_sigma, _median

pytestmark = pytest.mark.gpu
_TILES, _REF, _NOTES = [], {}, {}
N_SIZES = len(jn.sizes(64, 128))   # the number of distinct sizes does not depend on the tile sides as long as they differ
TAILS = [(0, 0), (5, 0), (0, 5), (5, 5)]   # (the destination's, the source's) rows and columns beyond what the join needs


def _tiles(hip):
    if not _TILES:
        d = hip.DensePropagator64(3)
        info = d.join_launch_info()
        d.close()
        assert info["threads"] == 256 and info["tile_rows"] % 2 == 0 and info["tile_cols"] % 2 == 0
        _TILES.extend([info["tile_rows"], info["tile_cols"]])
    return _TILES


def _pairs_of_sizes(hip, k, side):
    """side "nb": Nb = sizes[k] against Na in {3, 7, T_c + 1};  side "na": Na = sizes[k] against Nb in {3, 5}"""
    Tr, Tc = _tiles(hip)
    s = jn.sizes(Tr, Tc)
    assert len(s) == N_SIZES
    return [(Na, s[k]) for Na in (3, 7, jn.odd_near(Tc + 1))] if side == "nb" else [(s[k], Nb) for Nb in (3, 5)]


def _handle(hip, corner, N, x=None):
    """a handle of dimension N that holds `corner` in its live corner; everything else is poison"""
    n = corner.shape[0]
    x = np.arange(1.0, n + 1.0) if x is None else x
    S, xs = _poison(N, n, corner, x)
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = xs
    d.live = n
    return d, S, xs


def _pair(hip, SA, SB, tails, xa=None, xb=None):
    Na, Nb = SA.shape[0], SB.shape[0]
    dst = _handle(hip, SA, Na + Nb - 3 + tails[0], xa)
    src = _handle(hip, SB, Nb + tails[1], xb)
    return dst, src


def _expect(S, corner):
    want = S.copy()
    want[:corner.shape[0], :corner.shape[0]] = corner
    return want


def _note(key, text):
    """the figures of this run; the full-size test prints them together (profiles/r28/dense64_join_bench.txt is that output)"""
    _NOTES[key] = text


CASES = [(k, side) for side in ("nb", "na") for k in range(N_SIZES)]
CASE_IDS = [f"{side}-size{k}" for k, side in CASES]


# ---- 1. integer families ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,side", CASES, ids=CASE_IDS)
def test_join_integer_families_bit_for_bit(hip, k, side):
    for Na, Nb in _pairs_of_sizes(hip, k, side):
        SA, SB, E = jn.integer_corner(Na), jn.integer_corner(Nb, seed=1), jn.integer_E(Nb)
        for family, G in sorted(jn.GS.items()):
            corner = jn.exact_join(SA, SB, G, E)
            assert jn.same_bits(corner[3:Na, 3:Na], SA[3:Na, 3:Na])
            for tails in TAILS:
                (d, S, xs), (s, T, xt) = _pair(hip, SA, SB, tails)
                d.join_congruence(s, G, E)
                got, state, live = d.sigma, d.state, d.live
                src_after = (s.sigma, s.state, s.live)
                d.close(); s.close()
                what = f"{family} Na={Na} Nb={Nb} tails={tails}"
                assert live == Na + Nb - 3, what
                assert jn.same_bits(got[:live, :live], corner), what
                assert jn.same_bits(got, _expect(S, corner)), what + ": the poison moved"
                assert jn.same_bits(state, xs), what + ": the destination's state was touched"
                assert jn.same_bits(src_after[0], T) and jn.same_bits(src_after[1], xt) and src_after[2] == Nb, what + ": the source"


# ---- 2. floats --------------------------------------------------------------------------------------------------------------

def _float_case(Na, Nb):
    if (Na, Nb) not in _REF:
        SA, SB = jn.slam_like(Na), jn.slam_like(Nb, seed=1)
        G = np.array([[math.cos(0.7), -math.sin(0.7)], [math.sin(0.7), math.cos(0.7)]])
        E = np.random.default_rng(7000 + 31 * Na + Nb).standard_normal((Nb, 3))
        for a in (SA, SB, G, E):
            a.setflags(write=False)
        _REF[(Na, Nb)] = (SA, SB, G, E)
    return _REF[(Na, Nb)]


@pytest.mark.parametrize("k,side", CASES, ids=CASE_IDS)
def test_join_floats_within_the_componentwise_bound(hip, k, side):
    """|Sigma' - J S J^T|_ij <= gamma_14 (|J| |S| |J|^T)_ij against long double, gamma_3 on the cross entries and exact in the
    untouched corner (dense_join_cases.entry_gamma); the same bits from both N of the destination,
    both N of the source and from two runs; at Na, Nb <= 7 the op-by-op model bit for bit."""
    for Na, Nb in _pairs_of_sizes(hip, k, side):
        SA, SB, G, E = _float_case(Na, Nb)
        Nj, outs = Na + Nb - 3, []
        for tails in TAILS + [(5, 5)]:
            (d, S, xs), (s, T, xt) = _pair(hip, SA, SB, tails)
            d.join_congruence(s, G, E)
            got, after = d.sigma, s.sigma
            d.close(); s.close()
            assert jn.same_bits(got, _expect(S, got[:Nj, :Nj])) and jn.same_bits(after, T)
            assert jn.same_bits(got[3:Na, 3:Na], SA[3:Na, 3:Na])
            outs.append(got[:Nj, :Nj].copy())
        ratio = jn.bound_ratio(outs[0], SA, SB, G, E)
        print(f"Na={Na} Nb={Nb}: error / bound {ratio:.4f}")
        _note(("bound", Na, Nb), f"Na={Na} Nb={Nb}: max |err| / (gamma_k |J||S||J|^T), k = 14, 3 on the cross entries = {ratio:.4f}")
        assert all(jn.same_bits(outs[0], o) for o in outs[1:])
        assert ratio <= 1.0
        if Na <= 7 and Nb <= 7:
            assert jn.same_bits(outs[0], jn.np_join(SA, SB, G, E))


# ---- 3. no symmetrisation, the empty local map ----------------------------------------------------------------------------------

def test_non_symmetric_operands_give_the_non_symmetric_result(hip):
    Tr, Tc = _tiles(hip)
    Na, Nb = jn.odd_near(Tr + 1), jn.odd_near(Tc + 1)
    SA, SB, E, G = jn.integer_corner(Na), jn.integer_corner(Nb, seed=1), jn.integer_E(Nb), jn.GS["shear"]
    want = jn.exact_join(SA, SB, G, E)
    io = jn.iota(Na, Nb)
    assert not np.array_equal(want, want.T) and not np.array_equal(want[np.ix_(io, io)], want[np.ix_(io, io)].T)
    (d, S, xs), (s, T, xt) = _pair(hip, SA, SB, (5, 5))
    d.join_congruence(s, G, E)
    got = d.sigma
    d.close(); s.close()
    assert jn.same_bits(got, _expect(S, want))
    assert not jn.same_bits(got[:Na + Nb - 3, :Na + Nb - 3], jn.exact_join(SA.T.copy(), SB, G, E))
    assert not jn.same_bits(got[:Na + Nb - 3, :Na + Nb - 3], jn.exact_join(SA, SB.T.copy(), G, E))


@pytest.mark.parametrize("tails", [(0, 0), (5, 5)])
def test_b_zero_composes_the_pose_and_writes_the_pose_rows_and_columns_only(hip, tails):
    Tr, Tc = _tiles(hip)
    Na = jn.odd_near(Tc + 1)
    SA, SB, E, G = jn.integer_corner(Na), jn.integer_corner(3, seed=1), jn.integer_E(3), jn.GS["rot90"]
    (d, S, xs), (s, T, xt) = _pair(hip, SA, SB, tails)
    d.join_congruence(s, G, E)
    got, live = d.sigma, d.live
    d.close(); s.close()
    assert live == Na and jn.same_bits(got, _expect(S, jn.exact_join(SA, SB, G, E)))
    assert jn.same_bits(got[3:, 3:], S[3:, 3:])                 # nothing but the three pose rows and columns
    # join_map with an empty local map at the origin: the identity by value
    xa = jn.slam_state(Na)
    (d, S, xs), (s, T, xt) = _pair(hip, jn.slam_like(Na), np.zeros((3, 3)), tails, xa, np.zeros(3))
    d.join_map(s)
    got, state = d.sigma, d.state
    d.close(); s.close()
    assert np.array_equal(got[:Na, :Na], S[:Na, :Na]) and np.array_equal(state[:Na], xa)
    assert jn.same_bits(got[3:, 3:], S[3:, 3:]) and jn.same_bits(state[3:], xs[3:])


# ---- 4. join_map ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,side", CASES, ids=CASE_IDS)
def test_join_map(hip, k, side):
    """the state is the model's given the device's own cos and sin; within FP64_TOL of g with libm; theta' is not wrapped;
    the covariance is bit for bit join_congruence on a twin pair fed the terms that came back"""
    for Na, Nb in _pairs_of_sizes(hip, k, side):
        SA, SB = jn.slam_like(Na), jn.slam_like(Nb, seed=1)
        xa, xb = jn.slam_state(Na), jn.slam_state(Nb, seed=1)
        xa[0], xb[0] = 2.9, 0.6                                   # theta_A + theta_B > pi
        xb[1:3] = [0.8, -0.3]
        Nj = Na + Nb - 3
        for tails in ((0, 0), (5, 5)):
            (d, S, xs), (s, T, xt) = _pair(hip, SA, SB, tails, xa, xb)
            (tw, _, _), (ts, _, _) = _pair(hip, SA, SB, tails, xa, xb)
            G, E, _ = d.join_map(s, want_terms=True)
            tw.join_congruence(ts, G, E)
            got, state, live, twin = d.sigma, d.state, d.live, tw.sigma
            src_after = (s.sigma, s.state, s.live)
            for h in (d, s, tw, ts):
                h.close()
            assert live == Nj
            assert jn.same_bits(got, twin)                        # the poison included
            assert jn.same_bits(got[3:Na, 3:Na], SA[3:Na, 3:Na])
            c, sn = G[0, 0], G[1, 0]
            assert jn.same_bits(G, [[c, -sn], [sn, c]]) and abs(c - math.cos(xa[0])) <= 1e-15 and abs(sn - math.sin(xa[0])) <= 1e-15
            want_x, want_E = jn.state_model(xa, xb, c, sn)
            assert jn.same_bits(state[:Nj], want_x) and jn.same_bits(E, want_E)
            assert jn.same_bits(state[Nj:], xs[Nj:])
            assert state[0] == xa[0] + xb[0] > math.pi            # not wrapped
            assert jn.row_scale_err(state[:Nj][None, :], jn.g(xa, xb)[None, :]) <= FP64_TOL
            assert jn.row_scale_err(E, jn.join_terms(xa, xb)[1]) <= FP64_TOL
            assert jn.same_bits(src_after[0], T) and jn.same_bits(src_after[1], xt) and src_after[2] == Nb


# ---- 5. pending rows and regions ----------------------------------------------------------------------------------------------

def _deferred(h, n, count, seed=17):
    rng = np.random.default_rng(seed)
    for j in (1, n // 2 - 3)[:count]:
        cols = np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j])
        h.correct_sparse_deferred(cols, rng.standard_normal((2, 5)), 0.5 * np.eye(2), 0.1 * rng.standard_normal(2))


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("who", ["dst", "src"])
@pytest.mark.parametrize("count", [1, 2])
def test_pending_rows_are_flushed_first(hip, who, carry, count):
    """rows pending on the destination (carry on and off) or on the source: the join equals flush-first-then-join within
    FP64_TOL; with a single pending correction the bits match"""
    Tr, Tc = _tiles(hip)
    Na, Nb = jn.odd_near(Tr + 1), jn.odd_near(Tr + 3)
    SA, SB, xa, xb = jn.slam_like(Na), jn.slam_like(Nb, seed=1), jn.slam_state(Na), jn.slam_state(Nb, seed=1)
    runs = []
    for flush_first in (False, True):
        (d, _, _), (s, _, _) = _pair(hip, SA, SB, (5, 5), xa, xb)
        h, n = (d, Na) if who == "dst" else (s, Nb)
        h.carry = carry
        _deferred(h, n, count)
        assert h.pending == 2 * count
        if flush_first:
            h.flush()
            assert h.pending == 0
        d.join_map(s)
        assert d.pending == 0 and s.pending == 0 and d.live == Na + Nb - 3 and s.live == Nb
        runs.append((d.state, d.sigma, s.state, s.sigma))
        d.close(); s.close()
    Nj = Na + Nb - 3
    w, e = worst(runs[0][0][:Nj], runs[0][1][:Nj, :Nj], runs[1][0][:Nj], runs[1][1][:Nj, :Nj])
    assert w <= FP64_TOL, e
    assert jn.same_bits(runs[0][2], runs[1][2]) and jn.same_bits(runs[0][3], runs[1][3])   # the source after its own flush
    if count == 1:
        assert jn.same_bits(runs[0][0], runs[1][0]) and jn.same_bits(runs[0][1], runs[1][1])


def test_an_open_region_on_the_destination_ends_first(hip):
    Tr, Tc = _tiles(hip)
    Na, Nb, Nr = jn.odd_near(Tr + 1), 7, 9
    SA, SB, xa, xb = jn.slam_like(Na), jn.slam_like(Nb, seed=1), jn.slam_state(Na), jn.slam_state(Nb, seed=1)
    rng = np.random.default_rng(23)
    Hc, nu = rng.standard_normal((2, 5)), 0.1 * rng.standard_normal(2)
    runs = []
    for end_first in (False, True):
        (d, _, _), (s, _, _) = _pair(hip, SA, SB, (5, 5), xa, xb)
        ended = d.region_info()["ended_by_other_call"]
        d.region_begin(Nr)
        d.correct_sparse(np.array([0, 1, 2, 5, 6]), Hc, 0.5 * np.eye(2), nu)
        if end_first:
            d.region_end()
        d.join_map(s)
        info = d.region_info()
        assert not info["active"] and info["ended_by_other_call"] == ended + (0 if end_first else 1)
        assert d.live == Na + Nb - 3
        runs.append((d.state, d.sigma))
        d.close(); s.close()
    Nj = Na + Nb - 3
    w, e = worst(runs[0][0][:Nj], runs[0][1][:Nj, :Nj], runs[1][0][:Nj], runs[1][1][:Nj, :Nj])
    assert w <= FP64_TOL, e
    assert jn.same_bits(runs[0][0], runs[1][0]) and jn.same_bits(runs[0][1], runs[1][1])   # the same launches in the same order


def test_an_open_region_on_the_source_ends_first(hip):
    """the source is brought to Sigma in memory as get_sigma would: its region ends on its own stream, the destination's
    stream waits for it; the join equals end-first-then-join bit for bit, and the source is what region_end leaves"""
    Tr, Tc = _tiles(hip)
    Na, Nb, Nr = 7, jn.odd_near(Tr + 1), 9
    SA, SB, xa, xb = jn.slam_like(Na), jn.slam_like(Nb, seed=1), jn.slam_state(Na), jn.slam_state(Nb, seed=1)
    rng = np.random.default_rng(29)
    Hc, nu = rng.standard_normal((2, 5)), 0.1 * rng.standard_normal(2)
    runs = []
    for end_first in (False, True):
        (d, _, _), (s, _, _) = _pair(hip, SA, SB, (5, 5), xa, xb)
        ended = s.region_info()["ended_by_other_call"]
        s.region_begin(Nr)
        s.correct_sparse(np.array([0, 1, 2, 5, 6]), Hc, 0.5 * np.eye(2), nu)
        if end_first:
            s.region_end()
        G, E, _ = d.join_map(s, want_terms=True)
        info = s.region_info()
        assert not info["active"] and info["ended_by_other_call"] == ended + (0 if end_first else 1)
        assert d.live == Na + Nb - 3 and s.live == Nb and E.shape == (Nb, 3)
        runs.append((d.state, d.sigma, s.state, s.sigma, E, G))
        d.close(); s.close()
    assert all(jn.same_bits(p, q) for p, q in zip(runs[0], runs[1]))
    Nj = Na + Nb - 3                                              # ... and it is the join of what the source then holds
    assert jn.bound_ratio(runs[0][1][:Nj, :Nj], SA, runs[0][3][:Nb, :Nb], runs[0][5], runs[0][4]) <= 1.0


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(hip):
    """one case per rule (3) .. (7) and NULL G, on handles with rows pending, then on one inside a region.  RULE (4),
    DIFFERENT DEVICES, NEEDS A SECOND GPU: ON A MACHINE WITH ONE DEVICE THAT CASE DOES NOT RUN and this test says nothing
    about it (the order of the checks is then held by the header test and by reading dense64_join alone)."""
    Na, Nb = 13, 7
    SA, SB, xa, xb = jn.slam_like(Na), jn.slam_like(Nb, seed=1), jn.slam_state(Na), jn.slam_state(Nb, seed=1)
    (d, _, _), (s, _, _) = _pair(hip, SA, SB, (5, 5), xa, xb)
    (td, _, _), (ts, _, _) = _pair(hip, SA, SB, (5, 5), xa, xb)
    small, _, _ = _handle(hip, SA, Na + Nb - 4)                   # one state short of the joined map
    even, _, _ = _handle(hip, jn.slam_like(13)[:12, :12], 17, np.linspace(-1.0, 1.0, 12))
    for h in (d, s, td, ts):
        _deferred(h, Nb, 2)
    lib = hip.load()
    G, E, terms = np.eye(2), np.ones((Nb, 3)), np.full(4 + 3 * Nb, 7.0)
    cong = lambda a, b, g=G, e=E: lib.ekf_dense64_join_congruence(a._h, b._h, None if g is None else hip._d(g),
                                                                   None if e is None else hip._d(e), None)
    jmap = lambda a, b: lib.ekf_dense64_join_map(a._h, b._h, hip._d(terms), None)
    assert cong(d, d) == 1 and jmap(d, d) == 1 and b"same handle" in lib.ekf_last_error()             # (3)
    if hip.device_count() > 1:                                                                         # (4)
        far = hip.DensePropagator64(Nb, 1)
        assert cong(d, far) == 1 and jmap(d, far) == 1 and b"different devices" in lib.ekf_last_error()
        far.close()
    assert cong(even, s) == 1 and jmap(even, s) == 1 and cong(d, even) == 1 and jmap(d, even) == 1    # (5)
    assert b"3 + 2 n" in lib.ekf_last_error()
    assert cong(small, s) == 1 and jmap(small, s) == 1 and b"does not fit" in lib.ekf_last_error()    # (6)
    assert cong(d, s, None, E) == 1 and cong(d, s, G, None) == 1 and b"null G or E" in lib.ekf_last_error()   # (7)
    with pytest.raises(ValueError):
        d.join_congruence(s, G, np.ones((Nb - 1, 3)))                                                  # the wrapper's own
    with pytest.raises(ValueError):
        d.join_map(object())
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.ekf_dense64_join_launch_info(d._h, None, ctypes.byref(b), ctypes.byref(c)) == 1
    assert np.array_equal(terms, np.full(4 + 3 * Nb, 7.0))
    assert (d.pending, s.pending, d.live, s.live, small.live, even.live) == (4, 4, Na, Nb, Na, 12)
    same = all(jn.same_bits(p.sigma, q.sigma) and jn.same_bits(p.state, q.state) for p, q in ((d, td), (s, ts)))
    # an open region stays open through a refusal, on either side
    td.region_begin(7)
    ended = td.region_info()["ended_by_other_call"]
    assert cong(td, td) == 1 and cong(td, even) == 1 and cong(small, td) == 1 and cong(td, ts, None, E) == 1
    info = td.region_info()
    assert info["active"] and info["ended_by_other_call"] == ended and td.live == 7
    for h in (d, s, td, ts, small, even):
        h.close()
    assert same


# ---- 7. DenseEKFSLAM end to end -----------------------------------------------------------------------------------------------

def test_slam_filter_joins_a_local_map_and_fuses_what_both_saw(hip):
    """A global filter (room for 12) discovers six landmarks; a local filter started at the robot's pose maps four objects, two
    of them landmarks 1 and 4 of the global map seen again.  join(), then find_duplicates() names exactly (1, 6) and (4, 7),
    merge() leaves eight landmarks, the covariance is healthy and factors after symmetrize(), and state and Sigma of the join
    agree with the block formulas applied in numpy to the two read-out maps."""
    steps = dm.discovery_scenario(n=6, ticks=25)
    world = dm._world(6)
    f = hip.DenseEKFSLAM(12, grow_live=True)
    pose = np.zeros(3)
    for dth, dx, readings in steps:
        pose = pose + dm.bc.model_operands(pose, dth, dx)[2]
        f.prediction(dth, dx)
        f.data_association(readings)
    assert f.known == 6 and f.handle.live == 15
    objects = np.vstack([world[[1, 4]], [[4.5, 0.5], [-4.0, -2.5]]])
    local_xy = dm._body(pose, objects)                            # the objects in the frame of the robot's pose
    loc = hip.DenseEKFSLAM(4, grow_live=True)
    rng, lpose = np.random.default_rng(31), np.zeros(3)
    for t in range(3):
        dth, dx = dm._twist(t)
        lpose = lpose + dm.bc.model_operands(lpose, dth, dx)[2]
        loc.prediction(dth, dx)
        loc.data_association(dm._body(lpose, local_xy + rng.normal(0, 0.004, size=(4, 2))))
    assert loc.known == 4 and loc.handle.live == 11
    xa, SA = f.handle.state_block(0, 15), f.handle.sigma[:15, :15]
    xb, SB = loc.handle.state_block(0, 11), loc.handle.sigma[:11, :11]
    f.join(loc)
    assert f.known == 10 and f.handle.live == 23 and loc.known == 4 and loc.handle.live == 11
    G, E = jn.join_terms(xa, xb)
    want_S = np.asarray(jn.reference(SA, SB, G, E)[0], dtype=np.float64)
    w, e = worst(f.handle.state_block(0, 23), f.handle.sigma[:23, :23], jn.g(xa, xb), want_S)
    print(f"join against the block formulas in numpy: {w:.3e}")
    _note(("slam",), f"DenseEKFSLAM.join (15 + 11 states): worst |d| / scale against the numpy twin = {w:.3e}")
    assert w <= FP64_TOL, e
    gate, r_merge = 13.8, 0.01
    dups, below = f.find_duplicates(gate, r_merge)
    assert [(a, b) for a, b, _ in dups] == [(1, 6), (4, 7)], dups
    f.merge(4, 7, r_merge)                                        # landmark 9 moves into slot 7
    f.merge(1, 6, r_merge)                                        # landmark 8 moves into slot 6
    assert f.known == 8 and f.find_duplicates(gate, r_merge)[0] == []
    health = f.health()
    assert health["n_nonfinite"] == 0 and health["n_diag_bad"] == 0, health
    f.symmetrize()
    assert f.factor()["ok"] == 1
    got = f.state[3:3 + 16].reshape(8, 2)
    truth = np.vstack([world, objects[2:]])
    for p in truth:                                               # every object is in the map once, where it stands
        assert np.sum(np.hypot(*(got - p).T) < 0.1) == 1, (p, got)
    f.close(); loc.close()


# ---- 8. full size -----------------------------------------------------------------------------------------------------------

def _host_route(d, s, Na, Nb, G, E):
    """what a caller without the call does: both covariances down, the block formulas in numpy, the result up"""
    t0 = time.perf_counter()
    S, SB = d.sigma, s.sigma[:Nb, :Nb]

    def D(X):
        Y = X.copy()
        Y[1::2], Y[2::2] = G[0, 0] * X[1::2] + G[0, 1] * X[2::2], G[1, 0] * X[1::2] + G[1, 1] * X[2::2]
        return Y

    P, Pc, Spp = S[:3, :Na].copy(), S[:Na, :3].copy(), S[:3, :3].copy()
    Y = D(D(SB).T).T + E @ Spp @ E.T
    Xr, Xc = E @ P, Pc @ E.T
    Nj = Na + Nb - 3
    S[:3, :3], S[:3, Na:Nj], S[Na:Nj, :3], S[Na:Nj, Na:Nj] = Y[:3, :3], Y[:3, 3:], Y[3:, :3], Y[3:, 3:]
    S[:3, 3:Na], S[Na:Nj, 3:Na], S[3:Na, :3], S[3:Na, Na:Nj] = Xr[:3, 3:], Xr[3:, 3:], Xc[3:, :3], Xc[3:, 3:]
    d.set(Sigma=S)
    return (time.perf_counter() - t0) * 1e3


def _full_size_sample(rng, N, Na, Tr, Tc):
    """64 indices of the joined map: the pose (3), 21 of A's landmark states and 40 of B's appended ones -- in each range the
    edges of the range and of the tiles, filled up with seeded picks -- so that rows x columns reaches every launch's output"""
    def fill(edges, lo, hi, count):
        picked = set(edges)
        assert all(lo <= v < hi for v in picked)
        while len(picked) < count:
            picked.add(int(rng.integers(lo, hi)))
        return sorted(picked)
    out = np.array([0, 1, 2] + fill({3, 4, Tr + 2, Tr + 3, Na - 2, Na - 1}, 3, Na, 21) +
                   fill({Na, Na + 1, Na + Tr - 1, Na + Tr, Na + Tc - 1, Na + Tc, N - 2, N - 1}, Na, N, 40))
    assert out.shape == (64,) and np.sum(out < 3) == 3 and np.sum((out >= 3) & (out < Na)) == 21 and np.sum(out >= Na) == 40
    return out


def test_full_size_n10003_and_time(hip):
    """A destination of capacity 10003 with 4000 landmarks (Na = 8003) takes a local map of 1000 (Nb = 2003).  64 x 64 seeded
    entries -- rows and columns each drawn from the pose, from A's landmarks and from B's appended ones (_full_size_sample),
    so 1600 of them lie in the corner the hot pass writes, 840 in each rectangle, the rest on the pose rows and columns and
    in the untouched corner -- are held to the componentwise bound against long double (gamma_3 on the cross entries),
    and the untouched corner keeps its bits on a seeded sample.
    Printed: join_map's HIP-event time (median of 5 after 1), its rate on the declared bytes 16 (Nb - 3)^2 + 32 b (Na - 3) as a
    fraction of 8 TB/s, reframe(FIXED) at live = 10003 and correct_sparse(2, 5) in the same process, and the wall clock of
    the host route (get_sigma of both, numpy, set) measured in this run.  Asserted: join_map takes less than that host route.
    Measured on an MI355X: profiles/r28/dense64_join_bench.txt."""
    N, Na, Nb = 10003, 8003, 2003
    rng = np.random.default_rng(8)
    raw = _full_size_sigma(N, rng)
    SB = _full_size_sigma(Nb, rng)
    xa = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-7.0, 7.0, size=N - 3)])
    xb = np.concatenate([[0.2, 0.5, -0.4], rng.uniform(-7.0, 7.0, size=Nb - 3)])
    d, s = hip.DensePropagator64(N), hip.DensePropagator64(Nb)
    d.set(Sigma=raw)
    d.state = xa
    d.live = Na
    s.set(Sigma=SB)
    s.state = xb
    Tr, Tc = _tiles(hip)
    G, E, _ = d.join_map(s, want_terms=True)
    assert d.live == N and jn.row_scale_err(E, jn.join_terms(xa[:Na], xb)[1]) <= FP64_TOL
    rows, cols = _full_size_sample(rng, N, Na, Tr, Tc), _full_size_sample(rng, N, Na, Tr, Tc)
    got = np.vstack([d.sigma_block(rows[lo:lo + 8], cols) for lo in range(0, 64, 8)])
    rr, cc = np.repeat(rows, 64), np.tile(cols, 64)
    ratio = jn.sampled_bound_ratio(got.reshape(-1), raw, Na, SB, Nb, G, E, rr, cc)
    assert ratio <= 1.0, ratio
    in_b = int(np.sum(rows >= Na)) * int(np.sum(cols >= Na))     # samples the hot pass wrote
    mid = np.array(sorted({3, 4, Na - 2, Na - 1} | {int(v) for v in rng.integers(3, Na, size=60)}))
    assert jn.same_bits(d.sigma_block(mid[:32], mid), raw[np.ix_(mid[:32], mid)])       # the untouched corner

    def join_again():
        d.live = Na
        return d.join_map(s)

    t_join = _median(join_again, iters=5, warmup=1)
    t_reframe = _median(lambda: d.reframe(0, 0.1, 1.0, 2.0), iters=5, warmup=1)
    cs, Hc, R, nu = np.array([0, 1, 2, 3 + 2 * 3333, 4 + 2 * 3333]), rng.standard_normal((2, 5)), np.eye(2), np.zeros(2)
    d.set(Sigma=raw)
    t_corr = _median(lambda: d.correct_sparse(cs, Hc, R, nu)[-1], iters=5, warmup=1)
    d.set(Sigma=raw)
    d.live = Na
    t_host = _host_route(d, s, Na, Nb, G, E)
    d.close(); s.close()
    b = (Nb - 3) // 2
    declared = 16.0 * (Nb - 3) ** 2 + 32.0 * b * (Na - 3)
    rate = declared / (t_join * 1e-3) / 1e12
    lines = [f"N={N} Na={Na} Nb={Nb}: join_map {t_join:.4f} ms, {declared / 1e6:.1f} MB declared, {rate:.2f} TB/s = "
             f"{rate / 8.0:.3f} of 8 TB/s; reframe(FIXED) at live={N} {t_reframe:.4f} ms; correct_sparse(2, 5) {t_corr:.4f} ms",
             f"N={N}: the host route (get_sigma of both, numpy, set) {t_host:.1f} ms wall clock = {t_host / t_join:.0f} x "
             f"join_map (asserted > 1); 64 x 64 sampled entries ({in_b} of them in the corner the "
             f"hot pass wrote, gamma_3 on the cross entries): max |err| / bound = {ratio:.4f}"]
    lines += [_NOTES[k] for k in sorted(_NOTES, key=str)]
    print("\n".join(lines))
    assert t_join < t_host, (t_join, t_host)
