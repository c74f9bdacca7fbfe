"""-m gpu: ekf_dense64_extract_map (ekf_dense64_extract.hip) against the model of dense_extract_cases.  The source's live
dimension runs over the odd numbers nearest {3, 5, 7, T - 1, T, T + 1, 2 T + 1, 3 T + 2} for both tile sides the library
reports, the keep list over every family; the source is created with N = Nb and Nb + 5, the destination with N = Nd and
Nd + 5, and everything outside both live corners is poisoned with payload NaNs.  1. a pure copy, bit for bit; 2. the source
is untouched; 3. pending rows are carried, a destination's own rows and open regions go first; 4. a clone is the same filter;
5. refusals; 6. DenseEKFSLAM clone / restore / submap / join."""
import numpy as np
import pytest

import dense_extract_cases as ex
import dense_model_cases as dm
from parity import FP64_TOL, worst
from dense_frame_cases import slam_like, slam_state
from test_gpu_dense64_live import _poison

pytestmark = pytest.mark.gpu
_TILES = []
N_SIZES = len(ex.sizes(64, 128))   # the number of distinct sizes does not depend on the tile sides as long as they differ


def _tiles(hip):
    if not _TILES:
        d = hip.DensePropagator64(3)
        info = d.extract_launch_info()
        d.close()
        assert info["threads"] == 256 and info["tile_rows"] % 2 == 0 and info["tile_cols"] % info["tile_rows"] == 0
        _TILES.extend([info["tile_rows"], info["tile_cols"]])
    return _TILES


def _handle(hip, corner, x, N):
    """a handle of dimension N whose live corner holds `corner` and x; everything else is poison"""
    n = corner.shape[0]
    S, xs = _poison(N, n, corner, x)
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = xs
    d.live = n
    return d, S, xs


def _blank(hip, N):
    """a destination of dimension N that holds nothing but poison (of the other sign), live = N"""
    S, xs = _poison(N, 0, np.zeros((0, 0)), np.zeros(0))
    d = hip.DensePropagator64(N)
    d.set(Sigma=-S)
    d.state = -xs
    return d, -S, -xs


def _padded_want(d, S, xs):
    """what get_padded shows of a handle that holds S and xs: zero beyond N"""
    ld = d.launch_info()["ld"]
    P, p = np.zeros((ld, ld)), np.zeros(ld)
    P[:d.N, :d.N], p[:d.N] = S, xs
    return P, p


def _same_padded(got, want):
    return ex.same_bits(got[0], want[0]) and ex.same_bits(got[1], want[1])


# ---- 1. a pure copy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(N_SIZES))
def test_extract_is_a_pure_copy_bit_for_bit(hip, k):
    """every family of keep lists; the same bits from both N of the source and both N of the destination; the poison outside
    both corners (and the zero padding beyond N) where it was; the source as it was; the transposed gather does not match"""
    Tr, Tc = _tiles(hip)
    Nb = ex.sizes(Tr, Tc)[k]
    b = (Nb - 3) // 2
    corner, x = ex.source_corner(Nb), ex.source_state(Nb)
    fams = ex.families(b, Tr // 2, Tc // 2)
    for tail_s in (0, 5):
        s, S, xs = _handle(hip, corner, x, Nb + tail_s)
        before = s.padded()
        assert _same_padded(before, _padded_want(s, S, xs))
        for name, keep in sorted(fams.items()):
            lst = ex.as_list(keep, b)
            Nd = 3 + 2 * lst.size
            want_c, want_x = ex.expected_corner(corner, lst), ex.expected_state(x, lst)
            for tail_d in (0, 5):
                d, D, dx = _blank(hip, Nd + tail_d)
                ms = d.extract_map(s, keep)
                what = f"Nb={Nb} {name} tails=({tail_d}, {tail_s})"
                assert ms >= 0.0 and d.live == Nd and d.pending == 0, what
                D[:Nd, :Nd], dx[:Nd] = want_c, want_x
                got, want = d.padded(), _padded_want(d, D, dx)
                d.close()
                assert ex.same_bits(got[0][:Nd, :Nd], want_c), what
                assert _same_padded(got, want), what + ": the destination outside its corner, or its state"
                assert not ex.same_bits(got[0][:Nd, :Nd], ex.transposed_corner(corner, lst)), what
            assert s.live == Nb and s.pending == 0
        assert _same_padded(s.padded(), before), f"Nb={Nb} tail={tail_s}: the source"
        s.close()


def test_a_run_repeats_and_a_list_equals_null_for_the_identity(hip):
    Tr, Tc = _tiles(hip)
    Nb = ex.odd_near(3 * Tc + 2)
    b = (Nb - 3) // 2
    corner, x = ex.source_corner(Nb), ex.source_state(Nb)
    s, _, _ = _handle(hip, corner, x, Nb + 5)
    outs = []
    for keep in (None, np.arange(b), None):
        for k_arg in ((-1, b) if keep is None else (b,)):
            d, _, _ = _blank(hip, Nb)
            if keep is None:                                             # the raw call: k = -1 and k = b both mean "all"
                assert hip.load().ekf_dense64_extract_map(d._h, s._h, k_arg, None, None) == 0
            else:
                d.extract_map(s, keep)
            outs.append(d.padded())
            d.close()
    s.close()
    assert all(_same_padded(o, outs[0]) for o in outs[1:]) and ex.same_bits(outs[0][0][:Nb, :Nb], corner)


def _raw(hip, d, s, keep):
    import ctypes
    arr = (ctypes.c_int * max(1, len(keep)))(*[int(v) for v in keep])
    return hip.load().ekf_dense64_extract_map(d._h, s._h, len(keep), arr, None)


# ---- 2. / 3. pending rows -----------------------------------------------------------------------------------------------------

def _float_source(hip, Nb, tail, seed=1):
    corner, x = slam_like(Nb, seed=seed), slam_state(Nb, seed=seed)
    return _handle(hip, corner, x, Nb + tail)


def _defer(h, n, rows, seed=17):
    """`rows` pending rows from correct_sparse_deferred on a map of n states: one row, or corrections of two"""
    rng = np.random.default_rng(seed)
    b = (n - 3) // 2
    if rows == 1:
        h.correct_sparse_deferred(np.array([0, 1, 2, 5, 6]), rng.standard_normal((1, 5)), 0.5 * np.eye(1), 0.1 * rng.standard_normal(1))
    for i in range(rows // 2):
        j = (7 * i + 1) % b
        h.correct_sparse_deferred(np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j]), rng.standard_normal((2, 5)), 0.5 * np.eye(2),
                                  0.1 * rng.standard_normal(2))
    assert h.pending == rows


def _read_through(d, idx):
    """Sigma_cur[idx, idx] by the block readout (under carry it reads through the pending rows and flushes nothing)"""
    idx = np.asarray(idx)
    step = max(1, 65536 // idx.size)
    return np.vstack([d.sigma_block(idx[lo:lo + step], idx) for lo in range(0, idx.size, step)])


@pytest.mark.parametrize("carry", [True, False])
@pytest.mark.parametrize("p", [1, 2, 64])
def test_pending_rows_are_carried_not_applied(hip, p, carry):
    """the source has p rows pending: afterwards the destination has the same p, the source still has its own, and nothing of
    the source has changed.  Under carry the destination's Sigma_cur is the source's at iota x iota bit for bit; after flush on
    both, the identity list (same N) gives the same bits and a subset list the same values to FP64_TOL."""
    Tr, Tc = _tiles(hip)
    Nb = ex.odd_near(Tc + Tr + 1)
    b = (Nb - 3) // 2
    fams = ex.families(b, Tr // 2, Tc // 2)
    for name in ("identity", "random", "two_runs_inside"):
        keep = fams[name]
        lst = ex.as_list(keep, b)
        io, Nd = ex.iota(lst), 3 + 2 * lst.size
        s, S, xs = _float_source(hip, Nb, 5)
        d, D, dx = _blank(hip, Nb + 5 if keep is None else Nd + 5)
        s.carry = d.carry = carry
        _defer(s, Nb, p)
        src_cur = _read_through(s, np.arange(Nb)) if carry else None
        src_state = s.state
        d.extract_map(s, keep)
        what = f"{name} p={p} carry={carry}"
        assert (d.pending, s.pending, d.live, s.live, d.carry, s.carry) == (p, p, Nd, Nb, carry, carry), what
        assert ex.same_bits(s.state, src_state) and ex.same_bits(d.state[:Nd], src_state[io]) and ex.same_bits(d.state[Nd:], dx[Nd:])
        if carry:
            assert ex.same_bits(_read_through(d, np.arange(Nd)), src_cur[np.ix_(io, io)]), what
            assert ex.same_bits(_read_through(s, np.arange(Nb)), src_cur) and (d.pending, s.pending) == (p, p), what
        s.flush(); d.flush()
        assert (d.pending, s.pending) == (0, 0)
        got, src_after = d.padded(), s.padded()
        assert np.isfinite(src_after[0][:Nb, :Nb]).all() and not ex.same_bits(src_after[0][:Nb, :Nb], S[:Nb, :Nb]), what
        D[:Nd, :Nd], dx[:Nd] = got[0][:Nd, :Nd], src_after[1][io]
        S[:Nb, :Nb] = src_after[0][:Nb, :Nb]
        want_d, want_s = _padded_want(d, D, dx), _padded_want(s, S, src_state)   # (a correction moves the state at once)
        d.close(); s.close()
        assert _same_padded(got, want_d), what + ": the flush went beyond the extracted corner"
        assert _same_padded(src_after, want_s), what + ": the source's own flush"
        if carry:
            assert ex.same_bits(src_after[0][:Nb, :Nb], src_cur), what
        w, e = worst(got[1][:Nd], got[0][:Nd, :Nd], src_after[1][io], src_after[0][np.ix_(io, io)])
        assert w <= FP64_TOL, (what, e)
        if keep is None:
            assert ex.same_bits(got[0][:Nd, :Nd], src_after[0][:Nb, :Nb]), what


@pytest.mark.parametrize("carry", [True, False])
def test_the_destinations_own_pending_rows_are_applied_first(hip, carry):
    """the destination holds a map of its own with two rows pending at its full width (so its panels hold non-zeros beyond the
    extracted corner): extract equals flush-then-extract bit for bit, the carried rows included, and after a flush nothing
    beyond the corner has moved from what the destination's own flush left"""
    Tr, Tc = _tiles(hip)
    Nb = ex.odd_near(Tc + Tr + 1)
    b = (Nb - 3) // 2
    keep = ex.families(b, Tr // 2, Tc // 2)["every_second"]
    io, Nd = ex.iota(keep), 3 + 2 * keep.size
    runs = []
    for flush_first in (False, True):
        s, _, _ = _float_source(hip, Nb, 5)
        d, _, _ = _handle(hip, slam_like(Nb + 10, seed=2), slam_state(Nb + 10, seed=2), Nb + 10)
        s.carry = d.carry = carry
        _defer(d, Nb + 10, 2, seed=5)
        _defer(s, Nb, 4)
        if flush_first:
            d.flush()
        own = d.padded() if flush_first else None                        # (what the destination's own flush leaves)
        d.extract_map(s, keep)
        assert (d.pending, s.pending, d.live, s.live) == (4, 4, Nd, Nb)
        cur = _read_through(d, np.arange(Nd)) if carry else None
        d.flush()
        runs.append((d.padded(), cur, own))
        d.close(); s.close()
    (a, cur_a, _), (c, cur_c, own) = runs
    assert _same_padded(a, c)
    if carry:
        assert ex.same_bits(cur_a, cur_c)
    mask = np.ones_like(own[0], dtype=bool)
    mask[:Nd, :Nd] = False
    assert ex.same_bits(a[0][mask], own[0][mask]) and ex.same_bits(a[1][Nd:], own[1][Nd:])
    assert not ex.same_bits(a[0][:Nd, :Nd], own[0][:Nd, :Nd])


@pytest.mark.parametrize("side", ["dst", "src"])
def test_an_open_region_ends_first(hip, side):
    """a region open on the destination or on the source, with a correction absorbed and rows pending inside it: extract equals
    region_end-then-extract bit for bit on both handles, and the region is counted as ended by another call"""
    Tr, Tc = _tiles(hip)
    Nb, Nr = ex.odd_near(Tr + 1), 9
    rng = np.random.default_rng(23)
    Hc, nu = rng.standard_normal((2, 5)), 0.1 * rng.standard_normal(2)
    keep = np.array([3, 0, 7, 8, 9])
    runs = []
    for end_first in (False, True):
        s, _, _ = _float_source(hip, Nb, 5)
        d, _, _ = _handle(hip, slam_like(Nb, seed=2), slam_state(Nb, seed=2), Nb + 5)
        h = d if side == "dst" else s
        ended = h.region_info()["ended_by_other_call"]
        h.region_begin(Nr)
        h.correct_sparse(np.array([0, 1, 2, 5, 6]), Hc, 0.5 * np.eye(2), nu)
        h.correct_sparse_deferred(np.array([0, 1, 2, 7, 8]), Hc, 0.5 * np.eye(2), nu)
        if end_first:
            h.region_end()
        assert _raw(hip, d, s, keep) == 0                                # (the wrapper takes no list while the source is in a region)
        info = h.region_info()
        assert not info["active"] and info["ended_by_other_call"] == ended + (0 if end_first else 1)
        assert (d.pending, s.pending, d.live, s.live) == (0, 0, 13, Nb)
        runs.append((d.padded(), s.padded()))
        d.close(); s.close()
    assert _same_padded(runs[0][0], runs[1][0]) and _same_padded(runs[0][1], runs[1][1])
    io = ex.iota(keep)
    assert ex.same_bits(runs[0][0][0][:13, :13], runs[0][1][0][np.ix_(io, io)]) and ex.same_bits(runs[0][0][1][:13], runs[0][1][1][io])


# ---- 4. a clone is the same filter ----------------------------------------------------------------------------------------------

def test_a_clone_is_the_same_filter(hip):
    """a deferred, carrying filter is cloned in mid-discovery with rows pending; the same ticks -- prediction, association with
    matches and new landmarks, deferred corrections, a flush -- on both handles give the same decisions and the same bits"""
    steps = dm.discovery_scenario(n=6, ticks=25)
    f = hip.DenseEKFSLAM(8, grow_live=True, deferred=True, carry=True)
    g = hip.DenseEKFSLAM(8, grow_live=True, deferred=True, carry=True)
    for dth, dx, readings in steps[:8]:
        f.prediction(dth, dx)
        f.data_association(readings)
    a, c = f.handle, g.handle
    pending, known0 = a.pending, f.known
    assert pending > 0 and 0 < known0 < 6
    c.extract_map(a)
    assert (c.pending, c.live, a.pending, a.live) == (pending, a.live, pending, 3 + 2 * known0)
    known, matched, grew = [known0, known0], False, False
    for dth, dx, readings in steps[8:]:
        out = []
        for i, h in enumerate((a, c)):
            h.predict_landmarks(dth, dx)
            before = known[i]
            known[i], assoc, best, _ = h.associate_landmarks(readings, known[i], 8, deferred=True, grow_live=True)
            out.append((known[i], assoc, best))
            matched |= bool(np.any((assoc >= 0) & (assoc < before)))
            grew |= known[i] > before
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and ex.same_bits(out[0][2], out[1][2])
        assert a.pending == c.pending and a.live == c.live
    assert matched and grew and known[0] == 6
    rng = np.random.default_rng(3)
    Hc, nu = rng.standard_normal((2, 5)), 0.01 * rng.standard_normal(2)
    for h in (a, c):
        h.correct_sparse_deferred(np.array([0, 1, 2, 7, 8]), Hc, 0.5 * np.eye(2), nu)
        h.flush()
    pa, pc = a.padded(), c.padded()
    f.close(); g.close()
    assert np.isfinite(pa[0]).all() and _same_padded(pa, pc)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_come_in_order_and_change_nothing(hip):
    """one case per rule (3) .. (9) and the order between neighbours, on handles with rows pending, then on ones inside a
    region.  RULE (4), DIFFERENT DEVICES, NEEDS A SECOND GPU: on a machine with one device that case does not run."""
    Nb = 13
    b = (Nb - 3) // 2
    import ctypes
    pairs = []
    for _ in range(2):
        s, _, _ = _float_source(hip, Nb, 5)
        d, _, _ = _handle(hip, slam_like(Nb, seed=2), slam_state(Nb, seed=2), Nb + 5)
        _defer(s, Nb, 4)
        _defer(d, Nb, 2, seed=5)
        pairs.append((d, s))
    (d, s), (td, ts) = pairs
    small, _, _ = _handle(hip, slam_like(5), slam_state(5), 5)            # room for one landmark
    even, _, _ = _handle(hip, slam_like(13)[:12, :12], np.linspace(-1.0, 1.0, 12), 17)
    lib = hip.load()

    def ext(a, c, k, keep):
        arr = None if keep is None else (ctypes.c_int * max(1, len(keep)))(*keep)
        return lib.ekf_dense64_extract_map(a._h, c._h, k, arr, None)

    def refused(a, c, k, keep, words):
        assert ext(a, c, k, keep) == 1 and words in lib.ekf_last_error(), (k, keep, words, lib.ekf_last_error())

    refused(d, d, 2, [0, 1], b"same handle")                             # (3)
    if hip.device_count() > 1:                                           # (4)
        far = hip.DensePropagator64(Nb, 1)
        refused(d, far, 0, [], b"different devices")
        far.close()
    refused(d, even, 1, [0], b"3 + 2 b")                                  # (5)
    refused(d, even, -2, [0], b"3 + 2 b")                                 # (5) before (6)
    refused(d, s, -2, [0], b"k must be")                                  # (6)
    refused(d, s, -1, [0], b"k must be")
    refused(d, s, b + 1, None, b"k must be")
    refused(d, s, b - 1, None, b"k must be")
    refused(d, s, -3, [b], b"k must be")                                  # (6) before (7)
    refused(d, s, 2, [0, b], b"in [0, b)")                                # (7)
    refused(d, s, 1, [-1], b"in [0, b)")
    refused(d, s, 3, [1, 1, b], b"in [0, b)")                             # (7) before (8)
    refused(d, s, 2, [1, 1], b"twice")                                    # (8)
    refused(small, s, 2, [1, 1], b"twice")                                # (8) before (9)
    refused(small, s, 2, [0, 1], b"does not fit")                         # (9)
    refused(small, s, -1, None, b"does not fit")
    for a, c, keep in ((d, s, [0, 0]), (d, d, None), (s, object(), None), (d, s, [b]), (small, s, [0, 1]), (d, s, [[0]])):
        with pytest.raises(ValueError):                                   # the wrapper's own
            a.extract_map(c, keep)
    assert (d.pending, s.pending, d.live, s.live, small.live, even.live) == (2, 4, Nb, Nb, 5, 12)
    # an open region stays open through a refusal, on either side
    td.flush()
    td.region_begin(7)
    ended = td.region_info()["ended_by_other_call"]
    refused(td, td, 0, [], b"same handle")
    refused(td, even, 0, [], b"3 + 2 b")
    refused(td, ts, 2, [1, 1], b"twice")
    refused(small, td, 2, [0, 1], b"does not fit")
    refused(d, td, 1, [b], b"in [0, b)")
    info = td.region_info()
    assert info["active"] and info["ended_by_other_call"] == ended and td.live == 7 and ts.pending == 4
    d.flush()                                                             # (as its twin was, in front of the region)
    same = _same_padded(d.padded(), td.padded()) and _same_padded(s.padded(), ts.padded())
    for h in (d, s, td, ts, small, even):
        h.close()
    assert same


# ---- 6. DenseEKFSLAM --------------------------------------------------------------------------------------------------------------

def _run(f, steps):
    for dth, dx, readings in steps:
        f.prediction(dth, dx)
        f.data_association(readings)


@pytest.mark.parametrize("deferred", [False, True])
def test_slam_filter_clone_diverge_and_restore(hip, deferred):
    """snapshot, run the sequential rule on the filter and the joint rule on a second clone, restore: the filter is the
    snapshot again bit for bit, the known count and the pending rows included"""
    steps = dm.discovery_scenario(n=6, ticks=14)
    f = hip.DenseEKFSLAM(8, grow_live=True, deferred=deferred, carry=deferred)
    _run(f, steps[:10])
    snap = f.clone()
    assert isinstance(snap, hip.DenseEKFSLAM) and (snap.n, snap.handle.N, snap.deferred, snap.grow_live) == (8, 19, deferred, True)
    assert (snap.known, snap.init_flag, snap.handle.live, snap.handle.pending, snap.handle.carry) == \
           (f.known, f.init_flag, f.handle.live, f.handle.pending, deferred)
    assert (f.handle.pending > 0) == deferred
    alt = snap.clone()
    dth, dx, readings = steps[10]
    f.prediction(dth, dx); alt.prediction(dth, dx)
    seq, joint = f.data_association(readings), alt.joint_association(readings)
    assert seq.shape == joint.shape
    _run(f, steps[11:])
    pending = snap.handle.pending
    moved = f.state
    assert f.restore(snap) is f
    assert (f.known, f.handle.live, f.handle.pending, snap.handle.pending) == (snap.known, snap.handle.live, pending, pending)
    assert not ex.same_bits(moved, f.state)
    if deferred:                                                          # through the pending rows, nothing flushed
        idx = np.arange(f.handle.live)
        assert ex.same_bits(_read_through(f.handle, idx), _read_through(snap.handle, idx)) and f.handle.pending == pending
    live = f.handle.live                                                  # (the copy covers the live dimension)
    a, c = f.handle.padded(), snap.handle.padded()
    for h in (f, snap, alt):
        h.close()
    assert np.isfinite(a[0][:live, :live]).all() and ex.same_bits(a[0][:live, :live], c[0][:live, :live])
    assert ex.same_bits(a[1][:live], c[1][:live])


def test_slam_filter_submap_is_the_marginal_and_joins_back(hip):
    """submap() of a discovered map is the filter with the other landmarks' rows and columns deleted (modelled through
    get_sigma_block); a target that is not grow_live gets its live dimension back over the constructor's prior; a reused
    target whose tail is coupled is refused; join() of the submap into a fresh global filter gives the submap again"""
    steps = dm.discovery_scenario(n=6, ticks=25)
    f = hip.DenseEKFSLAM(8, grow_live=True)
    _run(f, steps)
    assert f.known == 6 and f.handle.live == 15
    keep = [4, 1, 3]
    io = ex.iota(keep)
    want_S, want_x = f.handle.sigma_block(io, io), f.handle.state_block(0, 15)[io]
    sub = f.submap(keep)
    assert (sub.known, sub.init_flag, sub.handle.live, sub.n, sub.handle.N, f.known, f.handle.live) == (3, False, 9, 8, 19, 6, 15)
    assert ex.same_bits(sub.handle.sigma_block(np.arange(9), np.arange(9)), want_S) and ex.same_bits(sub.handle.state_block(0, 9), want_x)
    assert np.isfinite(want_S).all() and want_S[3, 3] < 1.0               # (a landmark that was corrected, not the prior)
    # the global filter that is not grow_live: the live dimension goes back to 3 + 2 n, over the prior
    h = hip.DenseEKFSLAM(6)
    _run(h, steps)
    assert h.known == 6 and h.handle.live == 15
    io2 = ex.iota([2, 0])
    want2 = h.handle.sigma_block(io2, io2)
    sub2 = h.submap([2, 0])
    assert (sub2.known, sub2.handle.live) == (2, 15)
    got2 = sub2.handle.sigma[:15, :15]
    prior = np.zeros((15, 15))
    prior[:7, :7], prior[7:, 7:] = want2, hip.DenseEKFSLAM.PRIOR * np.eye(8)
    assert ex.same_bits(got2, prior)
    with pytest.raises(ValueError, match="coupled"):
        h.submap([1], into=sub2)                                          # sub2's second landmark is tied to its pose
    assert sub2.handle.live == 5 and ex.same_bits(sub2.handle.sigma[:5, :5], h.handle.sigma_block(ex.iota([1]), ex.iota([1])))
    # the inverse of the join: a fresh global filter at the origin takes the submap
    glob = hip.DenseEKFSLAM(8, grow_live=True)
    glob.join(sub)
    assert glob.known == 3 and glob.handle.live == 9
    w, e = worst(glob.handle.state_block(0, 9), glob.handle.sigma[:9, :9], want_x, want_S)
    assert w <= FP64_TOL, e
    for x in (f, sub, h, sub2, glob):
        x.close()
