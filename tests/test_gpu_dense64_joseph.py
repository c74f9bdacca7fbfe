"""-m gpu: ekf_dense64_correct_sparse_joseph (ekf_dense64_joseph.hip) against the model of dense_joseph_cases.py.
Integer families bit for bit (and equal to correct_sparse on a twin handle); slam_like against the long-double Joseph
expression; weights: the model, the bits of the considered entries and states, the tile count; the committed ill-conditioned
family (factor() says no after correct_sparse and yes after the Joseph call); pending rows; the singular S; the refusals; the
front ends with the flag; and N = 10003 timed against correct_sparse in the same process.

Seen on the MI355X: against the long-double expression <= 1.1e-15 on every shape (bound 1e-12); the ill-conditioned family:
pivot -0.20 at column 8 after correct_sparse, least pivot 0.34 after the Joseph call; N = 10003, m = 2, s = 5: correct_sparse
0.338 ms, the Joseph call 0.343 ms (1.01 x), 0.129 ms with one eighth of the states active and 37743 tiles skipped
(profiles/r25/dense64_joseph_bench.txt, which the full-size test rewrites)."""
import os

import numpy as np
import pytest

import dense_joseph_cases as jc
import dense_model_cases as mc
from parity import FP64_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 5


def _handle(hip, N, Sigma, x, Na=None):
    d = hip.DensePropagator64(N)
    d.set(F=np.eye(N), Q=np.zeros((N, N)), Sigma=Sigma)
    d.state = x
    if Na is not None and Na < N:
        d.live = Na
    return d


def _poisoned(c, N, Na):
    """the case on an N x N handle whose tail (rows and columns >= Na, states >= Na) is NaN"""
    Sigma, x = c["Sigma"].copy(), c["x"].copy()
    Sigma[Na:, :], Sigma[:, Na:], x[Na:] = np.nan, np.nan, np.nan
    return Sigma, x


def _layouts():
    return [(Na, Na) for Na in jc.SIZES] + [(Na + TAIL, Na) for Na in (5, 129)]


@pytest.mark.parametrize("N,Na", _layouts())
def test_integer_families_bit_for_bit(hip, N, Na):
    for m, s, order in jc.shapes(Na):
        c = jc.integer_case(N, m, s, order, 7000 + 31 * Na + 7 * m + s, Na)
        Sigma, x = _poisoned(c, N, Na)
        d, twin = _handle(hip, N, Sigma, x, Na), _handle(hip, N, Sigma, x, Na)
        nis, skipped, _ = d.correct_sparse_joseph(c["cols"], c["Hc"], c["R"], c["nu"])
        tnis, _ = twin.correct_sparse(c["cols"], c["Hc"], c["R"], c["nu"])
        wx, wS, wn = jc.np_joseph(x, Sigma, c["cols"], c["Hc"], c["R"], c["nu"], None, Na)
        got, gx = d.sigma, d.state
        what = f"N={N} Na={Na} m={m} s={s} {order}"
        assert jc.same_bits(got, wS) and jc.same_bits(gx, wx), what            # the model, the poisoned tail included
        assert jc.same_bits(got, twin.sigma) and jc.same_bits(gx, twin.state), what
        assert jc.same_bits(nis, tnis) and nis == wn and skipped == 0, what
        d.close(), twin.close()


@pytest.mark.parametrize("N,Na", _layouts())
def test_slam_like_against_the_long_double_joseph_expression(hip, N, Na):
    for m, s, order in jc.shapes(Na):
        c = jc.slam_case(N, m, s, order, 300 + m + s, Na)
        Sigma, x = _poisoned(c, N, Na)
        want = jc.joseph_longdouble(c["Sigma"][:Na, :Na], c["cols"], c["Hc"], c["R"])
        runs = []
        for _ in range(2):
            d = _handle(hip, N, Sigma, x, Na)
            d.correct_sparse_joseph(c["cols"], c["Hc"], c["R"], c["nu"])
            runs.append((d.sigma, d.state))
            d.close()
        err = jc.rel_cov_error(runs[0][0][:Na, :Na], want, c["Sigma"][:Na, :Na])
        print(f"N={N} Na={Na} m={m} s={s}: {err:.2e}")
        assert err <= jc.TOL, (N, Na, m, s, err)
        assert jc.same_bits(runs[0][0], runs[1][0]) and jc.same_bits(runs[0][1], runs[1][1])
        wx = jc.np_joseph(x, Sigma, c["cols"], c["Hc"], c["R"], c["nu"], None, Na)[0]
        assert np.abs(runs[0][1][:Na] - wx[:Na]).max() <= jc.TOL * max(1.0, np.abs(wx[:Na]).max())


def _plant(Sigma, x, w, Na):
    """distinct NaN payloads and -0.0 where row and column are both considered; a NaN payload in the considered states"""
    off = np.nonzero(w[:Na] == 0.0)[0]
    k = 0
    for i in off:
        for j in off:
            Sigma[i, j] = -0.0 if (i + j) % 3 == 0 else np.array([0x7FF8000000000000 + 0x1000 + k], dtype=np.uint64).view(np.float64)[0]
            k += 1
    for i in off[::2]:
        x[i] = np.array([0x7FF8000000000000 + 0x77000 + i], dtype=np.uint64).view(np.float64)[0]
    return off


@pytest.mark.parametrize("kind", jc.WEIGHT_KINDS)
@pytest.mark.parametrize("N,Na", [(5, 5), (129, 129), (300, 300), (305, 300)])
def test_weights(hip, N, Na, kind):
    d0 = hip.DensePropagator64(8)
    info = d0.joseph_launch_info()
    d0.close()
    assert info == {"tile_rows": 16, "tile_cols": 128, "threads": 256}
    pool = jc.active_prefix(kind, Na, info["tile_cols"])
    for m, s, order in [t for t in jc.shapes(Na) if t[:2] in ((2, 5), (3, 64), (32, 5), (1, 1), (3, 5)) and t[1] <= pool]:
        w = jc.weights(kind, N, Na, 50 + Na + m, info["tile_cols"])
        w[Na:] = 0.25                                                         # (ignored by the call; the wrapper wants them in range)
        exact = kind != "random"
        c = (jc.integer_case if exact else jc.slam_case)(N, m, s, order, 900 + Na + m + s, Na, pool)
        # the listed states stay active, so that no planted NaN is gathered into T or U
        w[c["cols"]] = np.where(w[c["cols"]] == 0.0, 1.0, w[c["cols"]])
        Sigma, x = _poisoned(c, N, Na)
        off = _plant(Sigma, x, w, Na)
        d = _handle(hip, N, Sigma, x, Na)
        nis, skipped, _ = d.correct_sparse_joseph(c["cols"], c["Hc"], c["R"], c["nu"], w)
        got, gx = d.sigma, d.state
        d.close()
        what = f"{kind} N={N} Na={Na} m={m} s={s}"
        assert skipped == jc.tiles_skipped(Na, w, info["tile_rows"], info["tile_cols"]), what
        if kind == "tiles" and Na > info["tile_cols"]:
            assert skipped > 0, what
        assert jc.same_bits(got[np.ix_(off, off)], Sigma[np.ix_(off, off)]), what        # NaN payloads and -0.0 survive
        assert jc.same_bits(gx[off], x[off]) and jc.same_bits(got[Na:], Sigma[Na:]) and jc.same_bits(got[:, Na:], Sigma[:, Na:]), what
        wx, wS, wn = jc.np_joseph(x, Sigma, c["cols"], c["Hc"], c["R"], c["nu"], w, Na)
        on = np.setdiff1d(np.arange(Na), off)
        if exact:
            assert jc.same_bits(got, wS) and jc.same_bits(gx, wx) and nis == wn, what
        else:
            clean = c["Sigma"][:Na, :Na]
            want = np.asarray(jc.joseph_longdouble(clean, c["cols"], c["Hc"], c["R"], w[:Na]), dtype=np.float64)
            keep = np.ones((Na, Na), dtype=bool)
            keep[np.ix_(off, off)] = False
            err = jc.rel_cov_error(np.where(keep, got[:Na, :Na], 0.0), np.where(keep, want, 0.0), clean)
            assert err <= jc.TOL, (what, err)
            assert np.abs(gx[on] - wx[on]).max() <= jc.TOL * max(1.0, np.abs(wx[on]).max()), what


def test_null_weights_skip_nothing_and_equal_all_ones(hip):
    N = 300
    c = jc.slam_case(N, 2, 5, "asc", 11)
    a, b = _handle(hip, N, c["Sigma"], c["x"]), _handle(hip, N, c["Sigma"], c["x"])
    _, s0, _ = a.correct_sparse_joseph(c["cols"], c["Hc"], c["R"], c["nu"])
    _, s1, _ = b.correct_sparse_joseph(c["cols"], c["Hc"], c["R"], c["nu"], np.ones(N))
    assert s0 == 0 and s1 == 0 and jc.same_bits(a.sigma, b.sigma) and jc.same_bits(a.state, b.state)
    a.close(), b.close()


def test_definiteness_on_the_ill_conditioned_family(hip):
    c = jc.ill_case()
    Na = jc.ILL["Na"]
    d = _handle(hip, Na, c["Sigma"], c["x"])
    assert d.factor()["ok"] == 1
    d.correct_sparse(c["cols"], c["Hc"], c["R"], c["nu"])
    short = d.factor()
    d.set(Sigma=c["Sigma"])
    d.state = c["x"]
    d.correct_sparse_joseph(c["cols"], c["Hc"], c["R"], c["nu"])
    jos = d.factor()
    d.close()
    print("short form:", short, "\nJoseph form:", jos)
    assert short["ok"] == 0 and jos["ok"] == 1


@pytest.mark.parametrize("rows", [2, 64])
def test_pending_rows_are_flushed_first(hip, rows):
    N = 129
    base = jc.slam_case(N, 2, 5, "asc", 21)
    a, b = _handle(hip, N, base["Sigma"], base["x"]), _handle(hip, N, base["Sigma"], base["x"])
    for d in (a, b):
        for k in range(rows // 2):
            p = jc.slam_case(N, 2, 5, "scattered", 400 + k)
            d.correct_sparse_deferred(p["cols"], p["Hc"], p["R"], p["nu"])
        assert d.pending == rows
    b.flush()
    c = jc.slam_case(N, 3, 64, "scattered", 22)
    w = jc.weights("range", N, N, 3)
    ra = a.correct_sparse_joseph(c["cols"], c["Hc"], c["R"], c["nu"], w)
    rb = b.correct_sparse_joseph(c["cols"], c["Hc"], c["R"], c["nu"], w)
    assert a.pending == 0 and jc.same_bits(a.sigma, b.sigma) and jc.same_bits(a.state, b.state) and ra[:2] == rb[:2]
    a.close(), b.close()


def test_singular_S_leaves_everything(hip):
    N = 129
    c = jc.integer_case(N, 2, 5, "asc", 5)
    Hc = np.tile(np.array([[1.0, 2.0, 3.0, 1.0, 2.0]]), (2, 1))               # a repeated row, R = 0: S is exactly singular
    d = _handle(hip, N, c["Sigma"], c["x"])
    with pytest.raises(hip.EkfError) as e:
        d.correct_sparse_joseph(c["cols"], Hc, np.zeros((2, 2)), c["nu"], jc.weights("scattered", N, N, 1))
    assert e.value.status == 5
    assert jc.same_bits(d.sigma, c["Sigma"]) and jc.same_bits(d.state, c["x"])
    d.close()


def test_refusals_leave_the_pending_rows(hip):
    import ctypes
    N = 64
    c = jc.slam_case(N, 2, 5, "asc", 31)
    d = _handle(hip, N, c["Sigma"], c["x"])
    d.correct_sparse_deferred(c["cols"], c["Hc"], c["R"], c["nu"])
    lib, ip = hip.load(), c["cols"].ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    def call(m, Hc, w):
        return lib.ekf_dense64_correct_sparse_joseph(d._h, m, 5, ip, hip._d(Hc) if Hc is not None else None, hip._d(c["R"]),
                                                     None, hip._d(w) if w is not None else None, None, None, None)
    w = np.ones(N)
    bad = [(33, np.ones((33, 5)), w), (2, None, w)]
    for v in (np.nan, -0.5, 1.5):
        wb = w.copy()
        wb[N - 1] = v
        bad.append((2, c["Hc"], wb))
    for m, Hc, wv in bad:
        assert call(m, Hc, wv) == 1 and d.pending == 2
    d.close()


def test_front_ends_with_the_flag(hip):
    n, ticks = 6, 20
    pairs = []
    for joseph in (False, True):
        f = hip.DenseEKFSLAM(n, joseph=joseph)
        log = []
        for dth, dx, z, vis in mc.slam_scenario(n, ticks):
            f.prediction(dth, dx)
            log.append(f.measurement(z, vis))
        pairs.append((f.state, f.handle.sigma, log))
        f.close()
    (x0, S0, l0), (x1, S1, l1) = pairs
    assert l0 == l1
    assert np.abs(x0 - x1).max() <= FP64_TOL * max(1.0, np.abs(x0).max())
    assert np.abs(S0 - S1).max() <= FP64_TOL * np.abs(S0).max()
    pairs = []
    for joseph in (False, True):
        f = hip.DenseEKFSLAM(n, joseph=joseph)
        log = []
        for dth, dx, readings in mc.discovery_scenario(n, ticks):
            f.prediction(dth, dx)
            log.append(tuple(f.data_association(readings)))
        pairs.append((f.state, f.handle.sigma, log, f.known))
        f.close()
    (x0, S0, l0, k0), (x1, S1, l1, k1) = pairs
    assert l0 == l1 and k0 == k1                                              # identical decisions
    assert np.abs(x0 - x1).max() <= FP64_TOL * max(1.0, np.abs(x0).max())
    assert np.abs(S0 - S1).max() <= FP64_TOL * np.abs(S0).max()
    with pytest.raises(ValueError):
        hip.DenseEKFSLAM(n, deferred=True, joseph=True)
    d = hip.DensePropagator64(3 + 2 * n)
    import ctypes
    k, done = ctypes.c_int(0), ctypes.c_int(0)
    z, vis, flag = np.zeros((n, 2)), np.ones(n, dtype=np.uint8), ctypes.c_int(1)
    assert hip.load().ekf_dense64_measure_landmarks(d._h, None, n, hip._d(z), vis.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                                    ctypes.byref(flag), 1 | jc.LM_JOSEPH, ctypes.byref(done), None, None, None) == 1
    assert hip.load().ekf_dense64_associate_landmarks(d._h, None, 1, hip._d(z), n, ctypes.byref(k), 1 | jc.LM_JOSEPH, None, None, None) == 1
    d.close()


def _median(f, iters=9, warmup=2):
    for _ in range(warmup):
        f()
    return float(np.median([f() for _ in range(iters)]))


def test_full_size_n10003_and_time(hip):
    """both calls move 16 N^2 bytes; the Joseph call carries twice the rank and one more small launch.  Guard: at most 2 x
    correct_sparse(2, 5); with one eighth of the states active it must beat the call with gain_w = NULL."""
    N, n_active = 10003, 1251
    rng = np.random.default_rng(10003)
    B = rng.standard_normal((N, 4))
    Sigma = B @ B.T / 4 + np.diag(rng.uniform(0.5, 1.0, size=N))
    c = jc.slam_case(16, 2, 5, "asc", 1)
    cols = np.array([0, 1, 2, 3 + 2 * 40, 4 + 2 * 40], dtype=np.int32)
    w = np.ones(N)
    w[n_active:] = 0.0
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)

    def timed(call):                                                          # each variant starts from the restored Sigma
        d.set(Sigma=Sigma)
        return _median(lambda: call()[-1])
    t_short = timed(lambda: d.correct_sparse(cols, c["Hc"], c["R"], c["nu"]))
    t_jos = timed(lambda: d.correct_sparse_joseph(cols, c["Hc"], c["R"], c["nu"]))
    t_part = timed(lambda: d.correct_sparse_joseph(cols, c["Hc"], c["R"], c["nu"], w))
    d.set(Sigma=Sigma)
    _, skipped, _ = d.correct_sparse_joseph(cols, c["Hc"], c["R"], c["nu"], w)
    got = d.sigma
    d.close()
    info = {"tile_rows": 16, "tile_cols": 128}
    assert skipped == jc.tiles_skipped(N, w, info["tile_rows"], info["tile_cols"]) > 0
    assert jc.same_bits(got[n_active:, n_active:], Sigma[n_active:, n_active:])
    lines = [f"N = {N}, m = 2, s = 5, medians of 9 after 2, HIP events",
             f"correct_sparse                  {t_short:.4f} ms",
             f"correct_sparse_joseph           {t_jos:.4f} ms  ({t_jos / t_short:.2f} x)",
             f"correct_sparse_joseph, w = 0 on states >= {n_active}  {t_part:.4f} ms, tiles_skipped {skipped}"]
    print("\n".join(lines))
    out = os.path.join(ROOT, "profiles", "r25")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "dense64_joseph_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    assert t_jos <= 2.0 * t_short, (t_jos, t_short)
    assert t_part < t_jos, (t_part, t_jos)
