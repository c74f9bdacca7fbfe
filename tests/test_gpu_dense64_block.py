"""-m gpu: the block-structured prediction of the fp64 dense handle (ekf_dense64_propagate_block, ekf_dense64_block.hip)
-- `sigma = At*sigma*At.t() + Q` (ekf_slam.cpp:101-102) for At = identity with an r x r Jacobian in [first, first + r)^2:
integer operands bit-exact, nothing outside the block's rows and columns written, random operands within 1e-12 per block
of numpy fp64 and of the dense ekf_dense64_propagate, the reference's own prediction() (live through oracle.RefEKF, and
replayed from tests/golden/dense_predict_ref.npz) within FP64_TOL, predict / score / correct cycles, position
independence and run-to-run determinism, N = 10003.

Worst values seen on the MI355X (printed by test_zz_report): random operands 5.6e-16 per region against numpy and 0 against
the dense propagate; the reference live, its fixture and the structured checker 0 (the same bits); 20 predict / score /
correct cycles 1.3e-15 per covariance block (state 3.5e-18), 0 against the dense cycle; N = 10003 random operands 0; the call
takes 6.5 / 9.1 / 38.6 us for r = 3 / 16 / 64 at N = 10003 against 584 us for correct(m = 2)."""
import os

import numpy as np
import pytest

import dense_block_cases as bc
import dense_correct_cases as dc
import dense_score_cases as ds
from parity import FP64_TOL, cov_err, state_err, worst
from test_gpu_dense64 import TOL   # what tests/test_gpu_dense64.py holds propagate to against numpy

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {}
R_GRID = (1, 2, 3, 5, 16, 17, 33, 63, 64)


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {v:.3e}")


def _firsts(N, r):
    mid = ((N - r) // 2) | 1                     # an odd middle offset
    return sorted({f for f in (0, 1, mid, N - r) if 0 <= f <= N - r})


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi, size=shape).astype(np.float64)


def _block_err(got, want, first, r):
    """worst relative error per region (rows, columns, corner, rest), each against its own max-abs"""
    b = np.zeros(len(want), dtype=bool)
    b[first:first + r] = True
    out = 0.0
    for rows, cols in ((b, ~b), (~b, b), (b, b), (~b, ~b)):
        w, g = want[np.ix_(rows, cols)], got[np.ix_(rows, cols)]
        if w.size:
            out = max(out, float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-3)))
    return out


# ---- 1. integers, bit-exact --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 3, 43, 127, 128, 129, 300, 403])
def test_block_integers_exact(hip, N):
    """every sum exact in fp64, so any order gives the same bits: pins rows vs columns (Sigma is unsymmetric), Fr vs Fr^T,
    the strip edges and the padding.  Each case is followed by one dense propagation with an integer F, whose result is
    again exact: anything written into the padding shows there."""
    rng = np.random.default_rng(900 + N)
    d = hip.DensePropagator64(N)
    G, GQ = _ints(rng, -2, 3, (N, N)), _ints(rng, -5, 6, (N, N))
    d.set(F=G, Q=GQ)
    count = 0
    for r in sorted({r for r in R_GRID if r <= N} | ({N} if N <= 64 else set())):   # r = N where N <= 64
        for first in _firsts(N, r):
            Sigma = _ints(rng, -3, 4, (N, N))
            Fr, Qr = _ints(rng, -2, 3, (r, r)), _ints(rng, -5, 6, (r, r))
            dx, x = _ints(rng, -4, 5, r), _ints(rng, -9, 10, N)
            wx, wS = bc.np_predict_literal(x, Sigma, first, Fr, Qr, dx)
            d.set(Sigma=Sigma)
            d.state = x
            d.propagate_block(first, Fr, Qr, dx)
            got = d.sigma
            bad = got != wS
            assert not bad.any(), f"r={r} first={first}: {bad.sum()} wrong elements, first at {np.argwhere(bad)[0]}"
            assert np.array_equal(d.state, wx), (r, first)
            d.propagate(1)
            assert np.array_equal(d.sigma, G @ wS @ G.T + GQ), (r, first)
            count += 1
    d.close()
    assert count >= 1


def test_block_whole_matrix_is_the_dense_product(hip):
    """r = N <= 64: the two entry points compute the same matrix product"""
    for N in (1, 3, 43, 64):
        rng = np.random.default_rng(70 + N)
        Sigma, Fr, Qr = _ints(rng, -3, 4, (N, N)), _ints(rng, -2, 3, (N, N)), _ints(rng, -5, 6, (N, N))
        d = hip.DensePropagator64(N)
        d.set(Sigma=Sigma)
        d.propagate_block(0, Fr, Qr)
        assert np.array_equal(d.sigma, Fr @ Sigma @ Fr.T + Qr), N
        S = bc.unsymmetric_cov(N, rng)
        F = np.eye(N) + rng.normal(size=(N, N)) / np.sqrt(N)
        Q = 1e-3 * rng.normal(size=(N, N))
        d.set(F=F, Sigma=S, Q=Q)
        d.propagate(1)
        dense = d.sigma
        d.set(Sigma=S)
        d.propagate_block(0, F, Q)
        e = _block_err(d.sigma, dense, 0, N)
        _note("whole_matrix_vs_dense", e)
        assert e <= TOL
        d.close()


# ---- 2. untouched means untouched -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,r,first", [(43, 3, 0), (300, 17, 131), (403, 64, 339), (129, 5, 63)])
def test_block_leaves_the_rest_alone(hip, N, r, first):
    rng = np.random.default_rng(N + r)
    S = bc.unsymmetric_cov(N, rng)
    x = rng.normal(size=N)
    Fr = np.eye(r) + 0.3 * rng.normal(size=(r, r))
    Qr = 1e-3 * rng.normal(size=(r, r))
    F0, Q0 = _ints(rng, -2, 3, (N, N)), _ints(rng, -5, 6, (N, N))
    outside = np.ones((N, N), dtype=bool)
    outside[first:first + r, :] = False
    outside[:, first:first + r] = False
    d = hip.DensePropagator64(N)
    d.set(F=F0, Sigma=S, Q=Q0)
    d.state = x
    d.propagate_block(first, Fr, Qr, rng.normal(size=r))
    got, gx = d.sigma, d.state
    assert np.array_equal(got[outside].view(np.uint64), S[outside].view(np.uint64))     # the same bits
    keep = np.ones(N, dtype=bool); keep[first:first + r] = False
    assert np.array_equal(gx[keep].view(np.uint64), x[keep].view(np.uint64))
    assert not np.array_equal(got[first:first + r], S[first:first + r])                 # (and the block did change)

    # one NaN planted outside the block's rows and columns is still the only NaN
    i, j = [int(v) for v in np.argwhere(outside)[len(np.argwhere(outside)) // 2]]
    Sn = S.copy(); Sn[i, j] = np.nan
    d.set(Sigma=Sn)
    d.propagate_block(first, Fr, Qr)
    nan = np.isnan(d.sigma)
    assert nan.sum() == 1 and nan[i, j]

    # Fr = I without Qr and dx: Sigma and the state equal as values
    d.set(Sigma=S)
    d.state = x
    d.propagate_block(first, np.eye(r))
    assert np.array_equal(d.sigma, S) and np.array_equal(d.state, x)

    # the F and Q given to set() are as they were
    Si = _ints(rng, -3, 4, (N, N))
    d.set(Sigma=Si)
    d.propagate(1)
    assert np.array_equal(d.sigma, F0 @ Si @ F0.T + Q0)
    d.close()


# ---- 3. random operands -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [43, 129, 403, 2003])
def test_block_random_operands(hip, N):
    rng = np.random.default_rng(N)
    d, d2 = hip.DensePropagator64(N), hip.DensePropagator64(N)
    big = N > 1000                                  # (a case there costs a second of numpy and a dense propagation)
    for r in ((3, 17, 64) if big else (1, 3, 5, 17, 33, 64)):
        if r > N:
            continue
        for first in (_firsts(N, r)[::2] + [N - r] if big else _firsts(N, r)):
            S = bc.unsymmetric_cov(N, rng)
            x = rng.normal(size=N)
            Fr = np.eye(r) + rng.normal(size=(r, r)) / np.sqrt(r)
            Qr = np.diag(rng.uniform(1e-4, 1e-2, size=r)) + 1e-4 * rng.normal(size=(r, r))
            dx = rng.normal(size=r)
            wx, wS = bc.np_predict_slices(x, S, first, Fr, Qr, dx)
            d.set(Sigma=S)
            d.state = x
            d.propagate_block(first, Fr, Qr, dx)
            got = d.sigma
            e = _block_err(got, wS, first, r)
            es = max(state_err(d.state, wx).values())
            F, Q = bc.embed(N, first, Fr, Qr)
            d2.set(F, S, Q)
            d2.propagate(1)
            e2 = _block_err(got, d2.sigma, first, r)
            _note("random_vs_numpy", e); _note("random_vs_dense_propagate", e2); _note("random_state", es)
            assert e <= TOL and e2 <= TOL and es <= TOL, (r, first, e, e2, es)
    d.close(); d2.close()


# ---- 4. the reference's prediction() ---------------------------------------------------------------------------------------------

def _gpu_predict(hip, N):
    d = hip.DensePropagator64(N)

    def predict(state, Sigma, first, Fr, Qr, dx):
        d.set(Sigma=Sigma)
        d.state = state
        d.propagate_block(first, Fr, Qr, dx)
        return d.state, d.sigma
    return d, predict


def _check_case(hip, case, key):
    d, predict = _gpu_predict(hip, len(case["state0"]))
    s, c = bc.replay_case(case, predict)
    d.close()
    w, e = worst(s, c, case["state1"], case["cov1"])
    _note(key, w)
    assert w <= FP64_TOL, e


@pytest.mark.parametrize("n", [20, 200])
@pytest.mark.parametrize("name,twists,off", bc.CASES)
def test_block_against_the_reference(hip, oracle, n, name, twists, off):
    """prediction() of the reference's own ekf_slam.cpp IS one block prediction with first = 0, r = 3"""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    _check_case(hip, bc.record_case(oracle.RefEKF, n, twists, n + off), f"reference_live_{name}")


@pytest.mark.parametrize("name", [c[0] for c in bc.CASES])
def test_block_reference_fixture_replayed(hip, name):
    """tests/golden/dense_predict_ref.npz: the same cases at n = 20 with the reference's recorded outputs -- never skips"""
    z = np.load(os.path.join(HERE, "golden", "dense_predict_ref.npz"))
    case = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    assert len(case["twists"]) == len(dict((c[0], c[1]) for c in bc.CASES)[name])
    _check_case(hip, case, f"reference_fixture_{name}")


def test_block_against_the_structured_checker(hip, oracle):
    n = 1000
    o = oracle.OracleEKF(n, oracle.STRUCTURED)
    N = o.N
    rng = np.random.default_rng(11)
    A = rng.normal(size=(N, 64))
    S0 = A @ A.T / 64 + np.eye(N)
    x0 = rng.normal(size=N)
    d = hip.DensePropagator64(N)
    for dth, dx in ((0.05, 0.02), (0.0, 0.07)):
        o.state, o.cov = x0, S0
        o.prediction(dth, dx)
        Fr, Qr, upd = bc.model_operands(x0, dth, dx)
        d.set(Sigma=S0)
        d.state = x0
        d.propagate_block(0, Fr, Qr, upd)
        w, e = worst(d.state, d.sigma, o.state, o.cov)
        _note("structured_checker", w)
        assert w <= FP64_TOL, e
    d.close()


# ---- 5. the cycle -----------------------------------------------------------------------------------------------------------------

def test_block_predict_score_correct_cycle(hip):
    """20 steps of propagate_block -> score -> correct at n = 200 with the reference's motion and measurement models,
    against numpy and against the same cycle with the dense propagate on a second handle"""
    n = 200
    N = 3 + 2 * n
    rng = np.random.default_rng(2024)
    world = rng.uniform(-2.0, 2.0, size=(n, 2))
    world[np.hypot(world[:, 0], world[:, 1]) < 0.3] += 0.6
    x = np.concatenate([[0.1, 0.0, 0.0], (world + rng.normal(0, 0.02, size=(n, 2))).reshape(-1)])
    A = rng.normal(size=(N, N))
    S = 0.01 * (A @ A.T / N + np.eye(N))
    d, d2 = hip.DensePropagator64(N), hip.DensePropagator64(N)
    for h in (d, d2):
        h.set(Sigma=S)
        h.state = x
    for it in range(20):
        dth, dxx = (0.0, 0.05) if it % 7 == 3 else (0.1 + 0.01 * it, 0.05)
        Fr, Qr, upd = bc.model_operands(x, dth, dxx)
        d.propagate_block(0, Fr, Qr, upd)
        F, Q = bc.embed(N, 0, Fr, Qr)
        d2.set(F=F, Q=Q)
        d2.propagate(1)
        x2 = d2.state; x2[:3] += upd; d2.state = x2
        x, S = bc.np_predict_slices(x, S, 0, Fr, Qr, upd)
        # a noisy sighting of landmark i, scored against eight candidates, then corrected with the right one
        i = int(rng.integers(0, n))
        th, px, py = x[:3]
        dxy = x[3 + 2 * i:5 + 2 * i] - [px, py] + rng.normal(0, 0.004, size=2)
        sx = np.cos(th) * dxy[0] + np.sin(th) * dxy[1]
        sy = -np.sin(th) * dxy[0] + np.cos(th) * dxy[1]
        cand = sorted({i} | set(int(v) for v in rng.integers(0, n, size=7)))
        terms = [dc.measurement_terms(x[:3], x, j, sx, sy) for j in cand]
        H, R, nu = np.stack([t[0] for t in terms]), terms[0][1], np.stack([t[2] for t in terms])
        _, wnis = ds.np_scores(S, H, R, nu)
        for h in (d, d2):
            nis, _, flags, _ = h.score(H, R, nu)
            assert not flags.any()
            assert np.abs(nis - wnis).max() <= FP64_TOL * np.abs(wnis).max()
        Hi, Ri, _, wrapped = terms[cand.index(i)]
        for h in (d, d2):
            h.correct(Hi, Ri, wrapped)
        x, S, _ = dc.np_correct(x, S, Hi, Ri, wrapped)
    ec, es = max(cov_err(d.sigma, S).values()), max(state_err(d.state, x).values())
    e2, es2 = max(cov_err(d.sigma, d2.sigma).values()), max(state_err(d.state, d2.state).values())
    _note("cycle_cov", ec); _note("cycle_state", es); _note("cycle_cov_vs_dense", e2); _note("cycle_state_vs_dense", es2)
    assert max(ec, es, e2, es2) <= FP64_TOL
    # the padding of Sigma is still zero: I Sigma I^T + 0 returns Sigma bit for bit
    before = d.sigma
    d.set(F=np.eye(N), Q=np.zeros((N, N)))
    d.propagate(1)
    assert np.array_equal(d.sigma, before)
    d.close(); d2.close()


# ---- 6. position independence and determinism -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [3, 17, 64])
def test_block_same_bits_wherever_it_sits(hip, r):
    """the same r x M row data, M x r column data and corner embedded at two `first` values and in two N: the block's
    rows and columns come out with the same bits; and the same call twice gives the same bits"""
    rng = np.random.default_rng(40 + r)
    M = 130                                        # the columns / rows outside the block that carry the data
    rowdat, coldat, corner = rng.normal(size=(r, M)), rng.normal(size=(M, r)), rng.normal(size=(r, r))
    Fr = np.eye(r) + rng.normal(size=(r, r)) / np.sqrt(r)
    Qr = 1e-3 * rng.normal(size=(r, r))
    outs = []
    for N, first in ((M + r, 0), (M + r, 37), (M + r, M), (300, 1), (300, 171)):
        other = np.ones(N, dtype=bool); other[first:first + r] = False
        idx = np.nonzero(other)[0][:M]             # where the data goes: the first M positions outside the block
        S = rng.normal(size=(N, N))
        b = np.arange(first, first + r)
        S[np.ix_(b, idx)] = rowdat
        S[np.ix_(idx, b)] = coldat
        S[np.ix_(b, b)] = corner
        d = hip.DensePropagator64(N)
        res = []
        for _ in range(2):
            d.set(Sigma=S)
            d.propagate_block(first, Fr, Qr)
            res.append(d.sigma)
        d.close()
        assert np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64))            # run to run
        g = res[0]
        outs.append((g[np.ix_(b, idx)].copy(), g[np.ix_(idx, b)].copy(), g[np.ix_(b, b)].copy()))
        e = _block_err(g, bc.np_predict_slices(np.zeros(N), S, first, Fr, Qr)[1], first, r)
        assert e <= TOL
    for o in outs[1:]:
        for a, b_ in zip(outs[0], o):
            assert np.array_equal(a.view(np.uint64), b_.view(np.uint64))


# ---- 7. N = 10003 ---------------------------------------------------------------------------------------------------------------------

def _host_apply(cur, x, first, Fr, Qr, dx):
    """the three slice updates on the block's rows and columns of `cur`, and the state, in place"""
    b = slice(first, first + len(Fr))
    rows, cols, corner = Fr @ cur[b, :], cur[:, b] @ Fr.T, (Fr @ cur[b, b]) @ Fr.T + Qr
    cur[b, :] = rows
    cur[:, b] = cols
    cur[b, b] = corner
    x[b] += dx


def test_block_full_size_n10003(hip):
    """Sigma goes up once and comes back once per kind of operand: the six calls (r = 3 and 64 at first = 0, an odd offset
    and N - r) follow each other on the device while numpy follows them on the block's rows and columns alone."""
    N = 10003
    rng = np.random.default_rng(8)
    d = hip.DensePropagator64(N)
    blocks = [(r, first) for r in (3, 64) for first in (0, 4321, N - r)]
    touched = np.zeros(N, dtype=bool)
    for r, first in blocks:
        touched[first:first + r] = True
    others = np.array(sorted(set([200, 5000, 9000] + list(rng.integers(0, N, size=12)))))
    others = others[~touched[others]]
    assert len(others) >= 8
    for exact in (True, False):
        if exact:
            S = rng.integers(-3, 4, size=(N, N)).astype(np.float64)
            x = _ints(rng, -9, 10, N)
        else:
            A = rng.standard_normal((N, 64))
            S = A @ A.T / 64 + np.eye(N)
            S += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))   # unsymmetric
            x = rng.standard_normal(N)
            del A
        d.set(Sigma=S)
        d.state = x
        cur, wx = S.copy(), x.copy()
        for r, first in blocks:
            if exact:
                Fr, Qr, dx = _ints(rng, -2, 3, (r, r)), _ints(rng, -5, 6, (r, r)), _ints(rng, -4, 5, r)
            else:
                Fr = np.eye(r) + rng.standard_normal((r, r)) / np.sqrt(r)
                Qr, dx = 1e-3 * rng.standard_normal((r, r)), rng.standard_normal(r)
            d.propagate_block(first, Fr, Qr, dx)
            _host_apply(cur, wx, first, Fr, Qr, dx)
        got, gx = d.sigma, d.state
        sub = np.ascontiguousarray(got[others][:, ~touched])
        assert np.array_equal(sub.view(np.uint64), np.ascontiguousarray(S[others][:, ~touched]).view(np.uint64))
        if exact:
            assert np.array_equal(gx, wx)
            bad = got != cur
            assert not bad.any(), f"{bad.sum()} wrong elements, first at {np.argwhere(bad)[0]}"
        else:
            for r, first in blocks:
                b = slice(first, first + r)
                e = max(np.abs(got[b, :] - cur[b, :]).max() / np.abs(cur[b, :]).max(),
                        np.abs(got[:, b] - cur[:, b]).max() / np.abs(cur[:, b]).max(),
                        np.abs(got[b, b] - cur[b, b]).max() / np.abs(cur[b, b]).max(),
                        np.abs(gx - wx).max() / np.abs(wx).max())
                _note(f"full_size_r{r}", e)
                assert e <= TOL, (r, first, e)
        del cur, got
    # 32 r N bytes against the 24 N^2 of a correction: at this N the call is below correct(m = 2) for every r
    H, R = rng.standard_normal((2, N)), 0.01 * np.eye(2)
    t_correct = []
    for _ in range(3):
        d.set(Sigma=S)
        t_correct.append(d.correct(H, R)[1])
    for r in (3, 16, 64):
        Fr = np.linalg.qr(rng.standard_normal((r, r)))[0]
        t_block = [d.propagate_block(4321, Fr, 1e-4 * np.eye(r)) for _ in range(7)][2:]
        print(f"N={N} r={r}: propagate_block median {np.median(t_block) * 1e3:.1f} us, correct(m=2) median "
              f"{np.median(t_correct) * 1e3:.1f} us")
        assert np.median(t_block) < np.median(t_correct), (r, t_block, t_correct)
    d.close()


def test_zz_report():
    for k in sorted(WORST):
        print(f"dense64 block worst {k}: {WORST[k]:.3e}")
    assert all(v <= FP64_TOL for v in WORST.values())
