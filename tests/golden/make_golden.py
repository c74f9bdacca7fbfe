"""Generates the committed golden vectors under tests/golden/ (run from the repo root:
`python tests/golden/make_golden.py`).

The fixtures are produced by the two independent CPU restatements under oracle/ (dense-literal C and NumPy), which
must agree to 1e-12 per block before anything is written -- and, where build() made oracle/_ref/libekf_slam_ref.so
(the reference's own rigid2d/src/ekf_slam.cpp compiled against the tests-only Armadillo subset tests/cpp/arma_double),
with the reference build too.  ref_edges.npz holds the hand-built edges of tests/ref_scenarios.py with the reference
build's outputs (it is only written when that build exists), so the GPU suite keeps a pin where oracle/_ref is absent.  Inputs come from ekf_slam_ml_amd/synth.py (deterministic) and are
stored next to the expected outputs so the fixtures stay valid even if the generator changes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ref_scenarios as rs  # noqa: E402

from ekf_slam_ml_amd import synth  # noqa: E402
from oracle import binding as ob  # noqa: E402
from oracle.np_restatement import NumpyEKF  # noqa: E402
from parity import worst  # noqa: E402

AGREE = 1e-12
# Decision margins ("fixtures need margins"): a fixture whose scores sit closer than this (relative)
# to the gates 10.0 / 1.0 of ekf_slam.cpp:293,330, or whose winner beats the runner-up by less (ekf_slam.cpp:305-309), is
# not written -- another summation order (the kernels', Armadillo's) could flip it.  Pick another seed instead.
MIN_MARGIN = 1e-6


def reference(n):
    """the reference build (None when oracle/_ref/libekf_slam_ref.so was not built)"""
    try:
        return ob.RefEKF(n)
    except FileNotFoundError:
        return None


def agree(o, p, what, r=None):
    w, e = worst(o.state, o.cov, p.state, p.sigma)
    assert w <= AGREE, f"{what}: C and NumPy restatements disagree: {e}"
    if r is not None:
        wr, er = worst(o.state, o.cov, r.state, r.cov)
        assert wr <= AGREE, f"{what}: C restatement and the reference build disagree: {er}"
        w = max(w, wr)
    return w


def known(name, cfg, checkpoints):
    log = synth.make_known_log(cfg)
    n, T = cfg.n, cfg.steps
    o, p, r = ob.OracleEKF(n, ob.DENSE), NumpyEKF(n), reference(n)
    cp_state = []
    for t in range(T):
        sensor, vis = log.expand_step(t)
        for f in (o, p, r):
            if f is not None:
                f.prediction(*log.twist[t, 0])
                f.measurement(sensor, vis)
        if t in checkpoints:
            cp_state.append(o.state.copy())
    w = agree(o, p, name, r)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), n=n, twist=log.twist[:, 0], lm_idx=log.lm_idx[:, 0],
                        z_xy=log.z_xy[:, 0], init_xy=log.init_xy[0], checkpoints=np.array(sorted(checkpoints)),
                        cp_state=np.array(cp_state), state=o.state, cov=o.cov)
    print(f"{name}: n={n} T={T} corrections={log.corrections} C-vs-NumPy {w:.2e}")


def unknown(name, cfg):
    log = synth.make_unknown_log(cfg)
    n, T = cfg.n, cfg.steps
    o, p, r = ob.OracleEKF(n, ob.DENSE), NumpyEKF(n), reference(n)
    ko, kp, kr = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    assoc = np.full((T, log.meas_xy.shape[2]), -2, dtype=np.int32)
    margins = ob.new_margins()
    for t in range(T):
        J = int(log.count[t, 0])
        m = log.meas_xy[t, 0, :J]
        o.prediction(*log.twist[t, 0]); p.prediction(*log.twist[t, 0])
        a = o.data_association(m, ko, margins)
        b = p.data_association(m, kp)
        assert np.array_equal(a, b) and np.array_equal(ko, kp), f"{name}: decisions differ at step {t}"
        if r is not None:
            r.prediction(*log.twist[t, 0])
            r.data_association(m, kr)
            assert np.array_equal(ko, kr), f"{name}: known lists differ from the reference build at step {t}"
        assoc[t, :J] = a
    w = agree(o, p, name, r)
    assert margins[:3].min() >= MIN_MARGIN, f"{name}: decision margins too thin {dict(zip(ob.MARGIN_KEYS, margins))}"
    np.savez_compressed(os.path.join(HERE, name + ".npz"), n=n, twist=log.twist[:, 0], count=log.count[:, 0],
                        meas_xy=log.meas_xy[:, 0], assoc=assoc, known=ko, state=o.state, cov=o.cov, margins=margins)
    print(f"{name}: n={n} T={T} known={int(ko.sum())} updates={(assoc >= 0).sum()} dropped={(assoc == -1).sum()} "
          f"C-vs-NumPy {w:.2e} margins {dict(zip(ob.MARGIN_KEYS, margins))}")


def maha(name):
    """calculate_maha_dis vectors on a mid-run snapshot (state, cov) of the known-association run."""
    g = np.load(os.path.join(HERE, "known_n20.npz"))
    n = int(g["n"])
    o, p = ob.OracleEKF(n, ob.DENSE), NumpyEKF(n)
    o.state, o.cov = g["state"], g["cov"]
    o.set_init_flag(1)
    p.state, p.sigma, p.landmark_init_flag = g["state"].copy(), g["cov"].copy(), True
    meas = np.array([[0.31, -0.12], [-0.4, 0.55], [0.05, 0.02], [1.2, -0.9]])
    scores = np.array([[o.maha(mx, my, i) for i in range(n)] for mx, my in meas])
    scores_np = np.array([[p.maha(mx, my, i) for i in range(n)] for mx, my in meas])
    assert np.abs(scores - scores_np).max() / np.abs(scores).max() < 1e-11
    r = reference(n)
    if r is not None:
        r.state, r.cov = g["state"], g["cov"]
        r.set_init_flag(1)
        scores_ref = np.array([[r.maha(mx, my, i) for i in range(n)] for mx, my in meas])
        assert np.abs(scores - scores_ref).max() / np.abs(scores).max() <= AGREE
    np.savez_compressed(os.path.join(HERE, name + ".npz"), n=n, state=g["state"], cov=g["cov"], meas=meas, scores=scores)
    print(f"{name}: {scores.shape} scores, range [{scores.min():.3g}, {scores.max():.3g}]")


def ref_edges(name):
    """the edges of tests/ref_scenarios.py as the reference build computes them; the restatements must agree"""
    if reference(1) is None:
        raise SystemExit(f"{name}: needs oracle/_ref/libekf_slam_ref.so (the reference build)")
    sc = rs.edge_scenarios()
    rec = rs.record(ob.RefEKF, sc)
    dense = rs.record(lambda n: ob.OracleEKF(n, ob.DENSE), sc)
    for k in sc:
        assert all(np.array_equal(dense[k][3][i], rec[k][3][i]) for i in rec[k][3]), f"{name}/{k}: known lists differ"
        w, e = worst(dense[k][2][-1], dense[k][4], rec[k][2][-1], rec[k][4])
        assert w <= AGREE, f"{name}/{k}: C restatement and the reference build disagree: {e}"
    rs.save(os.path.join(HERE, name + ".npz"), rec)
    print(f"{name}: {len(rec)} scenarios, {sum(len(v[1]) for v in rec.values())} calls")


if __name__ == "__main__":
    ob.build()
    only = set(sys.argv[1:])   # e.g. `make_golden.py unknown_n20`: rewrite that fixture alone
    if not only or "known_n20" in only:
        known("known_n20", synth.config1(steps=250), {0, 1, 10, 100, 249})
    if not only or "unknown_n20" in only:
        c = synth.config1(steps=200)
        c.seed = 77
        unknown("unknown_n20", c)
    if not only or "known_n200" in only:
        c2 = synth.config2(steps=12)
        known("known_n200", c2, {0, 5, 11})
    if not only or "maha_n20" in only:
        maha("maha_n20")
    if not only or "ref_edges" in only:
        ref_edges("ref_edges")
