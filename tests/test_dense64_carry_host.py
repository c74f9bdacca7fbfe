"""No GPU: the numpy model of the carried representation of the dense fp64 handle (tests/dense_carry_cases.py) -- Sigma_base
and the two pending panels, mapped by propagate_block / init_block, read through by the block readout.  Every chain of the
grid that tests/test_gpu_dense64_carry.py compares the device against bit for bit is proven exact in float64 here: every
product the model forms (for Sigma_base, for each panel, for Sigma_cur, for the scores) has all its terms integers over one
power of two with the sum of their absolute values below 2^52, so any order of summation -- numpy's, the device's
sequential fma, the matrix cores' in the flush -- gives the same number.  The carried model then equals the flush-first
model exactly."""
import numpy as np
import pytest

import dense_carry_cases as cc
import dense_deferred_cases as dd


def test_exact_product_bounds():
    big = np.array([[2.0 ** 26, 1.0]])
    with pytest.raises(cc.Inexact):
        cc.exact_product(big, big.T)                                 # 2^52 + 1: the bound is passed
    with pytest.raises(cc.Inexact):
        cc.exact_product(np.array([[2.0 ** -3 + 2.0 ** -30]]), np.array([[2.0 ** -3 + 2.0 ** -30]]))   # 60 fractional bits
    assert cc.exact_product(np.array([[3.0, -0.5]]), np.array([[2.0], [4.0]]), np.array([[0.25]]))[0, 0] == 4.25
    assert cc.frac_bits(np.array([0.25, 3.0, -0.5])) == 2 and cc.frac_bits(np.zeros((0, 3))) == 0


def test_the_grid_is_covered():
    """every (r, placement, p, s) is run at every N that can hold it; at most a quarter of the cells is held by no N (a
    one-wide block cannot straddle column 64: 12 of 180), every N and every value of r, p and s is run somewhere"""
    run, cells, nowhere = cc.grid()
    assert len(nowhere) * 4 <= len(cells), (len(nowhere), len(cells))
    assert all(c[0] == 1 and c[1] == "straddle" for c in nowhere), nowhere
    for k, values in enumerate((cc.GRID_N, cc.GRID_R, cc.GRID_PLACE, cc.GRID_P, cc.GRID_S)):
        assert {g[k] for g in run} == set(values), k
    # the sizes at which the map's code can go wrong are all there with rows pending up to the capacity
    assert {(g[1], g[3]) for g in run} >= {(r, p) for r in cc.GRID_R for p in cc.GRID_P}
    assert {(g[1], g[4]) for g in run} >= {(r, s) for r in cc.GRID_R for s in cc.GRID_S}


@pytest.mark.parametrize("N", cc.GRID_N)
def test_carried_chains_are_exact_and_equal_the_flush_first_model(N):
    run, _, _ = cc.grid()
    mine = [g for g in run if g[0] == N]
    assert mine
    most = 0
    for g in mine:
        chain = cc.carry_chain(*g)                                   # raises Inexact when a value leaves the integers
        p_at_map = [op["check"]["pending"] for op in chain["ops"] if op["op"] != "correct"]
        assert p_at_map[0] == p_at_map[1] == g[3], g                 # p rows pending at the first map and at the init
        most = max(most, max(p_at_map))
        carried, Sc = cc.run_model(chain, carry=True)
        flushed, Sf = cc.run_model(chain, carry=False)
        assert np.array_equal(Sc, chain["Sigma"]) and np.array_equal(Sf, chain["Sigma"]), g
        for i, (op, a, b) in enumerate(zip(chain["ops"], carried, flushed)):
            ck = op["check"]
            assert a["pending"] == ck["pending"] and np.array_equal(a["state"], ck["state"]), (g, i)
            assert np.array_equal(a["block"], ck["block"]) and np.array_equal(a["S"], ck["S"]), (g, i)
            for key in ("nis0", "state", "S", "nis", "Sigma_cur", "block"):          # carried == flush-first, exactly
                assert np.array_equal(np.asarray(a[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64),
                                      equal_nan=True), (g, i, key)
            if op["op"] != "correct":
                assert b["pending"] == 0 and a["pending"] > 0, (g, i)               # the two really differ in form
    assert most >= max(g[3] for g in mine)


def test_the_model_without_carried_calls_is_the_deferred_model():
    """on a chain of dense_deferred_cases the guarded overrides change no number"""
    chain = dd.integer_chain(65, "scattered")
    a, b = cc.CarriedModel(chain["Sigma0"], chain["x0"]), dd.DeferredModel(chain["Sigma0"], chain["x0"])
    for st in chain["steps"]:
        na = a.correct_deferred(st["cols"][0], st["Hc"][0], st["R"][0], st["nu"][0])
        nb = b.correct_deferred(st["cols"][0], st["Hc"][0], st["R"][0], st["nu"][0])
        assert na == nb == st["nis0"] and np.array_equal(a.state, b.state) and np.array_equal(a.state, st["state"])
        assert np.array_equal(a.Kt, b.Kt) and np.array_equal(a.Tp, b.Tp)
    assert np.array_equal(a.sigma_cur, chain["steps"][-1]["Sigma"])
