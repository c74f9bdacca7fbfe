"""Writes tests/golden/dense_score_ref.npz: recorded data of the reference build's calculate_maha_dis at n = 20 -- state,
covariance, 8 readings and the 8 x 20 matrix of RefEKF.maha(...) -- for the never-skipping comparison of
tests/test_gpu_dense64_score.py and the numpy check of tests/test_dense64_score_host.py.
Needs oracle/_ref/libekf_slam_ref.so (built by __graft_entry__.build() where the reference sources are present).

    python tests/golden/make_dense_score_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import binding  # noqa: E402
import dense_score_cases as ds  # noqa: E402
from parity import FP64_TOL  # noqa: E402


def main():
    case = ds.record_scores(binding.RefEKF, 20, ds.SEEDS[20])
    worst = 0.0
    for k, (sx, sy) in enumerate(case["readings"]):
        assert ds.margins_hold(case["maha"][k]), f"reading {k}: pick another seed"
        H, R, nu = ds.candidate_terms(case["state"], sx, sy)
        nis = ds.np_scores(case["cov"], H, R, nu)[1]
        worst = max(worst, float(np.abs(nis / case["maha"][k] - 1.0).max()))
        print(k, ds.reference_rule(case["maha"][k]), f"min {case['maha'][k].min():.3e} max {case['maha'][k].max():.3e}")
    print(f"numpy vs calculate_maha_dis, worst relative {worst:.2e}")
    assert worst <= FP64_TOL
    path = os.path.join(HERE, "dense_score_ref.npz")
    np.savez(path, **{k: np.asarray(v) for k, v in case.items()})
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
