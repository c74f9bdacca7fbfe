"""Writes tests/golden/dense_predict_ref.npz: inputs and recorded outputs of the reference build's prediction() at n = 20
(N = 43) from a random state and an unsymmetric covariance -- one call per branch of ekf_slam.cpp:79 and five calls in a
row -- for the never-skipping replay of tests/test_gpu_dense64_block.py.
Needs oracle/_ref/libekf_slam_ref.so (built by __graft_entry__.build() where the reference sources are present).

    python tests/golden/make_dense_predict_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import binding  # noqa: E402
import dense_block_cases as bc  # noqa: E402
from parity import FP64_TOL, worst  # noqa: E402


def main():
    out = {}
    for name, twists, off in bc.CASES:
        case = bc.record_case(binding.RefEKF, 20, twists, 20 + off)
        assert np.abs(case["cov0"] - case["cov0"].T).max() > 1e-5     # rows and columns differ
        # numpy's literal spelling of the same predictions meets the recording, so a GPU failure is the kernel's
        for spell in (bc.np_predict_literal, bc.np_predict_slices):
            s, c = bc.replay_case(case, spell)
            w = worst(s, c, case["state1"], case["cov1"])[0]
            print(f"{name}: {spell.__name__} vs reference worst per-block {w:.2e}")
            assert w <= FP64_TOL
        for k, v in case.items():
            out[f"{name}_{k}"] = np.asarray(v)
    path = os.path.join(HERE, "dense_predict_ref.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 100 * 1024


if __name__ == "__main__":
    main()
