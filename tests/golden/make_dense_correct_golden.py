"""Writes tests/golden/dense_correct_ref.npz: inputs and recorded outputs of the reference build's measurement() (one
visible landmark, three visible landmarks) at n = 20, for the never-skipping replay of tests/test_gpu_dense64_correct.py.
Needs oracle/_ref/libekf_slam_ref.so (built by __graft_entry__.build() where the reference sources are present).

    python tests/golden/make_dense_correct_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import binding  # noqa: E402
import dense_correct_cases as dc  # noqa: E402
from parity import FP64_TOL, worst  # noqa: E402


def main():
    out = {}
    for name, nvis, off in dc.CASES:
        case = dc.record_case(binding.RefEKF, 20, nvis, 20 + off)
        # numpy's literal spelling of the same corrections meets the recording, so a GPU failure is the kernel's
        s, c, nis = dc.replay_case(case, dc.np_correct)
        w = worst(s, c, case["state1"], case["cov1"])[0]
        rel = abs(nis - case["maha"]) / abs(case["maha"])
        print(f"{name}: numpy vs reference worst per-block {w:.2e}, nis rel {rel:.2e}")
        assert w <= FP64_TOL and rel <= FP64_TOL
        for k, v in case.items():
            out[f"{name}_{k}"] = np.asarray(v)
    path = os.path.join(HERE, "dense_correct_ref.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
