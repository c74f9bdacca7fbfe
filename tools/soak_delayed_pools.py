"""Extended differential check of pools' delayed data_association() (ekf_stepfused.hip, DELAYED + block cache) against the
eager run of the same pool: random pool sizes, map sizes, corrections per flush, surveyed shares, ragged reading counts,
filters that sit steps out, run boundaries.  Decisions and known counts must be identical, states within 1e-9.
(scenarios and runs: tests/pool_soak_cases.py, which the seeded slice under -m gpu shares -- DELAYED_POOL_SEEDS, tests/test_gpu_pool_soak.py)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: F401  (one HIP runtime)
from ekf_slam_ml_amd import capi as hip
import pool_soak_cases as cases

N_SCEN = int(sys.argv[1]) if len(sys.argv) > 1 else 60
bad = 0
for seed in range(N_SCEN):
    r = cases.run_delayed_pool(hip, cases.delayed_pool_scenario(seed))
    if not r.ok:
        bad += 1
        print(r.fail_line(), flush=True)
    if seed % 10 == 9:
        print("scenario", seed, "failures so far", bad, flush=True)
print("done, failures:", bad)
