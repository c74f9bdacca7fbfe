"""CPU: the launch plan of the eager rank-2 correction (ekf_rank2_plan.hpp: the one place launch_rank2 and the report hooks
ekf_batch_rank2_variant / _resident / _packing decide from), swept by tests/cpp/rank2_plan_check.cpp: every reason for
P = 1 where the header says it fires, the work floor at its exact edge, util(P) >= 0.97 > util(P') for P' < P, the grid over
ceil(N / P) virtual rows, packed never the queue, no packing without full_width, and the benchmark's headline pool (n and B
from BASELINE.json) on the tile queue with P = 1.  Built plain and with AddressSanitizer + UBSan (a stand-alone program:
nothing is preloaded).

The program's table (n, smallest packing B) -> P is kept for the shapes the GPU tests use in
tests/golden/rank2_packing_table.txt: a retune of the heuristic is a diff there, and the GPU case lists are checked against
it here, so that no row-packing case can go empty unnoticed."""
import json
import os
import re
import subprocess

import pytest

import dense_sigma_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WANT = ["ok sweep 1843200 plans", "ok prefix views", "ok work floor edges", "ok headline"]
PARITY_PACKED = ((200, 64), (100, 200), (60, 540), (333, 24), (376, 20))   # test_row_packed_rank2_is_bit_identical's shapes


def _headline():
    """(n, B) of the flagship workload, from BASELINE.json's metric and Monte-Carlo config"""
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    n = int(re.search(r"n=(\d+) landmarks", base["metric"]).group(1))
    m = re.search(r"8×(\d+) independent filters .* at n=(\d+)", base["configs"][4])
    assert int(m.group(2)) == n
    return n, int(m.group(1))


def _fixture():
    rows, resident = {}, None
    for line in open(os.path.join(HERE, "golden", "rank2_packing_table.txt")):
        if line.startswith("resident"):
            resident = line.strip()
        elif not line.startswith("#"):
            n, B, P, ld2n = (int(x) for x in line.split())
            rows[n] = (B, P, ld2n)
    return rows, resident


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    out = {}
    n, B = _headline()
    for sanitize in (False, True):
        exe = str(tmp_path_factory.mktemp("rank2_plan") / "rank2_plan_check")
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags,
                        "-I", os.path.join(ROOT, "ekf_slam_ml_amd", "csrc"),
                        "-o", exe, os.path.join(HERE, "cpp", "rank2_plan_check.cpp")], check=True)
        out[sanitize] = subprocess.run([exe, str(n), str(B)], capture_output=True, text=True)
    return out


@pytest.mark.parametrize("sanitize", [False, True])
def test_rank2_plan_sweep(program_output, sanitize):
    run = program_output[sanitize]
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    ok = [line for line in run.stdout.split("\n") if line.startswith("ok ")]
    assert len(ok) == len(WANT) and all(line.startswith(w) for line, w in zip(ok, WANT)), run.stdout[:2000]
    n, B = _headline()
    assert ok[3] == f"ok headline n={n} B={B} k_rank2_queue<16,true,256> rows 32"   # (bench.py ties a traffic record to this name)
    assert program_output[True].stdout == program_output[False].stdout


def test_packing_table_matches_the_fixture_and_the_gpu_cases(program_output):
    assert program_output[False].returncode == 0, program_output[False].stdout[-2000:]
    table = {}
    resident = None
    for line in program_output[False].stdout.split("\n"):
        if line.startswith("table "):
            n, B, P, ld2n = (int(x) for x in line.split()[1:])
            table[n] = (B, P, ld2n)
        elif line.startswith("resident"):
            resident = line.strip()
    assert min(table) >= 30 and max(table) <= 400 and len(table) > 100
    rows, fixture_resident = _fixture()
    assert {n: table.get(n) for n in rows} == rows            # a retune of rank2_packing() shows here ...
    assert resident == fixture_resident
    # ... and the GPU cases are what the table says: the new list sits AT the work floor, the older shapes above it
    for n, B, P in cases.POOL_PACKED_PLAN:
        assert rows[n][:2] == (B, P), (n, B, P, rows[n])
    n, B = cases.POOL_PACKED_BELOW
    assert rows[n][0] == B + 1 and n == cases.POOL_PACKED_TUNING_N
    n, B, P = cases.POOL_PACKED_QUEUE
    assert resident == f"resident n={n} B_min={B} P={P}"
    for n, B in cases.POOL_PACKED + PARITY_PACKED:
        assert B >= rows[n][0] and rows[n][1] > 1, (n, B, rows[n])
    # what the list covers (tests/dense_sigma_cases.py says why each case is there)
    plan = {n: (3 + 2 * n, P, rows[n][2]) for n, _, P in cases.POOL_PACKED_PLAN}
    assert any(N % P == 0 for N, P, _ in plan.values()) and any(N % P == 1 for N, P, _ in plan.values())
    assert any(ld2n == 64 for _, _, ld2n in plan.values()) and any(ld2n % 64 for _, _, ld2n in plan.values())
    assert max(P for _, P, _ in plan.values()) == max(P for _, P, _ in table.values())     # the largest P any pool takes
    assert all(B * (3 + 2 * n) * 2 * ld2n * 8 <= 100e6 for n, (B, _, ld2n) in table.items())   # ... and every row is < 100 MB of Sigma
    assert min(P for _, P, _ in plan.values()) == 2 == min(P for _, P, _ in table.values())
    N, P, _ = plan[cases.POOL_PACKED_TUNING_N]
    assert all(-(-N // P) % rows for rows, _, _ in cases.POOL_PACKED_TUNING) and -(-N // P) % 8   # a short last block of virtual rows
