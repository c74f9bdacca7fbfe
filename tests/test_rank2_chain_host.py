"""CPU: the plan of the chained pass (ekf_rank2_plan.hpp: rank2_chain_plan / rank2_chain_item, what k_rank2_chain decodes a
queue item with), swept by tests/cpp/rank2_chain_check.cpp over (B, N, m) including the benchmark's headline pool (n and B
from BASELINE.json) and the shapes of tests/test_gpu_rank2_chain.py: every tile of every filter in exactly one item, no item
over two filters, the item count equal to the queue's total, and the conditions under which a step chains.  The program also
asserts, from the header and for 256 compute units, the plan facts of every shape of tests/rank2_chain_cases.py (tile queue,
chains, ld, column chunks, 16-row tiles, rows of the last tile) and prints them; the printed table is held against that
module here.  Built plain and with AddressSanitizer + UBSan (a stand-alone program: nothing is preloaded)."""
import json
import os
import re
import subprocess

import pytest

import rank2_chain_cases as chain_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _headline():
    """(n, B) of the flagship workload, from BASELINE.json's metric and Monte-Carlo config"""
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    n = int(re.search(r"n=(\d+) landmarks", base["metric"]).group(1))
    return n, int(re.search(r"8×(\d+) independent filters", base["configs"][4]).group(1))


@pytest.mark.parametrize("sanitize", [False, True])
def test_rank2_chain_plan_sweep(tmp_path, sanitize):
    exe = str(tmp_path / "rank2_chain_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "ekf_slam_ml_amd", "csrc"),
                    "-o", exe, os.path.join(HERE, "cpp", "rank2_chain_check.cpp")], check=True)
    n, B = _headline()
    run = subprocess.run([exe, str(n), str(B)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert [line for line in lines if line.startswith("ok ")] == ["ok items 0", "ok conditions 0", "ok cases 0"], run.stdout
    # the program's table is the case module's: a shape changed in one place only fails here
    table = [line for line in lines if line.startswith("case ")]
    print("\n".join(table))
    assert table == [f"case {s.name} n={s.n} B={s.B} N={s.N} ld={s.ld} chunks={s.chunks} row_blocks={s.row_blocks} "
                     f"last_rows={s.last_rows} packing={int(s.packing)}" for s in chain_cases.SHAPES]
