"""bench.py's command line: a plain run carries the headline fields only, `--full` adds the
other legs to the same line, and `--dump-outputs` writes a fixed sample of the join's
result that equals the oracle's merge of the same synthetic replicas."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL_ONLY = ("config1_gpu", "join_t128", "config5_list_bind", "antientropy")


def test_dump_rows_are_fixed_bounded_and_cover_the_ends():
    import bench
    rows = bench.dump_rows(1 << 20, 4096)
    assert np.array_equal(rows, bench.dump_rows(1 << 20, 4096))      # seeded: run to run
    assert len(rows) == bench.DUMP_ROWS == len(set(rows.tolist()))
    assert np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == (1 << 20) - 1
    assert {1, (1 << 20) - 2} <= set(rows.tolist())
    assert np.array_equal(bench.dump_rows(7, 128), np.arange(7))     # small: every replica
    for R, E in ((1 << 20, 4096), (1000, 1 << 14), (3, 1 << 20), (1 << 20, 1 << 22)):
        n = len(bench.dump_rows(R, E))
        # float64 halves: 32 bytes per cell; one row at least (its head if wider than all)
        assert 1 <= n <= R
        assert n * min(E, bench.DUMP_BYTES // 32) * 32 <= bench.DUMP_BYTES <= 60 * 10**6


@pytest.mark.gpu
def test_plain_run_is_lean_and_dump_matches_the_oracle(tmp_path):
    """300 replicas (more than the sample takes) x 192 slots, 2 timed steps."""
    from oracle import columnar as orc
    R, E = 300, 192
    out = tmp_path / "dump"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--steps", "2", "--warmup", "1", "--replicas", str(R), "--elements",
                          str(E), "--dump-outputs", str(out)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "merged elements/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u64" and line["cpu_baseline"] is None
    assert line["value"] == pytest.approx(R * E / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(out)) == ["join_cells.npy", "join_rows.npy"]
    cells, rows = np.load(out / "join_cells.npy"), np.load(out / "join_rows.npy")
    assert cells.dtype == np.float64 and rows.dtype == np.float64
    assert cells.shape == (256, E, 2, 2) and rows[0] == 0 and rows[-1] == R - 1
    got = cells[..., 0].astype(np.uint64) | (cells[..., 1].astype(np.uint64) << np.uint64(32))
    tokens = orc.synth_tokens(E)
    for k, r in enumerate(rows.astype(np.int64)):
        A, B = orc.synth_orset(2, int(r), E), orc.synth_orset(3, int(r), E)
        assert np.array_equal(got[k], A | B), f"replica {r}"
        if k % 32 == 0 or k == len(rows) - 1:      # lasp_orset:merge/2 itself, token for token
            want = orc.ORDict.from_cells(A, tokens).merge(orc.ORDict.from_cells(B, tokens))
            assert orc.ORDict.from_cells(got[k], tokens).equal(want), f"replica {r}"


@pytest.mark.gpu
def test_full_run_carries_the_moved_legs():
    """`--full` at the smallest sizes its options allow: the line keeps the headline fields
    and gains the device legs that a plain run leaves out.  `--no-cpu`: the CPU baseline's
    own legs have fixed durations of several seconds."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--steps", "2", "--warmup", "1", "--replicas", "300", "--elements",
                          "192", "--full", "--wide-replicas", "64", "--no-cpu"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "u64"
    assert line["cpu_baseline"] is None
    assert line["config1_gpu"]["us_merge_nif"] > 0 and line["config1_gpu"]["us_bind_nif"] > 0
    assert line["config1_gpu"]["steady"]["us_per_step"] > 0
    assert line["join_t128"]["replicas"] == 64 and line["join_t128"]["kernel_ms"] > 0
    assert line["config5_list_bind"]["us_rebind_50k"] > 0
