"""bench.py --dump-outputs DIR: what the timed path returned in its last step, as DIR/<name>.npy (float64, at most 64 MB in
all, larger outputs as a seeded sample of rows), identical from run to run so that two builds can be compared file by file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_steps_must_be_positive():
    assert bench.parse_args(["--steps", "4"]).steps == 4
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_small_outputs_are_written_whole(tmp_path):
    sc = torch.from_numpy(np.random.RandomState(0).rand(1000, 3))
    bench.dump_outputs(str(tmp_path), {"sc_edge_info": sc, "row_ptr": torch.tensor([0, 400, 1000])})
    got = _read(tmp_path)
    assert sorted(got) == ["row_ptr", "sc_edge_info"]
    assert got["sc_edge_info"].dtype == np.float64 and np.array_equal(got["sc_edge_info"], sc.numpy())
    assert got["row_ptr"].dtype == np.float64 and list(got["row_ptr"]) == [0, 400, 1000]


def test_large_outputs_are_a_seeded_sample_within_the_budget(tmp_path):
    m = bench.DUMP_MAX_ROWS + 12345
    sc = torch.from_numpy(np.random.RandomState(1).rand(m, 3))
    rp = torch.arange(m, dtype=torch.int64)
    runs = []
    for k in range(2):
        d = str(tmp_path / str(k))
        bench.dump_outputs(d, {"sc_edge_info": sc, "row_ptr": rp})
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
        runs.append(_read(d))
    a, b = runs
    assert sorted(a) == ["row_ptr", "row_ptr_sample_rows", "sc_edge_info", "sc_edge_info_sample_rows"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["sc_edge_info_sample_rows"].astype(np.int64)
    assert rows.shape == (bench.DUMP_MAX_ROWS,) and (np.diff(rows) > 0).all() and rows[-1] < m
    assert np.array_equal(a["sc_edge_info"], sc.numpy()[rows])
    assert np.array_equal(a["row_ptr"], rows.astype(np.float64))


@pytest.mark.gpu
def test_bench_dumps_the_timed_output_reproducibly(tmp_path):
    """Two runs with the same arguments write the same files, and they hold what the oracle computes for the workload."""
    import oracle
    from rlap_amd import graphs
    n, m = 20000, 5
    outs = []
    for k in range(2):
        d = str(tmp_path / str(k))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--nodes", str(n), "--m", str(m), "--steps", "2",
                            "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", d], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["steps"] == 2
        outs.append(_read(d))
    assert sorted(outs[0]) == ["sc_edge_info"]
    assert np.array_equal(outs[0]["sc_edge_info"], outs[1]["sc_edge_info"])
    ref = oracle.approximate_cholesky(graphs.barabasi_albert(n, m, 2).numpy(), None, n, n // 2, "degree", "asc", shuffle_seed=7)
    assert np.array_equal(outs[0]["sc_edge_info"], ref)
