"""bench.py --dump-outputs on the GPU: the files hold exactly what a caller of
the timed path receives (the same seeded start, W warm-up transitions, then
the K timed ones, compared bit for bit with a sampler driven directly),
--steps sets the number of timed transitions, and a dump over the byte budget
is the documented rows of the same draws."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 200 chains: not a multiple of the 64-lane wave; 7 timed transitions after 3
C, D, L, K, W = 200, 64, 5, 7, 3


def _direct(gm, n_collect):
    x0 = gm.init_with_seed(C, D, 42, np.float64, row0=0).astype(np.float32)
    s = gm.HMC(gm.RosenbrockND(), x0, 0.01, L, dtype=np.float32, chain_offset=0).set_seed(42)
    s.run_positions(W, 0)
    return s, s.run_positions(n_collect, 0)


def test_dump_outputs_are_the_timed_calls_arrays(gm, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", str(W), "--chains", str(C), "--dim", str(D), "--leapfrog", str(L),
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == K and line["full"] is False and "configs" not in line
    assert line["ms_per_step"] == line["timing"]["wall_ms"] / K
    assert line["outputs"]["positions"]["rows"] == list(range(K))
    pos = np.load(tmp_path / "positions.npy")
    acc = np.load(tmp_path / "accept_counts.npy")
    assert pos.dtype == np.float32 and pos.shape == (K, C, D)
    assert acc.dtype == np.float64 and acc.shape == (C,)
    s, ds = _direct(gm, K)
    try:
        assert np.array_equal(pos, ds.block(0, K, 0, C))
        assert np.array_equal(acc, s.accept_counts().astype(np.float64))
    finally:
        s.close()
    assert np.isfinite(pos).all() and 0 < acc.sum() <= (K + W) * C


def test_dump_over_budget_is_the_sampled_rows(gm, monkeypatch):
    import bench
    from general_mcmc_amd.distributed import ControlPlane

    # room for 144 chain-rows: a sixteenth of the budget bounds the chains (9
    # of the 200), the rest the rows (16 of the 20)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 144 * D * 4)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = bench.parse(["--chains", str(C), "--dim", str(D), "--leapfrog", str(L)])
    be = bench.GpuBench(a, ControlPlane())
    n = 20
    s, ds = _direct(gm, n)
    try:
        arrays, rows = be.outputs(s, ds)
        keep = 9
        assert len(rows) == 16 and rows == sorted(set(rows)) and rows[-1] == n - 1
        assert arrays["positions"].shape == (16, keep, D)
        full = ds.block(0, n, 0, C)
        assert np.array_equal(arrays["positions"], full[rows][:, :keep])
        assert np.array_equal(arrays["accept_counts"], s.accept_counts()[:keep].astype(np.float64))
    finally:
        s.close()
