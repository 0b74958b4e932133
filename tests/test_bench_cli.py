"""bench.py's plain line and --dump-outputs: the files a comparison of two builds reads, their format and their size bound."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_FILES = ("out_rows", "out_rows_index", "out_head_sum", "kept_counts")


def _bench(args, env=None, timeout=900):
    env = dict(os.environ if env is None else env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    arrs = {n: np.load(os.path.join(d, f"{n}.npy")) for n in DUMP_FILES}
    assert sorted(os.listdir(d)) == sorted(f"{n}.npy" for n in DUMP_FILES)
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    return arrs


def test_dump_outputs_rows_and_sums():
    """dump_outputs on a stand-in call (host tensors): the sampled rows are O's rows, the head sums cover every row, the
    last 128-row block is always in the sample, the sample respects the byte budget and does not depend on the run."""
    import tempfile
    import bench
    B, S, H, D, NBv = 1, 1000, 4, 64, 7
    out = torch.randn(B, S, H, D).to(torch.bfloat16)
    call = types.SimpleNamespace(out=out, bufs={"counts": torch.arange(B * H * NBv, dtype=torch.int32).reshape(B * H, NBv)})
    comm = types.SimpleNamespace(world=1, rank=0, dist=None)
    old = bench.DUMP_ROWS_BYTES
    try:
        bench.DUMP_ROWS_BYTES = 4 * H * D * 300
        with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
            bench.dump_outputs(comm, call, d1)
            bench.dump_outputs(comm, call, d2)
            a, a2 = _load(d1), _load(d2)
    finally:
        bench.DUMP_ROWS_BYTES = old
    rows = a["out_rows_index"].astype(np.int64)
    assert len(rows) == 300 and np.all(np.diff(rows) > 0) and set(range(S - 128, S)) <= set(rows.tolist())
    assert np.array_equal(a["out_rows"], out.float().numpy()[:, rows])
    assert np.allclose(a["out_head_sum"], out.double().sum(1).numpy(), rtol=0, atol=1e-9)
    assert a["kept_counts"].shape == (B, H, NBv) and a["kept_counts"][0, 1, 0] == NBv
    for n in DUMP_FILES:
        assert np.array_equal(a[n], a2[n])


@pytest.mark.gpu
def test_plain_line_and_dump_one_and_two_ranks(tmp_path):
    """A plain run prints the headline fields for exactly --steps timed steps and nothing of --full; its dump holds finite
    rows of every head.  The same arguments at --gpus 2 (both ranks on one device, test hook) dump the same arrays: the mask
    bit for bit, O within rounding (the tail plan of a launch depends on its size)."""
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    rec = _bench(["--gpus", "1", "--workload", "tiny", "--steps", "3", "--warmup", "1", "--dump-outputs", d1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in rec, key
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["dtype"] == "bf16" and rec["higher_is_better"] is True
    assert not {"check", "cpu_baseline", "sustained", "regimes", "api", "fp8", "box_ref"} & set(rec)
    a = _load(d1)
    H, D = 4, 128
    assert a["out_rows"].shape[2:] == (H, D) and a["out_head_sum"].shape == (1, H, D)
    assert np.isfinite(a["out_rows"]).all() and np.isfinite(a["out_head_sum"]).all()
    assert float(np.abs(a["out_rows"]).max()) > 0

    env = dict(os.environ, RSA_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    rec2 = _bench(["--gpus", "2", "--workload", "tiny", "--steps", "3", "--warmup", "1", "--dump-outputs", d2], env=env)
    assert rec2["n_gpus"] == 2 and rec2["steps"] == 3
    b = _load(d2)
    assert np.array_equal(a["out_rows_index"], b["out_rows_index"])
    assert np.array_equal(a["kept_counts"], b["kept_counts"])
    assert np.abs(a["out_rows"] - b["out_rows"]).max() < 2e-2
    S = 4096 + 256
    assert np.abs(a["out_head_sum"] - b["out_head_sum"]).max() <= S * 2e-2   # every row within the row bound above
