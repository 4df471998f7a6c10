"""bench.py's multi-GPU entry (no GPU needed): ``python bench.py --gpus N``
outside a launcher starts N ranks under torch.distributed.run as a child
process and relays its exit code; under a launcher, WORLD_SIZE must equal
--gpus.  Also the options of a plain run and the files --dump-outputs writes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_launcher_command():
    cmd = bench.launcher_cmd(["--gpus", "8", "--steps", "3"], 8, 29511)
    assert cmd == [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                   "--nproc-per-node=8", "--master-addr", "127.0.0.1", "--master-port", "29511",
                   os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3"]


def test_gpus_gt1_relays_a_child_launcher(monkeypatch):
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return subprocess.CompletedProcess(cmd, 3)

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "4"])
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert ex.value.code == 3                       # the child's return code
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert "--nproc-per-node=2" in cmd and cmd[-4:] == ["--gpus", "2", "--steps", "4"]
    assert seen["env"]["MASTER_ADDR"] == "127.0.0.1"
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float32 .npy files; an array above 16 MB becomes the
    same seeded, ascending row sample in every run, its row numbers beside it."""
    import types

    import numpy as np
    import torch
    n, F = 40_000, 128                                  # 20.5 MB of float32: sampled
    agg = torch.arange(n, dtype=torch.float32)[:, None].expand(n, F)
    codes = torch.arange(50 * 3, dtype=torch.int16).view(50, 3)
    bidx = torch.tensor([4, 2, 9], dtype=torch.int32)
    names = ("emb", "emb_out", "ema_w", "cs", "rm_f", "rv_f", "rm_g", "rv_g")
    bank = types.SimpleNamespace(**{k: torch.full((2, 3), float(i)) for i, k in enumerate(names)})
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, agg, codes, bidx, bank)
        got.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = got
    assert set(a) == {"aggregate", "aggregate_rows", "codes"} | {f"bank_{k}" for k in names}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    rows = a["aggregate_rows"]
    assert a["aggregate"].shape == (32768, F) and rows.shape == (32768,)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a["aggregate"][:, 0], rows)
    assert np.array_equal(a["codes"], codes[bidx.long()].numpy().astype(np.float32))
    assert np.array_equal(a["bank_cs"], np.full((2, 3), 3.0, np.float32))
    # rank r > 0 of a multi-GPU run writes beside rank 0's files
    bench.dump_outputs(str(tmp_path / "a"), 1, agg[:10], codes, bidx, bank)
    assert np.load(tmp_path / "a" / "aggregate.rank1.npy").shape == (10, F)


def test_world_size_must_match_gpus(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert "WORLD_SIZE=4" in str(ex.value.code)
