"""bench.py's command line without a GPU: a plain run is the default (--full
off), and --dump-outputs writes float32 .npy files within its size limit."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float32(tmp_path):
    acts = torch.tensor([[0, 3], [2, 1]], dtype=torch.int32)
    u8 = torch.arange(256, dtype=torch.uint8)
    f = torch.tensor([1.5, -2.25e-30, 3e38])
    bench.dump_outputs(str(tmp_path / "o"), {"actions": acts, "planes": u8, "v": f})
    got = {k: np.load(tmp_path / "o" / (k + ".npy")) for k in ("actions", "planes", "v")}
    assert all(x.dtype == np.float32 for x in got.values())
    assert (got["actions"] == acts.numpy()).all() and (got["planes"] == u8.numpy()).all()
    assert (got["v"] == f.numpy()).all()


def test_dump_outputs_refuses_more_than_the_limit(tmp_path):
    big = torch.zeros(bench.DUMP_MAX_BYTES // 4 + 1)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "o"), {"big": big})
    assert not list((tmp_path / "o").iterdir())
