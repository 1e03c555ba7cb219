"""bench.py's options and its --dump-outputs writer, without a GPU (the writer takes any torch tensors)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("rib_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_is_the_default_and_steps_are_at_least_one():
    bench = _bench_module()
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_writes_float32_arrays_whole_when_they_fit(tmp_path):
    bench = _bench_module()
    img = torch.randn(1, 3, 8, 8)
    mask = torch.rand(1, 1, 8, 8, dtype=torch.float64)
    fuse = torch.randn(2, 1, 3, 8, 8).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path), {"img": img, "mask": mask, "fuse": fuse}, lambda msg: None)
    got = {n: np.load(str(tmp_path / (n + ".npy"))) for n in ("img", "mask", "fuse")}
    assert got["img"].dtype == np.float32 and np.array_equal(got["img"], img.numpy())
    assert got["mask"].dtype == np.float64 and np.array_equal(got["mask"], mask.numpy())
    assert got["fuse"].dtype == np.float32 and np.array_equal(got["fuse"], fuse.float().numpy())


def test_dump_samples_the_same_elements_when_the_outputs_exceed_the_budget(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 4096 + 4 * 3000)
    big = torch.arange(4000, dtype=torch.float32).reshape(4, 1000)
    small = torch.arange(2000, dtype=torch.float32) + 0.5
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"big": big, "small": small}, lambda msg: None)
    sizes = 0
    for n, t in (("big", big), ("small", small)):
        a, b = np.load(str(tmp_path / "a" / (n + ".npy"))), np.load(str(tmp_path / "b" / (n + ".npy")))
        assert np.array_equal(a, b) and a.ndim == 1 and 0 < a.size < t.numel()
        assert np.all(np.diff(a) > 0) and np.all(np.isin(a, t.numpy()))       # distinct elements, in flat order
        sizes += os.path.getsize(str(tmp_path / "a" / (n + ".npy")))
    assert sizes <= bench.DUMP_BUDGET_BYTES
