"""bench.py --dump-outputs: the files a run leaves for an output-for-output comparison of
two builds (host logic only: the arrays here are CPU tensors standing in for the state
the last timed step left)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("losses", "params", "grads", "adam_m", "adam_v")


def _state(pc, tail=16):
    g = torch.Generator().manual_seed(3)
    flat = lambda: torch.randn(pc + tail, generator=g, dtype=torch.float32)
    model = SimpleNamespace(param_count=pc, params=flat())
    opt = SimpleNamespace(losses=torch.randn(8, generator=g, dtype=torch.float64),
                          grads=flat(), m=flat(), v=flat())
    return model, opt


def test_dump_outputs_writes_every_array(tmp_path):
    model, opt = _state(1000)
    d = tmp_path / "out"
    bench.dump_outputs(str(d), model, opt)
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    got = {n: np.load(d / (n + ".npy")) for n in NAMES}
    assert got["losses"].dtype == np.float64 and got["losses"].shape == (8,)
    np.testing.assert_array_equal(got["losses"], opt.losses.numpy())
    for n, t in (("params", model.params), ("grads", opt.grads), ("adam_m", opt.m), ("adam_v", opt.v)):
        assert got[n].dtype == np.float32
        np.testing.assert_array_equal(got[n], t[:1000].numpy())     # the tail is not a parameter


def test_dump_outputs_samples_above_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 5 * 400)     # 400 bytes per array
    model, opt = _state(1000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), model, opt)
    bench.dump_outputs(str(b), model, opt)
    total = 0
    for n in NAMES:
        x, y = np.load(a / (n + ".npy")), np.load(b / (n + ".npy"))
        np.testing.assert_array_equal(x, y)               # the same sample in every run
        total += x.nbytes
    assert total <= 5 * 400
    idx = np.sort(np.random.default_rng(0).integers(0, 1000, 100))
    np.testing.assert_array_equal(np.load(a / "params.npy"), model.params[:1000].numpy()[idx])
    assert np.load(a / "losses.npy").shape == (8,)        # 64 bytes: under its share, whole


def test_bench_options_listed():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout
