"""Fused small-MLP step at padded input widths 384 and 512 (mlp_small_wide_kernel, 64-row tile)
against the fp32 CPU trainer on the same bf16-rounded inputs and weights.  3000 rows in 1024-row
chunks: a 952-row tail chunk of 14 tiles + 56 rows whose last 16-row strip holds 8 rows, on both
chunk lanes."""
import pytest
import torch

from shifu_amd.models.nn import MLPSpec, MLPTrainer
from test_mlp_small_gpu import _check, _data, _first_gradient, _pair

pytestmark = pytest.mark.gpu

CASES = [
    (256, [10], ["relu"], "squared"),                    # smallest width past the old bound, kp0 = 384
    (300, [50], ["tanh"], "squared"),                    # kp0 = 384, width not a multiple of 16
    (511, [64], ["sigmoid"], "squared"),                 # the bound: bias in the last column, full width
    (400, [45, 45], ["sigmoid", "tanh"], "squared"),     # two-layer dgrad at kp0 = 512 (all of the LDS)
    (300, [20, 7], ["leakyrelu", "sigmoid"], "squared"),
    (400, [33, 64], ["log", "leakyrelu_tf"], "log"),
    (383, [64], ["linear"], "absolute"),                 # kp0 = 384 exactly filled
]


@pytest.mark.parametrize("n_in,hidden,acts,loss", CASES)
def test_wide_gradient_and_error_match_cpu(n_in, hidden, acts, loss, monkeypatch):
    monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", "1")
    _check(MLPSpec(n_in=n_in, hidden=hidden, acts=acts, loss=loss), 3000)


def test_wide_fewer_rows_than_a_tile(monkeypatch):
    monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", "1")
    _check(MLPSpec(n_in=400, hidden=[45, 45], acts=["sigmoid", "tanh"]), 40)


def test_wide_gradient_is_reproducible(monkeypatch):
    monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", "1")
    _, gpu = _pair(MLPSpec(n_in=400, hidden=[33, 64], acts=["log", "leakyrelu_tf"]))
    assert gpu.fused_small
    d = gpu.prepare(*_data(400, 3000))
    (g1, e1), (g2, e2) = _first_gradient(gpu, d), _first_gradient(gpu, d)
    assert torch.equal(g1, g2) and torch.equal(e1, e2)


@pytest.mark.parametrize("n_in,hidden,acts,loss", CASES[1:4])
def test_wide_predict_matches_cpu(n_in, hidden, acts, loss, monkeypatch):
    monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", "1")
    cpu, gpu = _pair(MLPSpec(n_in=n_in, hidden=hidden, acts=acts), seed=8)
    assert gpu.fused_small
    x, y, s = _data(n_in, 2500, seed=1)
    pc = cpu.predict_rows(cpu.prepare(x, y, s).x)
    pg = gpu.predict_rows(gpu.prepare(x, y, s).x).cpu()
    assert pg.shape == (2500, 1)
    assert float((pc - pg).abs().max()) < 2e-2


def test_wide_bound_kp0_640_keeps_its_path(monkeypatch):
    # 16 rows: one contributor per float atomic of the layer-kernel path, so its gradient is
    # bitwise defined (the argument of the existing fallback test)
    spec = MLPSpec(n_in=600, hidden=[50], acts=["sigmoid"])
    x, y, s = _data(600, 16)
    monkeypatch.delenv("SHIFU_MLP_FUSED_SMALL", raising=False)
    grads = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", env)
        t = MLPTrainer(spec, device="cuda", seed=5, chunk_rows=1024)
        assert not t.fused_small
        grads.append(_first_gradient(t, t.prepare(x, y, s))[0])
    assert torch.equal(grads[0], grads[1])
