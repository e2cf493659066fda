"""Fused one-kernel gradient step of small MLPs (ops/csrc/mlp_small.hip, SHIFU_MLP_FUSED_SMALL=1)
against the fp32 CPU trainer on the same bf16-rounded inputs and weights.  3000 rows in 1024-row
chunks: a 952-row tail chunk whose last 32-row strip holds 24 rows, on both chunk lanes."""
import pytest
import torch

from shifu_amd.models.nn import MLPSpec, MLPTrainer

pytestmark = pytest.mark.gpu

CASES = [
    (90, [50], ["sigmoid"], "squared"),                  # kp0 = 128, width not a multiple of 16
    (200, [64], ["tanh"], "squared"),                    # kp0 = 256 (the bound), full width
    (200, [10], ["relu"], "squared"),                    # one 16-node block
    (90, [45, 45], ["sigmoid", "tanh"], "squared"),      # two-layer dgrad
    (200, [20, 7], ["leakyrelu", "sigmoid"], "squared"),
    (90, [33, 64], ["log", "leakyrelu_tf"], "log"),
    (200, [50], ["linear"], "absolute"),
]


def _data(n_in, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, n_in, generator=g).bfloat16().float()
    y = (x[:, :3].sum(1, keepdim=True) > 0).float()
    return x, y, torch.rand(n, generator=g) + 0.5


def _pair(spec, seed=5):
    cpu = MLPTrainer(spec, device="cpu", seed=seed, chunk_rows=1000, propagation="R")
    gpu = MLPTrainer(spec, device="cuda", seed=seed, chunk_rows=1024, propagation="R")
    cpu.params.flat.copy_(cpu.params.flat.bfloat16().float())
    gpu.params.flat.copy_(cpu.params.flat.cuda())
    return cpu, gpu


def _first_gradient(t, d):
    t.grad.zero_(); t.err_acc.zero_(); t.accumulate_gradients(d)
    if t.gpu:
        torch.cuda.synchronize()
    return t.grad.cpu().clone(), t.err_acc.cpu().clone()


def _check(spec, n):
    cpu, gpu = _pair(spec)
    assert gpu.fused_small
    x, y, s = _data(spec.n_in, n)
    (gc, ec), (gg, eg) = _first_gradient(cpu, cpu.prepare(x, y, s)), _first_gradient(gpu, gpu.prepare(x, y, s))
    assert float((gc - gg).norm() / gc.norm()) < 3e-2
    for vc, vg in zip(cpu.params.views(gc), gpu.params.views(gg)):
        assert float((vc - vg).norm() / vc.norm().clamp(min=1e-12)) < 5e-2
    assert abs(float(ec[0]) - float(eg[0])) / float(ec[0]) < 1e-2
    assert abs(float(ec[1]) - float(eg[1])) < 1e-2


@pytest.mark.parametrize("n_in,hidden,acts,loss", CASES)
def test_small_gradient_and_error_match_cpu(n_in, hidden, acts, loss, monkeypatch):
    monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", "1")
    _check(MLPSpec(n_in=n_in, hidden=hidden, acts=acts, loss=loss), 3000)


def test_small_fewer_rows_than_a_tile(monkeypatch):
    monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", "1")
    _check(MLPSpec(n_in=90, hidden=[45, 45], acts=["sigmoid", "tanh"]), 70)


def test_small_gradient_is_reproducible(monkeypatch):
    monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", "1")
    spec = MLPSpec(n_in=200, hidden=[20, 7], acts=["leakyrelu", "sigmoid"])
    _, gpu = _pair(spec)
    d = gpu.prepare(*_data(200, 3000))
    (g1, e1), (g2, e2) = _first_gradient(gpu, d), _first_gradient(gpu, d)
    assert torch.equal(g1, g2) and torch.equal(e1, e2)


@pytest.mark.parametrize("n_in,hidden,acts,loss", CASES[1:4])
def test_small_predict_matches_cpu(n_in, hidden, acts, loss, monkeypatch):
    monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", "1")
    cpu, gpu = _pair(MLPSpec(n_in=n_in, hidden=hidden, acts=acts), seed=8)
    assert gpu.fused_small
    x, y, s = _data(n_in, 2500, seed=1)
    pc = cpu.predict_rows(cpu.prepare(x, y, s).x)
    pg = gpu.predict_rows(gpu.prepare(x, y, s).x).cpu()
    assert pg.shape == (2500, 1)
    assert float((pc - pg).abs().max()) < 2e-2


@pytest.mark.parametrize("hidden,acts", [([65], ["sigmoid"]), ([40], ["ptanh"])])
def test_small_ineligible_nets_keep_their_path(hidden, acts, monkeypatch):
    # 16 rows: one block in the output kernel and one wgrad split, so the float atomics of the
    # layer-kernel path have a single contributor and its gradient is bitwise defined
    spec = MLPSpec(n_in=90, hidden=hidden, acts=acts)
    x, y, s = _data(90, 16)
    grads = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("SHIFU_MLP_FUSED_SMALL", env)
        t = MLPTrainer(spec, device="cuda", seed=5, chunk_rows=1024)
        assert not t.fused_small
        grads.append(_first_gradient(t, t.prepare(x, y, s))[0])
    assert torch.equal(grads[0], grads[1])


def test_small_is_opt_in(monkeypatch):
    monkeypatch.delenv("SHIFU_MLP_FUSED_SMALL", raising=False)
    assert not MLPTrainer(MLPSpec(n_in=90, hidden=[50], acts=["tanh"]), device="cuda", seed=5).fused_small
