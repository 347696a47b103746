"""CPU: bench.py --dump-outputs writes the loss, parameters and gradients of the last step as float32 .npy files inside the 64 MB
budget, sampling an over-budget array at the same seeded positions every time."""
import os

import numpy as np
import torch

import bench


def _model_after_one_step():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 1))
    m[0].bias.requires_grad_(False)          # a parameter without a gradient gets no grad.<name> file
    loss = m(torch.randn(4, 8)).pow(2).mean()
    loss.backward()
    return m, loss


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_writes_loss_params_and_grads(tmp_path):
    m, loss = _model_after_one_step()
    rec = bench.dump_outputs(str(tmp_path / "out"), loss, m)
    got = _load(rec["dir"])
    assert set(got) == {"loss", "param.0.weight", "param.0.bias", "param.1.weight", "param.1.bias",
                        "grad.0.weight", "grad.1.weight", "grad.1.bias"}
    assert all(a.dtype == np.float32 for a in got.values()) and rec["sampled"] == []
    assert got["loss"].shape == () and got["loss"] == np.float32(loss.item())
    np.testing.assert_array_equal(got["param.0.weight"], m[0].weight.detach().numpy())
    np.testing.assert_array_equal(got["grad.1.weight"], m[1].weight.grad.numpy())
    assert rec["bytes"] == sum(a.nbytes for a in got.values())
    assert open(os.path.join(rec["dir"], ".gitignore")).read() == "*\n"


def test_dump_samples_over_budget_arrays_at_fixed_positions(tmp_path, monkeypatch):
    m, loss = _model_after_one_step()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", (1 << 20) + 8 * 4 * 32)      # 32 elements per array
    a = bench.dump_outputs(str(tmp_path / "a"), loss, m)
    b = bench.dump_outputs(str(tmp_path / "b"), loss, m)
    assert sorted(a["sampled"]) == ["grad.0.weight", "param.0.weight"]
    ga, gb = _load(a["dir"]), _load(b["dir"])
    assert ga["param.0.weight"].shape == (32,)
    w = m[0].weight.detach().numpy().reshape(-1)
    assert np.isin(ga["param.0.weight"], w).all()
    for k in ga:
        np.testing.assert_array_equal(ga[k], gb[k])
