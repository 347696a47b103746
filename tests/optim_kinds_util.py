"""Shared pieces of the NAdamW / Lion tests (tests/test_emu_optim_kinds.py on the emulator, tests/test_gpu_optim_kinds.py on the GPU):
the recorded reference runs of tests/golden/optim_kinds.npz (made by make_golden_optim.py) and the tiny_cheb_f32 model they train."""
import types

import numpy as np
import torch

from tests.helpers import cfg_from_fixture, fixture_gso, fixture_params, load_fixture, maxabs

KINDS = ("nadamw", "lion")


def optim_fixture():
    return load_fixture("optim_kinds")


def tiny_model(dev="cpu", droprate=0.0):
    """the reference model of the tiny_cheb_f32 fixture (its weights), and that fixture's batch (make_golden.synth_xy)"""
    from stgcn_amd import models
    fx = load_fixture("tiny_cheb_f32")
    cfg = cfg_from_fixture(fx)
    N, B = int(fx["n_vertex"]), int(fx["B"])
    args = types.SimpleNamespace(Kt=cfg.Kt, Ks=cfg.Ks, act_func=cfg.act_func, graph_conv_type=cfg.graph_conv_type,
                                 gso=torch.from_numpy(fixture_gso("tiny_cheb_f32", fx)).to(dev), enable_bias=True, droprate=droprate,
                                 n_his=cfg.n_his)
    m = models.STGCNChebGraphConv(args, cfg.blocks, N)
    m.load_state_dict(fixture_params(fx, cfg, torch.float32), strict=True)
    m = m.to(dev)
    m.train()
    rs = np.random.RandomState(int(fx["seed"]) + 1)
    x = torch.from_numpy(rs.standard_normal((B, 1, cfg.n_his, N))).float().to(dev)
    y = torch.from_numpy(rs.standard_normal((B, N))).float().to(dev)
    return m, x, y


def check_trajectory(name, losses, model, fo):
    """losses and parameters of 3 training steps against the reference's (fixture part b).  Lion: only where the reference's update
    direction c is clear of zero at every step (|c| > 1e-5 max|c|): elsewhere its sign is not determined at fp32 gradient accuracy."""
    pre = f"train.{name}."
    assert np.allclose(losses, fo[pre + "losses"], rtol=1e-4), (losses, fo[pre + "losses"])
    checked = 0
    for k, v in model.state_dict().items():
        if pre + "param." + k not in fo:
            continue
        got, ref = v.detach().cpu().numpy(), fo[pre + "param." + k][-1]
        if name == "lion" and pre + "c." + k in fo:
            c = fo[pre + "c." + k]
            clear = np.all(np.abs(c) > 1e-5 * np.abs(c).reshape(len(c), -1).max(1).reshape((-1,) + (1,) * (c.ndim - 1)), axis=0)
            assert clear.mean() > 0.9, k
            got, ref = got[clear], ref[clear]
        assert maxabs(got, ref) <= 1e-4, (k, maxabs(got, ref))
        checked += 1
    assert checked >= 20
