#!/usr/bin/env python3
"""Generate the NAdamW / Lion fixture (optim_kinds.npz) by RUNNING THE REFERENCE's optimizers.

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_optim.py

The two optimizers are those main.py:149-152 builds for ``--opt nadamw`` and ``--opt lion``:
``torch.optim.NAdam(..., decoupled_weight_decay=True)`` and the reference's ``script/opt.py`` ``Lion``.

  (a) ``alone.*``: each optimizer alone for 6 steps on a handful of seeded fp32 tensors (one more tensor never gets a gradient),
      with StepLR(step_size=3, gamma=0.5) halving lr after step 3: initial values, the gradient sequence, parameters and state after
      every step, and for Lion the update direction c = beta1 m + (1 - beta1) g of every step.
  (b) ``train.<opt>.*``: 3 training steps (dropout 0) of the reference model in the ``tiny_cheb_f32`` configuration and weights
      (make_golden.py), on that fixture's batch: losses, the parameters of up to MAX_PARAM elements after every step, and for Lion the
      per-step c of the same parameters.

The reference is imported exactly as make_golden.py imports it (sys.path); nothing of it is stored but recorded numbers.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (import_reference, synth_gso, synth_xy, make_args; puts the repository root on sys.path)
from oracle import stgcn_oracle as orc  # noqa: E402

SHAPES = [(5,), (3, 4, 4), (64,), (1,), (257,)]
STEPS, LR, WD = 6, 1e-2, 1e-2
MAX_PARAM = 768          # parameters stored by (b): every tensor of at most this many elements (the fixture stays < 200 KB)


def import_lion():
    mg.import_reference()                       # (checks /root/reference and puts it on sys.path)
    from script import opt                      # noqa: E402  (reference package)
    return opt.Lion


def make_opt(name, params, Lion, lr, wd):
    if name == "nadamw":
        return torch.optim.NAdam(params, lr=lr, weight_decay=wd, decoupled_weight_decay=True)     # main.py:150
    return Lion(params, lr=lr, weight_decay=wd)                                                  # main.py:152


def lion_c(opt, p):
    b1 = opt.param_groups[0]["betas"][0]
    st = opt.state[p]
    m = st["exp_avg"] if "exp_avg" in st else torch.zeros_like(p)
    return (m * b1 + p.grad * (1 - b1)).detach().numpy().copy()      # the reference's own expression (script/opt.py)


def alone(out, Lion):
    g = torch.Generator().manual_seed(2024)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) * (10.0 ** ((k % 3) - 1)) for s in SHAPES] for k in range(STEPS)]
    grads[2][1].zero_()                          # a zero gradient: Lion's sign(0) = 0 in the first steps' c of that tensor
    for i, t in enumerate(init):
        out[f"alone.init.{i}"] = t.numpy().copy()
        out[f"alone.grad.{i}"] = np.stack([grads[k][i].numpy() for k in range(STEPS)])
    out["alone.n"] = np.array(len(SHAPES))
    out["alone.lr"], out["alone.wd"], out["alone.steps"] = np.array(LR), np.array(WD), np.array(STEPS)
    for name in ("nadamw", "lion"):
        ps = [torch.nn.Parameter(t.clone()) for t in init]
        idle = torch.nn.Parameter(torch.ones(3))
        opt = make_opt(name, ps + [idle], Lion, LR, WD)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)        # main.py:156
        rec = {}
        for k in range(STEPS):
            for p, gr in zip(ps, grads[k]):
                p.grad = gr.clone()
            if name == "lion":
                for i, p in enumerate(ps):
                    rec.setdefault(f"c.{i}", []).append(lion_c(opt, p))
            opt.step()
            sched.step()
            for i, p in enumerate(ps):
                rec.setdefault(f"param.{i}", []).append(p.detach().numpy().copy())
                rec.setdefault(f"exp_avg.{i}", []).append(opt.state[p]["exp_avg"].numpy().copy())
                if name == "nadamw":
                    rec.setdefault(f"exp_avg_sq.{i}", []).append(opt.state[p]["exp_avg_sq"].numpy().copy())
            if name == "nadamw":
                rec.setdefault("mu_product", []).append(float(opt.state[ps[0]]["mu_product"]))
            rec.setdefault("lr", []).append(opt.param_groups[0]["lr"])
        assert torch.equal(idle, torch.ones(3))
        for k, v in rec.items():
            out[f"alone.{name}.{k}"] = np.array(v) if k in ("mu_product", "lr") else np.stack(v)


def train(out, models, Lion):
    fx = dict(np.load(os.path.join(HERE, "tiny_cheb_f32.npz")))
    cfg = dict(Kt=3, Ks=3, act="glu", gct="cheb_graph_conv", n_his=12, droprate=0.0, blocks=[[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]])
    seed, B, n = int(fx["seed"]), int(fx["B"]), int(fx["n_vertex"])
    gso = fx["gso"]
    ocfg = orc.OracleConfig(Kt=cfg["Kt"], Ks=cfg["Ks"], n_his=cfg["n_his"], act_func=cfg["act"], graph_conv_type=cfg["gct"],
                            droprate=cfg["droprate"], blocks=cfg["blocks"])
    params = orc.random_params(ocfg, n, seed=seed, dtype=torch.float32)
    s, a = orc.param_checksums(params)
    assert abs(s - fx["param_checksum"][0]) <= 1e-6 * max(1.0, abs(a))          # the tiny_cheb_f32 weights
    xn, yn = mg.synth_xy(B, cfg["n_his"], n, seed + 1)
    x, y = torch.from_numpy(xn).float(), torch.from_numpy(yn).float()
    out["train.steps"], out["train.lr"], out["train.wd"] = np.array(3), np.array(1e-3), np.array(1e-3)
    for name in ("nadamw", "lion"):
        model = models.STGCNChebGraphConv(mg.make_args(cfg, torch.from_numpy(gso)), cfg["blocks"], n)
        model.load_state_dict(params, strict=True)
        model.train()
        opt = make_opt(name, model.parameters(), Lion, 1e-3, 1e-3)
        named = dict(model.named_parameters())
        keep = [k for k, v in model.state_dict().items() if v.numel() <= MAX_PARAM and k in named]
        losses, rec = [], {}
        for _ in range(3):
            opt.zero_grad()
            loss = torch.nn.MSELoss()(model(x).view(len(x), -1), y)      # main.py:166-168
            loss.backward()
            if name == "lion":
                for k in keep:
                    if named[k].grad is not None:
                        rec.setdefault("c." + k, []).append(lion_c(opt, named[k]))
            opt.step()
            losses.append(loss.item())
            for k in keep:
                rec.setdefault("param." + k, []).append(named[k].detach().numpy().copy())
        out[f"train.{name}.losses"] = np.array(losses)
        for k, v in rec.items():
            out[f"train.{name}.{k}"] = np.stack(v)


def main():
    _, models, _ = mg.import_reference()
    Lion = import_lion()
    torch.set_num_threads(1)       # bit-reproducible reductions
    out = {"meta_versions": mg.versions()}
    alone(out, Lion)
    train(out, models, Lion)
    path = os.path.join(HERE, "optim_kinds.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
