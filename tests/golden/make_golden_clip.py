#!/usr/bin/env python3
"""Generate the gradient-clipping fixture (optim_clip.npz): seeded tensors, a gradient sequence that crosses the clip threshold, and the
run of the REFERENCE's Lion behind ``torch.nn.utils.clip_grad_norm_`` on them.

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_clip.py

Setup as part (a) of make_golden_optim.py: a handful of seeded fp32 tensors (one more never gets a gradient), 6 steps,
StepLR(step_size=3, gamma=0.5).  The seeded normal gradients are scaled per step by 4, 4, 1/4, 1/4, 4, 1/4 and ``max_norm`` is the norm
of the UNSCALED first gradient: steps 1, 2 and 5 clip, steps 3, 4 and 6 do not, and every step's norm is at least 2 x away from the
threshold (asserted here).  AdamW and NAdam need no recorded run -- the tests run ``clip_grad_norm_`` + ``torch.optim`` inline on these
inputs; Lion exists in the reference only (script/opt.py), so its parameters, ``exp_avg``, update direction c, and torch's norm of every
step are recorded.  Nothing of the reference is stored but recorded numbers.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_optim as mo  # noqa: E402

SHAPES = [(5,), (3, 4, 4), (64,), (1,), (257,)]
SCALES = [4.0, 4.0, 0.25, 0.25, 4.0, 0.25]
STEPS, LR, WD = 6, 1e-2, 1e-2


def main():
    Lion = mo.import_lion()
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(2025)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    base = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(STEPS)]
    max_norm = float(torch.sqrt(sum((t.double() ** 2).sum() for t in base[0])))
    grads = [[t * SCALES[k] for t in base[k]] for k in range(STEPS)]
    out = {"meta_versions": mg.versions(), "n": np.array(len(SHAPES)), "steps": np.array(STEPS), "lr": np.array(LR), "wd": np.array(WD),
           "max_norm": np.array(max_norm), "scales": np.array(SCALES)}
    for i, t in enumerate(init):
        out[f"init.{i}"] = t.numpy().copy()
        out[f"grad.{i}"] = np.stack([grads[k][i].numpy() for k in range(STEPS)])
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    idle = torch.nn.Parameter(torch.ones(3))
    opt = Lion(ps + [idle], lr=LR, weight_decay=WD)                                  # main.py:152
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)            # main.py:156
    rec = {}
    for k in range(STEPS):
        for p, gr in zip(ps, grads[k]):
            p.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_([p for p in ps + [idle] if p.grad is not None], max_norm)
        ratio = float(total) / max_norm
        assert ratio >= 2.0 or ratio <= 0.5, (k, ratio)
        rec.setdefault("norm", []).append(float(total))
        for i, p in enumerate(ps):
            rec.setdefault(f"c.{i}", []).append(mo.lion_c(opt, p))
        opt.step()
        sched.step()
        for i, p in enumerate(ps):
            rec.setdefault(f"param.{i}", []).append(p.detach().numpy().copy())
            rec.setdefault(f"exp_avg.{i}", []).append(opt.state[p]["exp_avg"].numpy().copy())
    assert torch.equal(idle, torch.ones(3))
    for k, v in rec.items():
        out[f"lion.{k}"] = np.array(v, dtype=np.float32) if k == "norm" else np.stack(v)
    path = os.path.join(HERE, "optim_clip.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
