#!/usr/bin/env python3
"""What the loss kind costs the captured C2 step (207 nodes, batch size 32, fp32, resident series): train.GraphedTrainStep(loss=...) with
"mse", "mae" and "huber", each in a fresh child process per repeat, ALTERNATING within one session (host clock around replays that end in
a synchronise; the median of three windows of --steps replays per child).  Reported, not judged: the figures of profiles/loss_kinds.md.

  python tools/loss_kind_timing.py [--repeats 3] [--steps 1000]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_HIS, N_PRED, BS, ROWS = 12, 3, 32, 34272
BLOCKS = [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]]
KINDS = ("mse", "mae", "huber")


def child(kind: str, steps: int) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from stgcn_amd import DropoutStream, models
    from stgcn_amd.train import GraphedTrainStep, make_optimizer
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    dev = torch.device("cuda", 0)
    gso_np = np.load(os.path.join(ROOT, "tests", "golden", "gso_real.npz"))["metr_la.cheb_sym_norm_lap"]
    n = gso_np.shape[0]
    rs = np.random.RandomState(0)
    series = torch.from_numpy(rs.standard_normal((int(ROWS * 0.7), n)).astype(np.float32)).to(dev)
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=torch.from_numpy(gso_np).to(dev),
                                 enable_bias=True, droprate=0.5, n_his=N_HIS)
    torch.manual_seed(42)
    model = models.STGCNChebGraphConv(args, BLOCKS, n).to(dev)
    DropoutStream.manual_seed(42)
    opt = make_optimizer(model, capturable=True)
    step = GraphedTrainStep(model, opt, torch.zeros(BS, 1, N_HIS, n, device=dev), torch.zeros(BS, n, device=dev), series=series,
                            n_his=N_HIS, n_pred=N_PRED, loss=kind, huber_delta=1.0)
    assert step.fused and step.fold
    for _ in range(100):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    step.check()
    loss = float(step().item())
    assert loss == loss, "the step produced NaN"
    step.close()
    print(json.dumps({"kind": kind, "ms_per_step": statistics.median(ms), "windows_ms": ms, "loss": loss}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--child", choices=KINDS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps)
    runs = {k: [] for k in KINDS}
    for _ in range(a.repeats):
        for kind in KINDS:      # alternating: every kind sees the same stretch of the session
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps)], cwd=ROOT,
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:      # nothing more is started on the device after a failed run
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"{kind}: child exited with {out.returncode}")
            runs[kind].append(json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"])
            print(kind, round(runs[kind][-1], 5), flush=True)
    print(json.dumps({k: {"ms_per_step": round(statistics.median(v), 5), "runs_ms": [round(x, 5) for x in v]} for k, v in runs.items()}), flush=True)


if __name__ == "__main__":
    main()
