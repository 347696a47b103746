#!/usr/bin/env python3
"""What scoring a split costs at the C2 shape (207 nodes, batch size 32) on the demo's validation split (34 272 synthetic rows -> 5 140
validation rows -> 5 125 windows, 161 batches), in ONE process, alternating after warm-up, host clock around work that ends in a
synchronise:

  (a) host   data.evaluate_model + data.evaluate_metric, the reference's loop (a gather, eager launches and a host sync per batch, twice)
  (b) pass   one train.GraphedEvalPass.run() (161 hipGraph replays, one synchronise, all four metrics)
  (c) step   ms per replay of train.GraphedTrainStep on the same model (the pass's launches are a subset of the step's + one kernel)

Writes profiles/eval_pass_c2.json (ms per pass, ms per batch, spread = max - min over the repeats) and prints it.

  python tools/eval_pass_timing.py [--passes 20] [--out profiles/eval_pass_c2.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_HIS, N_PRED, BS = 12, 3, 32
BLOCKS = [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]]


def summary(ms, batches):
    return {"ms_per_pass": round(statistics.median(ms), 4), "ms_per_batch": round(statistics.median(ms) / batches, 5),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--rows", type=int, default=34272)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_pass_c2.json"))
    a = ap.parse_args()

    from train_demo import synthetic_speeds
    from stgcn_amd import DropoutStream, data, models
    from stgcn_amd.train import GraphedEvalPass, GraphedTrainStep, make_optimizer

    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    dev = torch.device("cuda", 0)
    gso_np = np.load(os.path.join(ROOT, "tests", "golden", "gso_real.npz"))["metr_la.cheb_sym_norm_lap"]
    n = gso_np.shape[0]
    vel = synthetic_speeds(a.rows, n)
    len_train, len_val, _ = data.split_lengths(a.rows)
    zs = data.ZScore()
    train = zs.fit_transform(vel[:len_train])
    val = zs.transform(vel[len_train:len_train + len_val])
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=torch.from_numpy(gso_np).to(dev),
                                 enable_bias=True, droprate=0.5, n_his=N_HIS)
    torch.manual_seed(42)
    model = models.STGCNChebGraphConv(args, BLOCKS, n).to(dev)
    DropoutStream.manual_seed(42)
    opt = make_optimizer(model, capturable=True)
    ev = GraphedEvalPass(model, val, N_HIS, N_PRED, BS, scaler=zs)
    assert ev.graph is not None, "the evaluation pass was not captured"
    model.train()
    series = torch.from_numpy(train.astype(np.float32)).to(dev)
    step = GraphedTrainStep(model, opt, torch.zeros(BS, 1, N_HIS, n, device=dev), torch.zeros(BS, n, device=dev), series=series,
                            n_his=N_HIS, n_pred=N_PRED)
    sampler = data.WindowSampler(val, N_HIS, N_PRED, dev)
    mse = torch.nn.MSELoss()
    batches = ev.batches

    def host():
        l = data.evaluate_model(model, mse, sampler.batches(BS))
        return (l,) + tuple(data.evaluate_metric(model, sampler.batches(BS), zs))

    def steps():
        model.train()
        for _ in range(batches):
            step()
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for fn in (host, ev.run, steps):      # warm-up of all three
        fn()
    t_host, t_pass, t_step = [], [], []
    m_host = m_pass = None
    for _ in range(a.passes):
        t, m_pass = timed(ev.run)
        t_pass.append(t)
        t, m_host = timed(host)
        t_host.append(t)
        t, _ = timed(steps)
        t_step.append(t)
    step.check()
    res = {"shape": {"nodes": n, "batch_size": BS, "val_rows": int(len_val), "windows": ev.num, "batches": batches},
           "host_loop": summary(t_host, batches), "graphed_pass": summary(t_pass, batches),
           "train_step": {"ms_per_step": round(statistics.median(t_step) / batches, 5), "spread_ms_per_step": round((max(t_step) - min(t_step)) / batches, 5)},
           "metrics_host": [float(v) for v in m_host], "metrics_pass": m_pass}
    res["speedup"] = round(res["host_loop"]["ms_per_pass"] / res["graphed_pass"]["ms_per_pass"], 2)
    res["pass_beats_host_by_more_than_its_spread"] = bool(res["host_loop"]["ms_per_pass"] - res["graphed_pass"]["ms_per_pass"] > res["host_loop"]["spread_ms"])
    res["batch_cheaper_than_step"] = bool(res["graphed_pass"]["ms_per_batch"] < res["train_step"]["ms_per_step"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    ev.close()
    step.close()


if __name__ == "__main__":
    main()
