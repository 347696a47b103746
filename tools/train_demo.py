#!/usr/bin/env python3
"""End-to-end run of the reference's main.py flow on the MI355X path with a synthetic METR-LA-shaped dataset
(34 272 rows x 207 sensors, v = clip(55 + 10 sin(2 pi t / 288 + phi_n) + N(0, 3^2), 0, 80); the real
vel.csv is not available offline): 70/15/15 split (main.py:108-114), z-score fitted on the training rows (main.py:116-119),
12 -> n_pred windows (script/dataloader.py:32-47), STGCNChebGraphConv on the real METR-LA operator, MSE + AdamW (or --opt nadamw | lion)(1e-3, 1e-3)
with StepLR(10, 0.95) per epoch (main.py:147-156), unshuffled minibatches of 32 (main.py:126-131; --shuffle: a fresh permutation of the
windows every epoch, drawn on the host and read through the step's device table), validation loss per epoch
(script/utility.py:90-101), test MAE / RMSE / WMAPE at the end (script/utility.py:103-121).

The training loop is `GraphedTrainStep(series=...)`: the z-scored (time, N) training series stays resident on the GPU and the
captured step windows it in place.  Validation and test scoring are `GraphedEvalPass`es (built once, before the training step, and
replayed every epoch): the metrics are summed on the device, `eval_s` beside `epoch_s` is the wall time of the validation pass.
One JSON line per epoch and one for the test metrics; a persistence forecast
(y_hat = last observed value) on the same windows is printed beside them for scale.

  python tools/train_demo.py [--epochs 3] [--n-pred 3] [--rows 34272] [--opt adamw | nadamw | lion] [--shuffle]
                             [--loss mse | mae | huber] [--huber-delta 1.0] [--missing FRAC] [--null-val V]

--missing FRAC zeroes a seeded random share of the synthetic readings (failed detectors report 0); --null-val V masks the readings equal
to V (and NaN) in training and in both evaluation passes (masked loss and metrics; the JSON rows gain "mape" and "observed").
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_HIS, KT, KS, BS = 12, 3, 3, 32
BLOCKS = [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]]


def synthetic_speeds(rows, n):
    rng = np.random.default_rng(0)
    phi = rng.uniform(0, 2 * np.pi, n)
    t = np.arange(rows)[:, None]
    return np.clip(55 + 10 * np.sin(2 * np.pi * t / 288 + phi[None, :]) + rng.normal(0, 3, (rows, n)), 0, 80)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--n-pred", type=int, default=3)
    ap.add_argument("--rows", type=int, default=34272)
    ap.add_argument("--opt", choices=("adamw", "nadamw", "lion"), default="adamw")     # main.py:59
    ap.add_argument("--shuffle", action="store_true", help="shuffled epochs: step.reshuffle() once per epoch")
    ap.add_argument("--loss", choices=("mse", "mae", "huber"), default="mse",
                    help="the loss the step trains on (nn.MSELoss / L1Loss / HuberLoss); val_loss stays the validation pass's MSE")
    ap.add_argument("--huber-delta", type=float, default=1.0)
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="clip the gradient by its global norm inside the captured step (clip_grad_norm_ + step); the log gains grad_norm / clip_coef")
    ap.add_argument("--missing", type=float, default=0.0,
                    help="zero out this share of the synthetic readings (seeded), as failed detectors do; 0 = the plain series")
    ap.add_argument("--null-val", type=float, default=None,
                    help="train and score on observed readings only: readings equal to this value (and NaN) are masked; nan = NaN-coded")
    a = ap.parse_args()

    from stgcn_amd import DropoutStream, data, models
    from stgcn_amd.train import GraphedEvalPass, GraphedTrainStep, make_optimizer

    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    dev = torch.device("cuda", 0)
    gso_np = np.load(os.path.join(ROOT, "tests", "golden", "gso_real.npz"))["metr_la.cheb_sym_norm_lap"]
    n = gso_np.shape[0]
    vel = synthetic_speeds(a.rows, n)
    if a.missing > 0:
        vel[np.random.default_rng(1).uniform(size=vel.shape) < a.missing] = 0.0
    ok = None if a.null_val is None else data.observed_mask(vel, a.null_val)      # from the raw readings, before the z-score
    len_train, len_val, len_test = data.split_lengths(a.rows)
    zs = data.ZScore()
    train = zs.fit_transform(vel[:len_train])
    val, test = zs.transform(vel[len_train:len_train + len_val]), zs.transform(vel[len_train + len_val:])

    args = types.SimpleNamespace(Kt=KT, Ks=KS, act_func="glu", graph_conv_type="cheb_graph_conv", gso=torch.from_numpy(gso_np).to(dev),
                                 enable_bias=True, droprate=0.5, n_his=N_HIS)
    torch.manual_seed(42)
    model = models.STGCNChebGraphConv(args, BLOCKS, n).to(dev)
    DropoutStream.manual_seed(42)
    opt = make_optimizer(model, lr=1e-3, weight_decay=1e-3, name=a.opt, capturable=True, max_grad_norm=a.max_grad_norm)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.95)

    series = torch.from_numpy(train.astype(np.float32)).to(dev)
    x0 = torch.zeros(BS, 1, N_HIS, n, device=dev)
    y0 = torch.zeros(BS, n, device=dev)
    # the evaluation passes first: their graphs keep the workspaces they captured, and the training step's constructor may still grow them
    ok_train = ok_val = ok_test = None
    if ok is not None:
        ok_train, ok_val, ok_test = ok[:len_train], ok[len_train:len_train + len_val], ok[len_train + len_val:]
    # (masked: the validation pass gets the scaler too, so that its MAPE is in the data's units; val_loss, the z-scored MSE, does not depend on it)
    val_pass = GraphedEvalPass(model, val, N_HIS, a.n_pred, BS, scaler=zs if ok is not None else None, valid=ok_val)
    test_pass = GraphedEvalPass(model, test, N_HIS, a.n_pred, BS, scaler=zs, valid=ok_test)
    model.train()
    step = GraphedTrainStep(model, opt, x0, y0, series=series, n_his=N_HIS, n_pred=a.n_pred, shuffle=a.shuffle, shuffle_seed=42,
                            loss=a.loss, huber_delta=a.huber_delta, valid=None if ok is None else torch.from_numpy(ok_train).to(dev))
    windows = series.shape[0] - N_HIS - a.n_pred + 1
    steps_per_epoch = windows // BS
    first_epoch_steps = steps_per_epoch
    if a.shuffle:
        # one epoch = one walk through the table, so that reshuffle() falls on the wrap of the position: the constructor's own steps
        # already took the head of the first permutation, the first epoch runs what is left of it
        steps_per_epoch = step.order.numel() // BS
        first_epoch_steps = steps_per_epoch - (int(step.index.item()) // BS + 1)
    test_s = data.WindowSampler(test, N_HIS, a.n_pred, dev)

    for epoch in range(a.epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = torch.zeros((), device=dev)
        n_steps = first_epoch_steps if epoch == 0 else steps_per_epoch
        for _ in range(n_steps):
            acc += step()                       # loss stays on the device: no per-step host sync (main.py:170 does .item())
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        step.check()                            # (once per epoch, where the loss is read: names the operator if an in-launch wait gave up)
        sched.step()
        if a.shuffle:
            step.reshuffle()                    # the next epoch's permutation, written into the table the graph already reads
        opt.sync_lr()                           # the captured AdamW reads its learning rate from device memory
        t0 = time.perf_counter()
        vm = val_pass.run()                     # one synchronise per pass (script/utility.py:90-101 on the device)
        val_loss = vm["mse"]
        eval_s = time.perf_counter() - t0
        row = {"epoch": epoch + 1, "train_loss": round(float(acc.item()) / n_steps, 6), "val_loss": round(val_loss, 6),
               "lr": opt.param_groups[0]["lr"], "steps": n_steps, "epoch_s": round(el, 3), "eval_s": round(eval_s, 3),
               "train_windows_per_s": round(n_steps * BS / el, 1)}
        if ok is not None:
            row.update(mape=round(vm["mape"], 6), observed=vm["elements"])
        if a.max_grad_norm is not None:         # of the epoch's last step (device words of the clip state)
            row.update(grad_norm=round(float(opt.last_grad_norm.item()), 6), clip_coef=round(float(opt.last_clip_coef.item()), 6))
        print(json.dumps(row), flush=True)

    m = test_pass.run()
    mae, rmse, wmape = m["mae"], m["rmse"], m["wmape"]
    # persistence forecast on the same test windows, in the original units
    ys, ps = [], []
    for x, y in test_s.batches(BS):
        ys.append(zs.inverse_transform(y.cpu().numpy()).reshape(-1))
        ps.append(zs.inverse_transform(x[:, 0, -1, :].cpu().numpy()).reshape(-1))
    test_row = {"MAE": round(mae, 4), "RMSE": round(rmse, 4), "WMAPE": round(wmape, 6)}
    if ok is None:
        p_mae, p_rmse, p_wmape = data.metrics_from_arrays(np.concatenate(ys), np.concatenate(ps))
    else:                                       # the persistence forecast on the same observed labels
        shift = N_HIS + a.n_pred - 1
        p_mae, p_rmse, p_wmape, _ = data.masked_metrics_from_arrays(np.concatenate(ys), np.concatenate(ps), ok_test[shift:shift + len(test_s)])
        test_row.update(mape=round(m["mape"], 6), observed=m["elements"])
    print(json.dumps({"test": test_row,
                      "persistence_forecast": {"MAE": round(p_mae, 4), "RMSE": round(p_rmse, 4), "WMAPE": round(p_wmape, 6)},
                      "test_windows": len(test_s), "n_pred": a.n_pred, "data": "synthetic METR-LA-shaped speeds, real METR-LA graph"}), flush=True)


if __name__ == "__main__":
    main()
