#!/usr/bin/env python3
"""What the window table of a shuffled epoch costs the captured C2 step (207 nodes, batch size 32, fp32), and whether the default path
kept its speed.  Four forms of train.GraphedTrainStep(series=...), each in a fresh child process per repeat, ALTERNATING within one session
(host clock around replays that end in a synchronise; the median of three windows of --steps replays per child):

  parent_index    index mode on a checkout of the parent commit (--parent-tree, library built there)
  index           index mode on this tree
  table_identity  shuffle=True with set_order(arange): the table path on the addresses of index mode
  table_shuffled  shuffle=True, a drawn permutation: the table path without the row sharing of consecutive windows

Writes profiles/shuffled_step_c2.json: median and spread (max - min over the repeats) of ms per step for each form, and the condition
"index mode is not slower than the parent by more than the parent's own spread".  The cost of the table is reported, not judged.

  git worktree add ab_base HEAD~1 && (cd ab_base && python -m stgcn_amd.build --force)
  python tools/shuffle_step_timing.py [--parent-tree ab_base] [--repeats 5] [--steps 1000]
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
FORMS = ("parent_index", "index", "table_identity", "table_shuffled")


def child(form: str, tree: str, steps: int) -> None:
    """One measurement with the package of ``tree``; prints one JSON line."""
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from stgcn_amd import DropoutStream, models
    from stgcn_amd.train import GraphedTrainStep, make_optimizer
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    dev = torch.device("cuda", 0)
    gso_np = np.load(os.path.join(ROOT, "tests", "golden", "gso_real.npz"))["metr_la.cheb_sym_norm_lap"]
    n = gso_np.shape[0]
    rs = np.random.RandomState(0)
    series = torch.from_numpy(rs.standard_normal((int(ROWS * 0.7), n)).astype(np.float32)).to(dev)      # the demo's training split, z-scored
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=torch.from_numpy(gso_np).to(dev),
                                 enable_bias=True, droprate=0.5, n_his=N_HIS)
    torch.manual_seed(42)
    model = models.STGCNChebGraphConv(args, BLOCKS, n).to(dev)
    DropoutStream.manual_seed(42)
    opt = make_optimizer(model, capturable=True)
    kw = dict(shuffle=True, shuffle_seed=1) if form.startswith("table") else {}
    step = GraphedTrainStep(model, opt, torch.zeros(BS, 1, N_HIS, n, device=dev), torch.zeros(BS, n, device=dev), series=series,
                            n_his=N_HIS, n_pred=N_PRED, **kw)
    assert step.fold, "the pack launch should carry the batch position"
    if form == "table_identity":
        step.set_order(torch.arange(step.order.numel(), dtype=torch.int64))
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
    print(json.dumps({"form": form, "ms_per_step": statistics.median(ms), "windows_ms": ms, "loss": loss}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=os.path.join(ROOT, "ab_base"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shuffled_step_c2.json"))
    ap.add_argument("--child", choices=FORMS)
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tree, a.steps)
    if a.repeats < 5:
        ap.error("at least five repeats per form")
    if not os.path.exists(os.path.join(a.parent_tree, "stgcn_amd", "libstgcn_hip.so")):
        ap.error(f"{a.parent_tree}: no built checkout of the parent commit (see the header comment)")
    runs = {f: [] for f in FORMS}
    for _ in range(a.repeats):
        for form in FORMS:      # alternating: every form sees the same stretch of the session
            tree = a.parent_tree if form == "parent_index" else ROOT
            env = dict(os.environ)
            env.pop("STGCN_AMD_LIB", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, "--tree", tree, "--steps", str(a.steps)],
                                 env=env, cwd=tree, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:      # nothing more is started on the device after a failed run
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"{form}: child exited with {out.returncode}")
            runs[form].append(json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"])
            print(form, round(runs[form][-1], 5), flush=True)
    res = {"shape": {"nodes": 207, "batch_size": BS, "dtype": "fp32", "steps_per_window": a.steps, "repeats": a.repeats}}
    for f in FORMS:
        v = runs[f]
        res[f] = {"ms_per_step": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
                  "spread_ms": round(max(v) - min(v), 5), "runs_ms": [round(x, 5) for x in v]}
    d = res["index"]["ms_per_step"] - res["parent_index"]["ms_per_step"]
    res["index_minus_parent_ms"] = round(d, 5)
    res["index_not_slower_than_parent_by_more_than_its_spread"] = bool(d <= res["parent_index"]["spread_ms"])
    res["table_identity_cost_ms"] = round(res["table_identity"]["ms_per_step"] - res["index"]["ms_per_step"], 5)
    res["table_shuffled_cost_ms"] = round(res["table_shuffled"]["ms_per_step"] - res["index"]["ms_per_step"], 5)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
