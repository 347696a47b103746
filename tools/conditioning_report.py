#!/usr/bin/env python3
"""profiles/conditioning_errors.md from the JSON lines tests/test_emu_conditioning.py and tests/test_gpu_conditioning.py append to
$STGCN_COND_REPORT (one line per run: row, condition, product form, launch mode, backend, every key's error beside its oracle32 twin).

    STGCN_COND_REPORT=/tmp/emu.jsonl python -m pytest tests/test_emu_conditioning.py -q
    STGCN_COND_REPORT=/tmp/gpu.jsonl python -m pytest tests/test_gpu_conditioning.py -q -m gpu
    python tools/conditioning_report.py /tmp/emu.jsonl /tmp/gpu.jsonl [--before /tmp/emu_before.jsonl] > profiles/conditioning_errors.md

--before: emulator lines of an earlier library (the column "emulator, before"): how the tanh_f defect read under this criterion.
Per (row, product form, launch mode) and backend: the worst ratio err / max(oracle32 err, floor / R) over all conditions and keys, the
condition and key that set it, and the largest error over its bar (<= 1 passes)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import conditioning_util as cu      # noqa: E402

META = ("row", "condition", "x6", "mode", "backend")


def load(path):
    with open(path) as fh:
        return [json.loads(ln) for ln in fh if ln.strip()]


def summarise(lines):
    """{(row, x6, mode): (worst ratio, condition, key, worst err / bar, its condition, its key, runs)}"""
    out = {}
    for ln in lines:
        err = {k: v for k, v in ln.items() if k not in META}
        ratio, key = cu.worst_ratio(err)
        over = max(((v / cu.effective_bar(k, err), k) for k, v in err.items() if not k.startswith("oracle32.") and cu.is_measured(k)), default=(0.0, None))
        g = (ln["row"], ln["x6"], ln["mode"])
        cur = out.get(g, (0.0, None, None, 0.0, None, None, 0))
        if ratio > cur[0]:
            cur = (ratio, ln["condition"], key) + cur[3:]
        if over[0] > cur[3]:
            cur = cur[:3] + (over[0], ln["condition"], over[1]) + cur[6:]
        out[g] = cur[:6] + (cur[6] + 1,)
    return out


def cell(s):
    return "-" if s is None else f"{s[0]:.1f} ({s[1]}, {s[2]}); {s[3]:.2f} of bar ({s[4]}, {s[5]})"


def main():
    args = sys.argv[1:]
    before = []
    if "--before" in args:
        i = args.index("--before")
        before = load(args[i + 1])
        del args[i:i + 2]
    lines = [ln for p in args for ln in load(p)]
    emu = summarise([ln for ln in lines if ln["backend"] == "emu"])
    gpu = summarise([ln for ln in lines if ln["backend"] == "gpu"])
    old = summarise(before)
    print("| row | product form | launches | runs (emu / gpu) | emulator | MI355X | emulator, before |")
    print("|---|---|---|---|---|---|---|")
    for g in sorted(set(emu) | set(gpu)):
        n = f"{emu[g][6] if g in emu else 0} / {gpu[g][6] if g in gpu else 0}"
        print(f"| {g[0]} | {'bf16x6' if g[1] == 'default' else 'fp32 MFMA'} | {g[2]} | {n} | {cell(emu.get(g))} | {cell(gpu.get(g))} | {cell(old.get(g))} |")
    # the same by condition, over all rows: worst ratio (row / product form, key)
    print()
    print("| condition | emulator | MI355X |")
    print("|---|---|---|")
    by = {}
    for ln in lines:
        err = {k: v for k, v in ln.items() if k not in META}
        ratio, key = cu.worst_ratio(err)
        cur = by.setdefault(ln["condition"], {}).get(ln["backend"], (0.0, None, None))
        if ratio > cur[0]:
            by[ln["condition"]][ln["backend"]] = (ratio, ln["row"] + ("" if ln["x6"] == "default" else " fp32 MFMA"), key)
    fmt = lambda c: "-" if c is None else f"{c[0]:.1f} ({c[1]}, {c[2]})"
    for cond in list(cu.CONDITIONS) + list(cu.BIG_ONLY):
        if cond in by:
            print(f"| {cond} | {fmt(by[cond].get('emu'))} | {fmt(by[cond].get('gpu'))} |")


if __name__ == "__main__":
    main()
