"""profiles/block_stage_errors.md from the figures tests/test_gpu_block_paths.py measures:

    STGCN_BLOCK_REPORT=block_report.jsonl python -m pytest tests/test_gpu_block_paths.py -q -m gpu
    python tools/block_stage_report.py block_report.jsonl > profiles/block_stage_errors.md

and profiles/block_hook_errors.md from those of tests/test_gpu_block_hooks.py (the oracle32.hook.* columns from the emulator run of the
same table, tests/test_emu_block_hooks.py, which measures them on the CPU):

    STGCN_BLOCK_REPORT=hooks_gpu.jsonl python -m pytest tests/test_gpu_block_hooks.py -q -m gpu -k test_block_hooks
    STGCN_BLOCK_REPORT=hooks_cpu.jsonl python -m pytest tests/test_emu_block_hooks.py -q -k test_block_hooks_on_the_emulator
    python tools/block_stage_report.py --hooks hooks_gpu.jsonl hooks_cpu.jsonl > profiles/block_hook_errors.md
"""
import json
import sys

f = lambda v: "%.1e" % v


def hook_report(gpu_path, cpu_path):
    from tests.block_util import bar
    gpu = [json.loads(l) for l in open(gpu_path)]
    cpu = {json.loads(l)["case"].replace(" emu", ""): json.loads(l) for l in open(cpu_path)} if cpu_path else {}
    out = ["# LayerNorm hook epilogues of fp32 blocks: per-row errors on the MI355X", "",
           "Measured by `tests/test_gpu_block_hooks.py` (harness `tests/block_util.py`, consumer mode; table made by",
           "`tools/block_stage_report.py --hooks`).  Row names, the pair P -> Q of each row and the branch it reaches: the `CASES` table of that",
           "file.  `debug` / `prod`: the two launch sequences, as in `profiles/block_stage_errors.md`.  `worst`: the key that comes closest to",
           "its bar (value / bar; keys with bar 0 are all 0 unless listed under the table), with its value.  `rowstat g` / `gx`: the row partials",
           "Q wrote against the float64 sums, max error / max |ref| (bar 1e-3); `vs own pass`: against the partials P's own",
           "`ln_bwd_rowstats_kernel` writes for the same dy (bar 1e-3); `NaN`: partials the backward left unwritten; `dy bits`: elements of Q's input",
           "gradient that differ from Q run without a hook; `launches`: |observed - expected| `ln_bwd_rowstats` launches (bars 0).  `oracle32 g / gx`:",
           "the same sums formed in `np.float32` the way the kernels form them, measured on the CPU (`tests/test_emu_block_hooks.py`; the rows",
           "`big` and `many` are measured in the GPU run, at their full size), bar 2.5e-4.", "",
           "| row | worst | rowstat g | rowstat gx | vs own pass g / gx | NaN | dy bits | launches | bitwise | oracle32 g / gx |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    nonzero = []
    for d in gpu:
        for half, pre in (("debug", ""), ("prod", "prod.")):
            e = {k[len(pre):]: v for k, v in d.items() if k != "case" and (k.startswith("prod.") == bool(pre))}
            ratios = [(v / bar(k), k, v) for k, v in e.items() if 0 < bar(k) < float("inf") and not k.startswith("oracle32.")]
            _, wk, wv = max(ratios)
            nonzero += [(d["case"], half, k, v) for k, v in e.items() if bar(k) == 0 and v != 0]
            o = cpu.get(d["case"]) if (d["case"] in cpu and "big" != d["case"] and "many" != d["case"]) else d
            out.append("| %s %s | `%s` %s | %s | %s | %s / %s | %d | %d | %d | %s | %s |" % (
                d["case"], half, wk, f(wv), f(e["hook.rowstat_g"]), f(e["hook.rowstat_gx"]), f(e["hook.rowstat_vs_own_pass_g"]),
                f(e["hook.rowstat_vs_own_pass_gx"]), e["hook.rowstat_nan"], e["hook.dy_bitwise_vs_unhooked"], e["grad_none_ok.hook_launches"],
                ("%d" % d["prod.bitwise_vs_debug"]) if pre else "",
                "" if pre else "%s / %s" % (f(o["oracle32.hook.rowstat_g"]), f(o["oracle32.hook.rowstat_gx"]))))
    out += ["", "Every key with bar 0 is 0 on every row." if not nonzero else "KEYS WITH BAR 0 THAT ARE NOT 0: %s" % nonzero]
    print("\n".join(out))


if sys.argv[1] == "--hooks":
    sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
    hook_report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    sys.exit(0)
rows = [json.loads(l) for l in open(sys.argv[1])]
out = ["# ST block: per-row, per-stage errors on the MI355X", "",
       "Measured by `tests/test_gpu_block_paths.py` (harness `tests/block_util.py`, table made by `tools/block_stage_report.py`) against the",
       "float64 stage oracle.  Row names, shapes and the branch each one reaches: the `CASES` table of `tests/test_gpu_block_paths.py`.",
       "Every row has two lines: `debug` is the launch sequence of the stage tests (`stgcn_set_debug_stages`: `ln_gate_bwd` and",
       "`align_gate_bwd` launched in front of the fused kernels), `prod` the sequence of a training step, run with the partial-sum arena",
       "filled with NaN between forward and backward.  Forward columns are absolute errors, bar 1e-4.  Backward columns are max error /",
       "max |reference|, bar 1e-3; `-` = the stage stays on chip in that sequence.  `grad` / `slice`: the worst whole-tensor parameter",
       "gradient / the worst per-tap (`tc1_w`, `tc2_w`), per-term (`gc_w`), ragged-tail (`ln_w`, `ln_b`) and edge-step (`dx.t0`, `dx.tlast`)",
       "slice, with the key it belongs to.  `oracle32`: the worst of the same metrics for the stage oracle run in `np.float32` against its",
       "float64 run (what rounding alone does; bar for the inputs 2.5e-4).  `kink`: graph-conv outputs whose float64 pre-activation is",
       "within 1e-4 of zero / of those, units the library put on the other side of ReLU than the oracle.  `bitwise`: elements of y, dx and",
       "all parameter gradients that differ between the two sequences (bar 0); `NaN`: NaN elements among them in the production run.", "",
       "| row | G | y | y tail | dZ2 | dYg | dA | dZ1 | dx | grad (worst) | slice (worst) | oracle32 (worst) | kink | bitwise | NaN |",
       "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
zero_keys_ok = True
for d in rows:
    for half, pre in (("debug", ""), ("prod", "prod.")):
        e = {k[len(pre):]: v for k, v in d.items() if k != "case" and (k.startswith("prod.") == bool(pre))}
        w = lambda p: max(((v, k[len(p):]) for k, v in e.items() if k.startswith(p) and k != "slice.y.tail"), default=(0.0, "-"))
        g, s = w("grad."), w("slice.")
        o = max(((v, k[len("oracle32."):]) for k, v in d.items() if k.startswith("oracle32.")), default=(0.0, "-"))
        zero_keys_ok &= all(v == 0 for k, v in e.items() if k.startswith(("grad_none_ok", "kink.")) or k.endswith("bitwise"))
        c = lambda k: f(e[k]) if k in e else "-"
        out.append("| %s %s | %s | %s | %s | %s | %s | %s | %s | %s | %s `%s` | %s `%s` | %s | %d / %d | %s | %s |" % (
            d["case"], half, c("fwd.G"), c("fwd.y"), c("slice.y.tail"), c("bwd.dZ2"), c("bwd.dYg"), c("bwd.dA"), c("bwd.dZ1"), c("bwd.dx"),
            f(g[0]), g[1], f(s[0]), s[1], ("%s `%s`" % (f(o[0]), o[1])) if not pre else "", e["info.relu_units_within_fwd_tol_of_zero"],
            e["info.relu_units_on_the_other_side"], ("%d" % d["prod.bitwise_vs_debug"]) if pre else "", ("%d" % d["prod.nan_elements"]) if pre else ""))
out += ["", "Every `kink.*`, `fwd.y_repeat_bitwise` and `grad_none_ok.*` key (the chain words among them) is 0 on every row." if zero_keys_ok else
        "SOME `kink.*` / `bitwise` / `grad_none_ok.*` KEY IS NOT 0: see the report file."]
print("\n".join(out))
