"""profiles/head_stage_errors.md from the figures tests/test_gpu_head.py measures:

    STGCN_HEAD_REPORT=head_report.jsonl python -m pytest tests/test_gpu_head.py -q -m gpu
    python tools/head_stage_report.py head_report.jsonl > profiles/head_stage_errors.md
"""
import json
import sys

f = lambda v: "%.1e" % v
rows = [json.loads(l) for l in open(sys.argv[1])]
out = ["# Output head: per-case, per-stage errors on the MI355X", "",
       "Measured by `tests/test_gpu_head.py` (harness `tests/head_util.py`, table made by `tools/head_stage_report.py`) against the float64 stage",
       "oracle.  Case letters, shapes and the branch each one reaches: the `CASES` table of `tests/test_gpu_head.py`.",
       "Forward columns are absolute errors (`rstd`: relative), bar 1e-4 (`out`: 5e-5).  Backward columns are max error / max |reference|,",
       "bar 1e-3 (`dx` and whole-tensor parameter gradients: 2e-4).  `grad` / `slice`: the worst of the ten parameter gradients / of the per-tap",
       "(`tc_w[:, :, k]`) and ragged-tail (`ln_w`, `ln_b`) slices, with the key it belongs to.  `oracle32`: the worst of the same gradient and",
       "slice metrics for the stage oracle run in `np.float32` against its float64 run (what rounding alone does; bar for the inputs 2.5e-4).",
       "`kink`: hidden units whose float64 pre-activation is within 1e-4 of zero / of those, units the library put on the other side of ReLU",
       "than the oracle (they take the library's side in the backward reference, of the float32 oracle too, so `oracle32` of a row with such a",
       "unit differs a little from the figure in the `CASES` comment; both counts are bounded by the harness).", "",
       "## fp32", "",
       "| case | U | S | mean | rstd | yln | hd | out | dh1 | dyln | dZ | dx | grad (worst) | slice (worst) | oracle32 (worst) | kink |",
       "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
zero_keys_ok = True
for d in rows:
    if "stored" in d:
        continue
    w = lambda pre: max(((v, k[len(pre):]) for k, v in d.items() if k.startswith(pre)), default=(0.0, "-"))
    g, s, o = w("grad."), w("slice."), w("oracle32.")
    zero_keys_ok &= all(v == 0 for k, v in d.items() if k.startswith(("chain.", "grad_none_ok", "kink.")) or k.endswith("bitwise"))
    loss = (" (loss %s)" % f(d["loss.rel"])) if "loss.rel" in d else ""
    out.append("| %s%s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s `%s` | %s `%s` | %s `%s` | %d / %d |" % (
        d["case"], loss, f(d["fwd.U"]), f(d["fwd.S"]), f(d["fwd.mean"]), f(d["fwd.rstd_rel"]), f(d["fwd.yln"]), f(d["fwd.hd"]), f(d["fwd.out"]),
        f(d["bwd.dh1"]), f(d["bwd.dyln"]), f(d["bwd.dZ"]), f(d["bwd.dx"]) if "bwd.dx" in d else "none", f(g[0]), g[1], f(s[0]), s[1], f(o[0]), o[1],
        d["info.relu_units_within_fwd_tol_of_zero"], d["info.relu_units_on_the_other_side"]))
out += ["", "Every `chain.*`, `kink.*`, `fwd.out_repeat_bitwise` and `grad_none_ok.*` key is 0 on every row." if zero_keys_ok else
        "SOME `chain.*` / `kink.*` / `bitwise` / `grad_none_ok.*` KEY IS NOT 0: see the report file.", "",
        "## bf16 (`tests/bf16_util.py::run_head_case_bf16`, against the bf16 statement of the oracle)", "",
        "Bars: `dx` (stored bf16) relative rms 2^-9 = 2.0e-3 and max 2^-5 = 3.1e-2; fp32 outputs 1e-2 of max.  Cases b, g, h (a backward that is not",
        "dense and has to form `dx`) are refused with `head.tconv_bwd_data: no bf16 variant`; the test asserts the refusal.", "",
        "| case | dx rms | dx max | out | worst gradient |", "|---|---|---|---|---|"]
for d in rows:
    if "stored" not in d:
        continue
    g = max((v, k[len("grad.head."):]) for k, v in d["f32"].items() if k.startswith("grad.head."))
    dx = d["stored"].get("head.dx")
    out.append("| %s | %s | %s | %s | %s `%s` |" % (d["case"], f(dx["rms"]) if dx else "none", f(dx["max"]) if dx else "none",
                                                   f(d["f32"]["head.out"]), f(g[0]), g[1]))
print("\n".join(out))
