"""profiles/bf16_block_stage_errors.md from the figures tests/test_gpu_bf16_paths.py measures:

    STGCN_BF16_PATHS_REPORT=bf16_report.jsonl python -m pytest tests/test_gpu_bf16_paths.py -q -m gpu -k test_bf16_block_paths
    python tools/bf16_stage_report.py bf16_report.jsonl > profiles/bf16_block_stage_errors.md

Further files on the command line (e.g. the report of a single row run on its own) are appended as sections of their own:
    python tools/bf16_stage_report.py bf16_report.jsonl "title=lead_report.jsonl"
"""
import json
import sys

f = lambda v: "%.1e" % v


def table(rows):
    out = ["| row | G | y | y tail | dYg | dA | dx | grad (worst) | slice (worst) | min slice ratio | ReLU flips | mean / mean over std | clean vs poisoned bits | NaN |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    zero_ok = True
    for d in rows:
        e, s = d["f32"], d["stored"]
        c = lambda k: ("%s / %s" % (f(s[k]["rms"]), f(s[k]["max"]))) if k in s else "-"
        w = lambda p: max(((v, k[len(p):]) for k, v in e.items() if k.startswith(p)), default=(0.0, "-"))
        g, sl = w("grad."), w("slice.")
        ratio = min(((v, k[len("info.slice_ratio."):]) for k, v in e.items() if k.startswith("info.slice_ratio.")), default=(0.0, "-"))
        zero_ok &= all(v == 0 for k, v in e.items() if "grad_none_ok" in k or k.endswith("bitwise"))
        out.append("| %s | %s | %s | %s | %s | %s | %s | %s `%s` | %s `%s` | %.2f `%s` | %s | %s / %s | %s | %s |" % (
            d["case"], c("fwd.G"), c("fwd.y"), c("slice.y.tail"), c("bwd.dYg"), c("bwd.dA"), c("bwd.dx"), f(g[0]), g[1], f(sl[0]), sl[1],
            ratio[0], ratio[1], f(e["relu_flip_rate"]), f(e["fwd.mean"]), f(e["fwd.mean_over_std"]),
            ("%d" % e["prod.bitwise_clean_vs_poisoned"]) if "prod.bitwise_clean_vs_poisoned" in e else "-",
            ("%d" % e["prod.nan_elements"]) if "prod.nan_elements" in e else "-"))
    out += ["", "Every `fwd.y_repeat_bitwise` and `grad_none_ok.*` key (the chain words among them) is 0 on every row." if zero_ok else
            "SOME `bitwise` / `grad_none_ok.*` KEY IS NOT 0: see the report file."]
    return out


def main(argv):
    rows = [json.loads(l) for l in open(argv[1])]
    out = ["# bf16 ST block: per-row, per-stage errors on the MI355X", "",
           "Measured by `tests/test_gpu_bf16_paths.py` (harness `tests/bf16_util.py`, table made by `tools/bf16_stage_report.py`) against the bf16",
           "statement of the stage oracle, backward teacher-forced on the library's own saved tensors.  Row names, shapes and the branch each one",
           "reaches: the `CASES` table of `tests/test_gpu_bf16_paths.py`.  Every row runs twice with a shared oracle, the partial-sum arena clean and",
           "then filled with NaN between forward and backward; the line shows the poisoned run.  Stored bf16 tensors: relative rms error / max error",
           "over max |reference| (bars 2^-9 = 2.0e-3 / 2^-5 = 3.1e-2); `y tail`: the same over the last ragged 16-node tile.  `grad` / `slice`: the worst",
           "whole-tensor parameter gradient / the worst per-tap (`tc1_w`, `tc2_w`), per-term (`gc_w`) and ragged-tail (`ln_w`, `ln_b`) slice, max error over",
           "that slice's own max (bar 1e-2), with the key it belongs to; the stored slices `dx.t0`, `dx.tlast` pass the stored bars wherever `dx` is listed.",
           "`min slice ratio`: the smallest max |slice| / max |whole tensor| of the oracle on the row's inputs (condition: >= 0.25).  `ReLU flips`: share of",
           "graph-conv outputs on the other side of zero than the oracle's (bar 2e-3).  `mean / mean over std`: worst LayerNorm slab mean error over",
           "max |mean| + 1e-3 / in units of the slab's standard deviation (bars 1e-3; rows with fewer than 4 slabs are held to the second only).",
           "`clean vs poisoned bits`: elements of y, dx and all parameter gradients that differ between the two runs (bar 0); `NaN`: NaN elements among them.", ""]
    out += table(rows)
    for extra in argv[2:]:
        title, path = extra.split("=", 1)
        rows = [json.loads(l) for l in open(path)]
        out += ["", "## " + title, ""] + table(rows)
        for d in rows:
            e, s = d["f32"], d["stored"]
            out += ["", "`%s`: `fwd.mean` %s, `fwd.mean_over_std` %s, `fwd.rstd` %s; oracle max |mean| %s, min 1 / rstd %s; mismatch rates %s." % (
                d["case"], f(e["fwd.mean"]), f(e["fwd.mean_over_std"]), f(e["fwd.rstd"]), f(e["info.ref_abs_mean_max"]), f(e["info.ref_std_min"]),
                ", ".join("`%s` %s" % (k, f(v["mismatch"])) for k, v in s.items() if k.startswith("fwd.") and not k.endswith("fp64")))]
            if e["fwd.mean_over_std"] <= 1e-3 < e["fwd.mean"]:
                out += ["`fwd.mean` is over its 1e-3 bar and `fwd.mean_over_std` far inside the same bar: conditioning, not a defect.  The row's single slab",
                        "has a mean close to zero beside its standard deviation, and `fwd.mean` divides by that mean; the stored tensors in front of the",
                        "LayerNorm differ from the oracle at the usual rounding-boundary rates.  The row does not enter the table with this seed."]
    print("\n".join(out))


if __name__ == "__main__":
    main(sys.argv)
