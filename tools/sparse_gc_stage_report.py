#!/usr/bin/env python3
"""profiles/sparse_gc_stage_errors.md from the JSON lines tests/test_gpu_sparse_gc.py::test_bf16_activations_track_the_dense_tiled_bf16_path
appends to $STGCN_SPARSE_REPORT: rms error against the float64 stage oracle, relative to the oracle's rms, of the sparse path and of the
dense tiled bf16 path on the same case.

    STGCN_SPARSE_REPORT=/tmp/sparse.jsonl python -m pytest tests/test_gpu_sparse_gc.py -q -m gpu -k bf16
    python tools/sparse_gc_stage_report.py /tmp/sparse.jsonl > profiles/sparse_gc_stage_errors.md"""
import json
import sys


def main(path):
    print("bf16 activations: rms(got - float64 oracle) / rms(oracle) per tensor; the test holds sparse <= 1.25 x dense.\n")
    for line in open(path):
        r = json.loads(line)
        print(f"### {r['case']}\n\n| tensor | sparse (CSR, L in fp32) | dense tiled (L in bf16) | sparse / dense |\n|---|---|---|---|")
        for k, v in r["sparse"].items():
            d = r["dense"][k]
            print(f"| {k} | {v:.3e} | {d:.3e} | {v / d if d else float('nan'):.3f} |")
        print()


if __name__ == "__main__":
    main(sys.argv[1])
