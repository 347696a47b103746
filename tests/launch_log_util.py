"""Coverage of a CASES table as a checked fact: the launch log (STGCN_LAUNCH_LOG, one line "label@tag <kernel> <workgroups> <threads>" per
launch, flushed line by line) of one run of the table, cut into the byte range each half of each row wrote, shows that every row took the
kernel instance and the workgroup count it is in the table for.  Shared by the fp32 table (tests/test_gpu_block_paths.py, halves "debug"
and "prod") and the bf16 table (tests/test_gpu_bf16_paths.py, halves "clean" and "poisoned").

The log is opened once per process, so a table is logged by ONE child pytest (run_child): under its own time limit, never started again.
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def span_recorder(name, spans_env):
    """on_half(half, "begin" | "end") for the pair runners: appends {"row", "half", "lo", "hi"} (byte range of the launch log) to the file
    os.environ[spans_env] names.  None unless that variable and STGCN_LAUNCH_LOG are set (the plain run of the table)."""
    path, log = os.environ.get(spans_env), os.environ.get("STGCN_LAUNCH_LOG")
    if not path or not log:
        return None
    size = lambda: os.path.getsize(log) if os.path.exists(log) else 0      # (the library flushes every line)
    state = {}

    def on_half(half, edge):
        if edge == "begin":
            state[half] = size()
        else:
            with open(path, "a") as fh:
                fh.write(json.dumps({"row": name, "half": half, "lo": state[half], "hi": size()}) + "\n")
    return on_half


def parse_launch_log(log_bytes, spans):
    """{(row, half): [(label, kernel text, workgroups)]} from the launch log and the byte spans span_recorder wrote."""
    out = {}
    for s in spans:
        rows = []
        for ln in log_bytes[s["lo"]:s["hi"]].decode().splitlines():
            label, kernel, wgs, _threads = ln.split("\t")
            rows.append((label.split("@")[0], kernel, int(wgs)))
        out[(s["row"], s["half"])] = rows
    return out


def read_launches(log_path, spans_path):
    with open(log_path, "rb") as fh:
        log = fh.read()
    with open(spans_path) as fh:
        return parse_launch_log(log, [json.loads(ln) for ln in fh.read().splitlines()])


def check_rows_take_their_branch(launches, cases, halves, key="log"):
    """Every (kernel text, workgroups or None) of row[key] appears in every half of the row."""
    for name, row in cases.items():
        for half in halves:
            got = launches[(name, half)]
            assert got, (name, half)
            for text, wgs in row[key]:
                hit = [g for g in got if text in g[1] and (wgs is None or g[2] == wgs)]
                assert hit, f"row {name} ({half}): no launch of '{text}' with {wgs} workgroups in {got}"


def run_child(env_extra, files, k, timeout=300, marker="gpu"):
    """One child pytest over `files` -k `k` with env_extra set; returns its stdout.  A child that fails, skips, dies or runs out of time
    fails the calling test and is not started again."""
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", *files, "-m", marker, "-x", "-q", "-p", "no:cacheprovider", "-k", k],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    return r.stdout


def passed(stdout):
    m = re.search(r"(\d+) passed", stdout)
    return int(m.group(1)) if m else 0
