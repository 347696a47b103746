"""CPU: the C-ABI library builds for gfx950, loads without a GPU and exports every symbol that
include/stgcn_hip.h declares (no compute calls here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(stgcn_[a-z0-9_]+)\s*\(", hdr)))


def test_header_lists_expected_entry_points():
    from stgcn_amd import _lib
    assert declared_symbols() == sorted(_lib.EXPORTED_SYMBOLS)


def test_hip_library_builds_loads_and_exports_all_symbols():
    from stgcn_amd import _lib, build
    try:
        path = build.build()
    except RuntimeError as e:          # no hipcc on this machine
        pytest.skip(str(e))
    L = _lib._Lib(path)
    for sym in declared_symbols():
        assert hasattr(L.dll, sym), sym
    hdr = open(os.path.join(ROOT, "include", "stgcn_hip.h")).read()
    abi = int(re.search(r"#define STGCN_ABI_VERSION (\d+)", hdr).group(1))
    assert L.backend == "hip-gfx950" and L.dll.stgcn_version() == abi == _lib.ABI_VERSION


def test_stale_library_is_refused(monkeypatch):
    """A library built from another revision of the header must not be bound (its argument lists differ)."""
    from stgcn_amd import _lib, build
    try:
        path = build.build()
    except RuntimeError as e:
        pytest.skip(str(e))
    monkeypatch.setattr(_lib, "ABI_VERSION", _lib.ABI_VERSION + 1)
    with pytest.raises(_lib.StgcnError, match="ABI revision"):
        _lib._Lib(path)


def test_missing_library_fails_loudly(tmp_path):
    from stgcn_amd import _lib
    with pytest.raises(_lib.StgcnError):
        _lib._Lib(str(tmp_path / "nope.so"))


def test_product_package_never_imports_oracle():
    import ast
    pkg = os.path.join(ROOT, "stgcn_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            tree = ast.parse(open(os.path.join(pkg, fn)).read())
            for node in ast.walk(tree):
                names = []
                if isinstance(node, ast.Import):
                    names = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    names = [node.module or ""]
                assert not any(n.split(".")[0] in ("oracle", "tests") for n in names), f"{fn} imports {names}"


def test_no_kernel_of_the_library_uses_scratch():
    """Register spills cost the fused kernels 30-50 % (a 17-VGPR spill took tc2_ln_fwd from 23 to 35 us): the gfx950 build must not
    contain a kernel with a scratch allocation (hipcc -Rpass-analysis=kernel-resource-usage, device code only)."""
    import subprocess
    import tempfile
    from stgcn_amd import build
    try:
        hipcc = build.find_hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", '-DSTGCN_BACKEND_NAME="hip-gfx950"',
               "-Rpass-analysis=kernel-resource-usage", os.path.join(build.CSRC, "stgcn_capi.hip"), "-o", os.path.join(tmp, "dev.o")]
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
    name, bad = None, []
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and int(m.group(1)) > 0:
            bad.append((name, int(m.group(1))))
    # (no exceptions since round 5: the one kernel that spilled -- the fp32 three-role chained launch of round 4 -- was removed)
    assert not bad, bad
