"""The C-ABI library loads and exports every symbol include/slender_hip.h declares; the ctypes table mirrors the header.
No compute calls (no GPU here)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slender_hip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|long long|const char\*)\s+(sod_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(3).strip()
        n = 0 if args in ("void", "") else len([a for a in args.split(",") if a.strip()])
        out[m.group(2)] = n
    return out


def test_header_matches_ctypes_table():
    from slenderobjdet_amd import _C

    decl = _declared()
    assert sorted(decl) == _C.exported_symbols()
    for name, n in decl.items():
        assert len(_C._SIGS[name]) == n, f"{name}: header has {n} parameters, ctypes table {len(_C._SIGS[name])}"


def test_library_exports_every_symbol():
    from slenderobjdet_amd import _C

    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _C.load()   # raises if a symbol is missing
    assert lib.sod_version().decode().startswith("slender_hip")
    assert lib.sod_reduce_workspace_bytes() >= 8 * 1024 * 4
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _C.LIB_PATH]).decode()
    for name in _declared():
        assert re.search(rf"\bT {name}\b", syms), name


def test_product_fails_loudly_without_gpu_tensors():
    """No silent CPU fallback: CPU tensors are rejected by the op layer."""
    import torch

    from slenderobjdet_amd import _C
    from slenderobjdet_amd.layers import functional as HF

    with pytest.raises(_C.SlenderHipError):
        HF.conv2d_fwd(torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16), torch.zeros(8, 3, 3, 8, dtype=torch.bfloat16), None, stride=1, pad=1)
    with pytest.raises(_C.SlenderHipError):
        HF.focal_loss_fwd(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32))


def test_product_does_not_import_oracle():
    """oracle/ is test infrastructure: nothing under slenderobjdet_amd/ may import it."""
    for dp, _, files in os.walk(os.path.join(ROOT, "slenderobjdet_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dp, f)


def test_fastdiv_host_model():
    """The multiply-high division used by the conv kernels (csrc/common.h) is exact for n < 2^31."""
    import random

    def make(d):
        if d <= 1:
            return 0, 0
        l = 0
        while (1 << l) < d:
            l += 1
        return (((1 << 32) * ((1 << l) - d)) // d + 1) & 0xFFFFFFFF, l

    random.seed(0)
    for d in list(range(1, 70)) + [84, 100, 168, 1344, 16800, 22400, 2304, 268800, (1 << 20) + 7]:
        mul, shr = make(d)
        for n in [0, 1, d - 1, d, d + 1, 2 * d - 1, (1 << 31) - 1] + [random.randrange(1 << 31) for _ in range(200)]:
            got = n if d == 1 else (((n * mul) >> 32) + n) >> shr
            assert got == n // d, (n, d)


def test_no_kernel_spills_or_uses_scratch(tmp_path):
    """The kernels that pace their LDS-DMA pipelines with counted ``s_waitcnt vmcnt(N)`` (bottleneck_fused.hip, conv_igemm256.hip,
    conv_wgrad256.hip, the ring kernels of conv_igemm.hip and conv_wgrad_ring.hip) derive N from the vector-memory instructions they issue themselves;
    scratch (spill) accesses would join that count - two experimental variants that spilled a few registers computed garbage /
    faulted on the MI355X.  hipcc cross-compiles for gfx950 without a GPU: no kernel of these files may report a spilled register.
    (conv_dispatch.hip, the host side of the convolutions, holds no kernel: like version.hip it has nothing to report.)"""
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "slenderobjdet_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    # ... and no kernel of the WHOLE library may touch scratch memory at all: a dynamically indexed private array (the rotated IoU's point
    # list until round 3: 400 B per lane) costs a trip to memory per access
    files = sorted(f[:-4] for f in os.listdir(src) if f.endswith(".hip"))
    procs = []
    for f in files:
        d = tmp_path / f
        d.mkdir()
        procs.append((f, d, subprocess.Popen([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=off",
                                              "-save-temps=obj", "-c", os.path.join(src, f + ".hip"), "-o", str(d / (f + ".o"))],
                                             cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for f, d, p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, out.decode()[-2000:]
        asm = [x for x in os.listdir(d) if x.endswith("gfx950.s")]
        assert asm, os.listdir(d)
        text = open(d / asm[0]).read()
        spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]      # (SGPR spills go to VGPR lanes, not to memory)
        if not spills and "__global__" not in open(os.path.join(src, f + ".hip")).read():
            continue                                                                     # a file without kernels (version.hip)
        assert spills and max(spills) == 0, (f, spills)
        assert "scratch_" not in text, f
