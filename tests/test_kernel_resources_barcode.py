"""Registers and scratch memory of the barcode whitelist's kernels (csrc/cfr_barcode.hip), from the remarks hipcc prints when it
cross-compiles the file for gfx950 (`-Rpass-analysis=kernel-resource-usage`, as tests/test_kernel_resources_quant.py does): every kernel
waits on random 16-byte fetches from the table, so each must stay far inside the 64 registers of eight waves per SIMD and use no scratch.
The first cross-compile gave 12 (k_bc_build), 14 (k_bc_count, k_bc_lookup) and 36 (k_bc_correct) registers; the budgets below are those
figures with a few registers of room for a compiler update (24 and 40: still eight waves per SIMD), so that a kernel that starts to
keep arrays in registers is noticed.  k_bc_correct holds its block's misses in 4104 bytes of LDS.  No GPU."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "centrifuger_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# kernel -> (VGPR ceiling, scratch ceiling in bytes per lane); all of them 8 waves per SIMD
BUDGET = {"k_bc_build": (24, 0), "k_bc_count": (24, 0), "k_bc_lookup": (24, 0), "k_bc_correct": (40, 0)}
LDS_CEILING = 8192   # bytes per block of 256 lanes: eight such blocks fit a CU's LDS several times over


def test_barcode_kernels_have_no_scratch_and_keep_eight_waves_per_simd():
    assert os.path.exists(HIPCC), "hipcc is part of the build environment"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", "-o", "/dev/null",
                        os.path.join(CSRC, "cfr_barcode.hip"), "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    found, cur = {}, None
    for line in r.stderr.decode().splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = next((k for k in BUDGET if k in m.group(2)), None)
            if cur:
                found[cur] = [None, None, None]
        elif cur:
            found[cur][{"VGPRs": 0, "ScratchSize [bytes/lane]": 1, "LDS Size [bytes/block]": 2}[m.group(1)]] = int(m.group(2))
    print("\n".join(f"{k:14s} {v[0]:4d} VGPRs {v[1]:4d} B scratch {v[2]:6d} B LDS" for k, v in found.items()))
    assert set(found) == set(BUDGET)
    bad = [f"{k}: {found[k][0]} VGPRs (<= {v}), {found[k][1]} bytes of scratch (<= {s}), {found[k][2]} bytes of LDS (<= {LDS_CEILING})"
           for k, (v, s) in BUDGET.items() if found[k][0] > v or found[k][1] > s or found[k][2] > LDS_CEILING]
    assert not bad, "\n".join(bad)
