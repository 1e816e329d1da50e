"""Registers and scratch memory of the compressor's kernels (csrc/cfr_gz.hip), from the remarks hipcc prints when it cross-compiles the
file for gfx950 (`-Rpass-analysis=kernel-resource-usage`, as tests/test_kernel_resources_tsv.py does for the formatter's): no lane keeps
an array, so no scratch.  The record and pack kernels stay at 64 registers (8 waves per SIMD); k_gz_deflate is one wave per workgroup
with 17.25 KiB of LDS, which allows 9 workgroups per CU whatever its registers are: at most 128 (4 waves per SIMD).  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "centrifuger_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# kernel -> (VGPR ceiling, scratch ceiling in bytes per lane)
BUDGET = {"k_dump_len": (64, 0), "k_dump_write": (64, 0), "k_gz_deflate": (128, 0), "k_gz_pack": (64, 0)}


def test_gz_kernels_have_no_scratch_and_stay_inside_their_registers():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", "-o", "/dev/null",
                        os.path.join(CSRC, "cfr_gz.hip"), "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    found, cur = {}, None
    for line in r.stderr.decode().splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = next((k for k in BUDGET if k in m.group(2)), None)
            if cur:
                found[cur] = [None, None]
        elif cur:
            found[cur][0 if m.group(1) == "VGPRs" else 1] = int(m.group(2))
    print("\n".join(f"{k:22s} {v[0]:4d} VGPRs {v[1]:4d} B scratch" for k, v in found.items()))
    assert set(found) == set(BUDGET)
    bad = [f"{k}: {found[k][0]} VGPRs (<= {v}), {found[k][1]} bytes of scratch (<= {s})" for k, (v, s) in BUDGET.items() if found[k][0] > v or found[k][1] > s]
    assert not bad, "\n".join(bad)
