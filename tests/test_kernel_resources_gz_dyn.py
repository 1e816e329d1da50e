"""Registers, scratch memory and LDS of the kernel of the compressor's dynamic mode (k_gzd_* in csrc/cfr_gz.hip), from the remarks hipcc
prints when it cross-compiles the file for gfx950 (`-Rpass-analysis=kernel-resource-usage`, as tests/test_kernel_resources_gz.py does
for the other four, which must still be there with their budgets): no lane keeps an array, so no scratch; at most 128 VGPRs (4 waves
per SIMD); at most 32 KiB of LDS - the hash table, the CRC table, histograms, code tables and lengths, the code build's workspace and
the staging of pass B - which leaves five workgroups per CU.  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_kernel_resources_gz import BUDGET, CSRC, HIPCC

MAX_VGPRS, MAX_SCRATCH, MAX_LDS = 128, 0, 32 * 1024


def test_dynamic_kernels_have_no_scratch_128_registers_and_32_kib_of_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", "-o", "/dev/null",
                        os.path.join(CSRC, "cfr_gz.hip"), "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    found, cur = {}, None
    for line in r.stderr.decode().splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = m.group(2)
            found[cur] = {}
        elif cur:
            found[cur][m.group(1).split()[0]] = int(m.group(2))
    new = {k: v for k, v in found.items() if "k_gzd_" in k}
    old = {name: [v for k, v in found.items() if name in k] for name in BUDGET}
    print("\n".join(f"{k}: {v}" for k, v in new.items()))
    assert new, "no k_gzd_ kernel in cfr_gz.hip"
    for k, v in new.items():
        assert not any(name in k for name in BUDGET), f"{k} would be taken for one of the fixed-mode kernels"
        assert v["VGPRs"] <= MAX_VGPRS and v["ScratchSize"] <= MAX_SCRATCH and v["LDS"] <= MAX_LDS, (k, v)
    for name, (vgprs, scratch) in BUDGET.items():
        assert len(old[name]) == 1, f"{name}: found {len(old[name])} times"
        assert old[name][0]["VGPRs"] <= vgprs and old[name][0]["ScratchSize"] <= scratch, (name, old[name][0])
