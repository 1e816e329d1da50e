"""Registers and scratch memory of the inflater's kernel (csrc/cfr_inflate.hip) and of the id gather (csrc/cfr_tokenize.hip), from the
remarks hipcc prints when it cross-compiles the files for gfx950 (`-Rpass-analysis=kernel-resource-usage`, as
tests/test_kernel_resources_gz.py does for the compressor's): no lane keeps an array, so no scratch.  k_bgzf_inflate is one wave per
workgroup with 5.5 KiB of LDS, so its registers decide how many workgroups share a CU: at most 128 (4 waves per SIMD, 16 workgroups
per CU), the ceiling of the one-wave-per-workgroup compressor.  The gather stays at 64 registers.  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "centrifuger_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# file -> kernel -> (VGPR ceiling, scratch ceiling in bytes per lane)
BUDGET = {"cfr_inflate.hip": {"k_bgzf_inflate": (128, 0)}, "cfr_tokenize.hip": {"k_tok_id_len": (64, 0), "k_tok_ids": (64, 0)}}


@pytest.mark.parametrize("source", list(BUDGET))
def test_inflate_kernels_have_no_scratch_and_stay_inside_their_registers(source):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    budget = BUDGET[source]
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", "-o", "/dev/null",
                        os.path.join(CSRC, source), "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    found, cur = {}, None
    for line in r.stderr.decode().splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = next((k for k in budget if re.search(r"\d" + k + "E", m.group(2))), None)
            if cur:
                found[cur] = [None, None]
        elif cur:
            found[cur][0 if m.group(1) == "VGPRs" else 1] = int(m.group(2))
    print("\n".join(f"{k:22s} {v[0]:4d} VGPRs {v[1]:4d} B scratch" for k, v in found.items()))
    assert set(found) == set(budget)
    bad = [f"{k}: {found[k][0]} VGPRs (<= {v}), {found[k][1]} bytes of scratch (<= {s})" for k, (v, s) in budget.items() if found[k][0] > v or found[k][1] > s]
    assert not bad, "\n".join(bad)
