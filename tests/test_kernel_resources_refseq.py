"""Registers and scratch memory of the kernels of the reference-text front end (csrc/cfr_refseq.hip), from the remarks hipcc prints when
it cross-compiles the file for gfx950 (`-Rpass-analysis=kernel-resource-usage`, as tests/test_kernel_resources_inflate.py does for the
inflater's): no lane keeps an array, so no scratch.  The kernels are 256 lanes wide and carry masks and counters only: 64 registers
let eight waves share a SIMD, the ceiling of the tokeniser's gathers.  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "centrifuger_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# file -> kernel -> (VGPR ceiling, scratch ceiling in bytes per lane)
BUDGET = {"cfr_refseq.hip": {"k_ref_maps": (64, 0), "k_ref_mark": (64, 0), "k_ref_compact": (64, 0), "k_ref_records": (64, 0), "k_ref_assemble": (64, 0),
                             "k_ref_unpack": (64, 0), "k_pack_text": (64, 0)}}


@pytest.mark.parametrize("source", list(BUDGET))
def test_refseq_kernels_have_no_scratch_and_stay_inside_their_registers(source):
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
