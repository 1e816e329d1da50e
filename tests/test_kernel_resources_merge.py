"""Registers and scratch memory of the --merge-readpair kernels, by the probe of tests/test_kernel_resources.py (hipcc cross-compiles
gfx950 without a GPU; `-Rpass-analysis=kernel-resource-usage`): instantiated as csrc/cfr_device.hip launches them, they have no
scratch memory and stay inside the 128 registers of four waves per SIMD."""
import os

import pytest

from test_kernel_resources import HIPCC, probe, violations

# kernel -> (VGPR ceiling, scratch ceiling in bytes per lane)
BUDGET = {
    "k_merge_decide": (128, 0),
    "k_merge_write": (128, 0),
}


def test_merge_kernels_have_no_scratch_and_keep_four_waves_per_simd(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    found = probe(list(BUDGET), str(tmp_path), "probe_merge")
    print("\n".join(f"{k:20s} {found[k][0]:4d} VGPRs {found[k][1]:5d} B scratch {found[k][2]} waves/SIMD" for k in BUDGET if k in found))
    bad = violations(found, BUDGET)
    assert not bad, "\n".join(bad)
