"""Code-generation checks on the indexed UDP receive kernels (CPU only: hipcc cross-compiles
udp_indexed_kernel.hip to gfx950 assembly, as tests/test_isa_udp.py does for the strided ones), from the kernel
metadata alone: no scratch, at most 128 VGPRs (four waves per SIMD), no spills, and the instantiations meant."""
import os
import re

import pytest

from test_isa import HIPCC, _asm
from test_isa_udp import _metadata

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def test_udp_indexed_kernels_registers_and_scratch():
    meta = {k: m for k, m in _metadata(_asm("udp_indexed_kernel.hip")).items() if "udp_indexed_kernel" in k}
    # eight alignment classes x {verifying, header-only}; the cooperative window is chosen per wave, not per launch
    assert len(meta) == 16, sorted(meta)
    inst = sorted((int(m.group(1)), int(m.group(2))) for m in
                  (re.search(r"udp_indexed_kernelILi(\d+)ELb([01])E", k) for k in meta))
    assert inst == [(mis, ho) for mis in range(0, 16, 2) for ho in (0, 1)], inst
    assert not any("udp_classify" in k for k in _metadata(_asm("udp_indexed_kernel.hip"))), "a strided kernel in this unit"
    for k, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m["vgpr_count"])
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (k, m)
