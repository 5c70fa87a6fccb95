"""Code-generation checks on the UDP gather kernels (CPU only: hipcc cross-compiles udp_gather_kernel.hip to gfx950
assembly, as tests/test_isa_udp.py does for the receive kernels), from the kernel metadata alone: the count, the
scan and the copy in its two source-shift classes, no scratch, no spills, at most 128 VGPRs."""
import os

import pytest

from test_isa import HIPCC, _asm, _kernels
from test_isa_udp import _metadata

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def test_udp_gather_kernels_registers_and_scratch():
    asm = _asm("udp_gather_kernel.hip")
    ks = sorted(k for k in _kernels(asm) if "udp_gather" in k)
    # count, scan, and the copy for a payload that starts 0 or 2 bytes into a dword
    assert len(ks) == 4, ks
    assert sum("udp_gather_count_kernel" in k for k in ks) == 1
    assert sum("udp_gather_scan_kernel" in k for k in ks) == 1
    assert sum("udp_gather_copy_kernel" in k for k in ks) == 2
    meta = _metadata(asm)
    for k in ks:
        m = meta[k]
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m["vgpr_count"])
