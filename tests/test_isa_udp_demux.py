"""Code-generation checks on the UDP demux kernels (CPU only: hipcc cross-compiles udp_demux_kernel.hip to gfx950
assembly, as tests/test_isa_udp_gather.py does for the gather), from the kernel metadata alone: the eight launches'
kernels (the copy in its two source-shift classes) and no other, nothing of the gather's in the translation unit, no
scratch, no spills, at most 128 VGPRs, and LDS at or below what DESIGN §18 states."""
import os
import re

import pytest

from test_isa import HIPCC, _asm, _kernels
from test_isa_udp import _metadata

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

# one 4-byte entry per possible subscription in count and place (16 KiB), the scans' per-wave partials
LDS_MAX = {
    "udp_demux_count_kernel": 16384,
    "udp_demux_cols_kernel": 0,
    "udp_demux_subs_kernel": 64,
    "udp_demux_place_kernel": 16384,
    "udp_demux_sum_kernel": 0,
    "udp_demux_scan_kernel": 128,
    "udp_demux_copy_kernel": 0,
    "udp_demux_subbytes_kernel": 0,
}


def _lds(asm):
    """{kernel symbol: group_segment_fixed_size}: within a kernel's entry the metadata's fields are in alphabetical
    order, so the size stands before the kernel's own .name (four spaces deep; an argument's .name is deeper)."""
    out, size = {}, None
    for line in asm.split("amdhsa.kernels:", 1)[1].splitlines():
        m = re.match(r"    \.(group_segment_fixed_size|name):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "name":
            out[m.group(2).strip("'\"")] = size
            size = None
        else:
            size = int(m.group(2))
    return out


def test_udp_demux_kernels_registers_scratch_and_lds():
    asm = _asm("udp_demux_kernel.hip")
    ks = sorted(_kernels(asm))
    assert not [k for k in ks if "udp_gather" in k], ks
    assert all("udp_demux_" in k for k in ks), ks
    assert len(ks) == 9, ks
    for name in LDS_MAX:
        assert sum(name in k for k in ks) == (2 if name == "udp_demux_copy_kernel" else 1), (name, ks)
    meta, lds_of = _metadata(asm), _lds(asm)
    for k in ks:
        m = meta[k]
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m["vgpr_count"])
        lds = next(v for name, v in LDS_MAX.items() if name in k)
        assert lds_of[k] is not None and lds_of[k] <= lds, (k, lds_of[k])
        print(k, m["vgpr_count"], m.get("sgpr_count"), lds_of[k])
