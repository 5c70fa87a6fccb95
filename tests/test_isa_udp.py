"""Code-generation checks on the UDP receive kernels (CPU only: hipcc cross-compiles udp_kernel.hip to gfx950
assembly, as tests/test_isa.py does for the other kernels): no scratch, at most 128 VGPRs (four waves per SIMD),
and no divergent-descriptor (waterfall) loop around a buffer access -- the subscription probe uses plain
per-lane pointer loads, the record store a wave-uniform descriptor."""
import os
import re

import pytest

from test_isa import HIPCC, _asm, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def _metadata(asm):
    """{kernel symbol: {field: int}} from the listing's amdhsa.kernels metadata."""
    out, cur = {}, None
    for line in asm.split("amdhsa.kernels:", 1)[1].splitlines():
        m = re.match(r"\s+\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "name":
            cur = out.setdefault(m.group(2).strip("'\""), {})
        elif cur is not None and re.fullmatch(r"\d+", m.group(2)):
            cur[m.group(1)] = int(m.group(2))
    return out


def test_udp_kernels_registers_scratch_and_descriptors():
    asm = _asm("udp_kernel.hip")
    ks = {k: b for k, b in _kernels(asm).items() if "udp_classify" in k}
    # eight alignment classes x {verifying, header-only} with the cooperative window, and frame_off = 0's two
    assert len(ks) == 18, sorted(ks)
    meta = _metadata(asm)
    for k, body in ks.items():
        m = meta[k]
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m["vgpr_count"])
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (k, m)
        assert not any(re.match(r"\s+v_cmp_eq_u64_e\d+ vcc, s\[", l) for l in body), f"waterfall loop in {k}"
        assert not any("scratch_" in l for l in body), k
        # the record store and the probe's loads are there in the forms meant
        assert sum("buffer_store_dwordx4" in l for l in body) == 1, k
        assert any("global_load_dwordx2" in l for l in body), k
