"""CPU: what the indexed UDP receive path's GPU tests stand on.  tests/udp_indexed_np.py (the gather into a strided
twin ring) reproduces udp_np.udp_classify_np on an identity layout and marks out-of-class offsets; the header's
PN_UF_BADOFF is the binding's UF.BADOFF; pn_udp_classify_indexed is declared and exported; EfviUdpRingLayout's
arithmetic (tests/cpp/test_udp_ring_layout, host only) is the reference's."""
import ctypes
import os
import re
import subprocess

import numpy as np

import pollnet_amd as pa

import udp_indexed_np as uin
import udp_np as un

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(un.ip4("239.3.0.%d" % (1 + i % 4)), 40000 + i // 4) for i in range(12)]


def _ring(seed, n, stride, frame_off):
    rng = np.random.default_rng(seed)
    slots = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    room = stride - frame_off - 42
    for i in range(n):
        ip, port = PAIRS[i % len(PAIRS)]
        plen = (0, 1, 17, 54, 55, room, room - 1, 300)[i % 8]
        kw = [{}, {"udp_csum": 0}, {"ulen": 8 + plen + 2}, {"ip_csum": 7}, {"proto": 6}][i % 5]
        un.put_udp_frame(slots[i], frame_off, rng.integers(0, 256, plen, dtype=np.uint8).tobytes(), un.ip4("10.3.3.3"),
                         ip, 1000 + i, port + (i % 7 == 6), **kw)
        if i % 11 == 4:
            slots[i, frame_off + 42] ^= 1
    return slots


def test_identity_layout_reproduces_the_strided_records():
    subs = un.make_subs(PAIRS)
    for frame_off, stride, n in [(2, 2048, 80), (0, 112, 40), (14, 1536, 40), (6, 128, 33)]:
        slots = _ring(stride + frame_off, n, stride, frame_off)
        offsets = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(frame_off)
        avail = stride - frame_off
        for verify in (True, False):
            exp = un.udp_classify_np(slots, stride, frame_off, subs, verify)
            got = uin.udp_classify_indexed_np(slots, offsets, frame_off % 16, avail, subs, verify)
            assert np.array_equal(got, exp), (frame_off, stride, verify)
        fl = exp["flags"]
        assert (fl & un.MATCH).any() and (fl & un.NOCSUM).any() and (fl & un.LEN_BAD).any() and un.deliver(fl).any()
        twin, tstride, in_class = uin.twin_ring(slots, offsets, frame_off % 16, avail)
        assert tstride % 16 == 0 and tstride >= frame_off % 16 + avail and in_class.all()
        assert np.array_equal(twin[:, frame_off % 16:frame_off % 16 + avail], slots[:, frame_off:])


def test_avail_is_the_trunc_rule_and_out_of_class_rows_are_badoff():
    subs = un.make_subs(PAIRS)
    stride, frame_off, n = 256, 2, 24
    slots = _ring(5, n, stride, frame_off)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(frame_off)
    full = uin.udp_classify_indexed_np(slots, offsets[:-1], 2, 254, subs)
    short = uin.udp_classify_indexed_np(slots, offsets[:-1], 2, 100, subs)  # 34 + ulen_even > 100: payloads above 58
    longer = full["payload_len"] > 58
    assert longer.any() and (short["flags"][longer] & un.TRUNC).all()
    assert ((full["flags"][longer] & un.TRUNC) == 0).any()  # the same frames fit the larger avail
    assert np.array_equal(short[~longer & ((full["flags"] & un.LEN_BAD) == 0)],
                          full[~longer & ((full["flags"] & un.LEN_BAD) == 0)])
    stray = offsets[:-1].copy()
    stray[[0, 7, 8]] += np.uint64(4)
    stray[3] = np.uint64(2**40 + 3)  # far outside the buffer: never read
    got = uin.udp_classify_indexed_np(slots, stray, 2, 254, subs)
    bad = np.zeros(n - 1, bool)
    bad[[0, 3, 7, 8]] = True
    assert (got[bad] == uin.badoff_record()).all()
    assert got[0]["flags"] == uin.BADOFF and got[0]["sub_id"] == un.NO_SUB and got[0]["payload_off"] == 0
    assert np.array_equal(got[~bad], full[~bad])


def test_badoff_flag_of_the_header_is_the_bindings():
    src = open(os.path.join(ROOT, "include", "pollnet_amd.h")).read()
    m = re.search(r"#define\s+PN_UF_BADOFF\s+(0x[0-9A-Fa-f]+)u", src)
    assert m, "PN_UF_BADOFF is not defined in include/pollnet_amd.h"
    assert int(m.group(1), 16) == pa.UF.BADOFF == uin.BADOFF == 0x4000
    others = [int(v, 16) for k, v in re.findall(r"#define\s+(PN_UF_\w+)\s+(0x[0-9A-Fa-f]+)u", src) if k != "PN_UF_BADOFF"]
    assert len(others) == 10 and not any(v & 0x4000 for v in others)
    assert sorted(others) == sorted(un.ALL_FLAGS)


def test_indexed_entry_point_is_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "pollnet_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+pn_udp_classify_indexed\s*\(([^)]*)\)", src)
    assert m, "pn_udp_classify_indexed is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "base", "offsets", "eth_mod16", "n", "avail", "results",
                                                         "stream"]
    lib = ctypes.CDLL(pa.LIB_PATH)
    assert hasattr(lib, "pn_udp_classify_indexed")
    assert callable(pa.RxContext.udp_classify_indexed)
    # without a ctx: PN_EINVAL and a message that names the function, nothing else touched
    lib.pn_udp_classify_indexed.restype = ctypes.c_int
    lib.pn_udp_classify_indexed.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 2
    lib.pn_last_error.argtypes = [ctypes.c_void_p]
    lib.pn_last_error.restype = ctypes.c_char_p
    assert lib.pn_udp_classify_indexed(None, None, None, 0, 0, 96, None, None) == -1
    assert b"pn_udp_classify_indexed" in lib.pn_last_error(None)


def test_efvi_udp_ring_layout_arithmetic():
    exe = os.path.join(ROOT, "tests", "cpp", "test_udp_ring_layout")
    assert os.path.exists(exe), "tests/cpp/test_udp_ring_layout not built (make)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "PASS" in p.stdout, p.stdout + p.stderr
