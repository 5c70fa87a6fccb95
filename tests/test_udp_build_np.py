"""Pins tests/udp_build_np.py (the ring pn_udp_build must leave, written from the header's contract) before any GPU
test trusts it: mode EFVI against the reference's own update_udp_pkt, modes PLAIN and CSUM through the receive
side's model (tests/udp_np.py), the checksum that computes to 0, and the new entry points' declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

import pollnet_amd as pa
from oracle import pyoracle as orc

import udp_build_np as ub
import udp_np as un
from test_tx import craft_udp_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _templates(seed, n_ch, defect_every=8):
    """n_ch header templates as test_tx's _ref_efvi_datagrams builds its headers: random MACs, addresses, ports and
    header words, and every 8th on the header whose cached sum's first fold carries.  The four fields
    every build overwrites hold garbage."""
    rng = np.random.default_rng(seed)
    need = 0x1FFFF - 0x11C5
    out, defect = [], []
    for i in range(n_ch):
        e = np.zeros(42, np.uint8)
        e[0:12] = rng.integers(0, 256, 12)
        e[12:14] = (0x08, 0x00)
        if i % defect_every == 0:
            e[14:34] = np.frombuffer(craft_udp_header([0xFFFF, need - 0xFFFF], [0, 0], 0), np.uint8)
        else:
            e[14:34] = rng.integers(0, 256, 20)
            e[14], e[23] = 0x45, 17
        e[34:42] = rng.integers(0, 256, 8)
        e[16:18] = rng.integers(0, 256, 2)
        e[24:26] = rng.integers(0, 256, 2)
        w = e[14:34].copy()
        w[2:4] = 0
        w[10:12] = 0
        c = int(w.view("<u2").astype(np.int64).sum())
        defect.append((c >> 16) + (c & 0xFFFF) >= 0x10000)
        out.append(bytes(e))
    return out, np.array(defect)


def _batch(seed, n, n_ch, room, pay_bytes=1 << 16):
    rng = np.random.default_rng(seed)
    pay = rng.integers(0, 256, pay_bytes, dtype=np.uint8)
    lens = rng.integers(0, room + 1, n).astype(np.uint16)
    lens[:4] = (0, 1, room - 1, room)
    offs = np.array([rng.integers(0, pay_bytes - int(l) + 1) for l in lens], np.uint64)
    chans = rng.integers(0, n_ch, n).astype(np.uint32)
    return pay, offs, lens, chans


def test_efvi_mode_equals_the_references_update_udp_pkt():
    ref = orc.ref_core()
    if ref is None:
        pytest.skip("oracle/_ref/libref_core.so not built (needs /root/reference)")
    stride, n, n_ch = 2048, 400, 64
    for frame_off in (8, 2):
        tmpl, defect = _templates(0xE0 + frame_off, n_ch)
        assert defect.sum() >= n_ch // 8
        room = stride - frame_off - 42
        pay, offs, lens, chans = _batch(frame_off, n, n_ch, room)
        ring = np.random.default_rng(1).integers(0, 256, n * stride, dtype=np.uint8)
        got, flens = ub.udp_build_np(ring, stride, frame_off, ub.make_channels(tmpl), pay, len(pay), offs, lens, chans,
                                     ub.UB_EFVI)
        assert (flens == 42 + lens.astype(np.int64)).all()
        assert defect[chans].sum() >= n // 16
        for i in range(n):
            ln, off = int(lens[i]), int(offs[i])
            t = bytearray(tmpl[chans[i]])
            t[40:42] = b"\0\0"  # init_udp_pkt's udp checksum, which update_udp_pkt never touches (Efvi.h:643)
            buf = np.frombuffer(bytes(t) + bytes(pay[off:off + ln]), np.uint8).copy()
            ref.ref_efvi_udp_datagram(buf.ctypes.data, ln)
            at = i * stride + frame_off
            assert bytes(got[at:at + 42 + ln]) == bytes(buf), i
            # nothing else of the slot changed
            assert (got[i * stride:at] == ring[i * stride:at]).all()
            assert (got[at + 42 + ln:(i + 1) * stride] == ring[at + 42 + ln:(i + 1) * stride]).all()


def _dest_templates(n_ch):
    """Distinct (group, port) destinations; returns (templates, pairs)."""
    pairs = [(un.ip4("239.%d.%d.%d" % (1 + i // 4096, (i // 16) % 256, 1 + i % 16)), 20000 + i % 977) for i in range(n_ch)]
    tmpl = [ub.make_template(bytes([2, 0, 0, 0, 0, 1 + i % 7]), bytes([1, 0, 0x5E, p[0][1] & 0x7F, p[0][2], p[0][3]]),
                             un.ip4("10.1.%d.%d" % (i % 200, 1 + i % 250)), p[0], 30000 + i % 1000, p[1])
            for i, p in enumerate(pairs)]
    return tmpl, pairs


@pytest.mark.parametrize("mode", [ub.UB_PLAIN, ub.UB_CSUM])
def test_plain_and_csum_frames_come_back_through_the_receive_model(mode):
    stride, frame_off, n, n_ch = 2048, 8, 300, 64
    tmpl, pairs = _dest_templates(n_ch)
    subs = un.make_subs(pairs)
    room = stride - frame_off - 42
    pay, offs, lens, chans = _batch(77 + mode, n, n_ch, room)
    ring = np.random.default_rng(2).integers(0, 256, n * stride, dtype=np.uint8)
    got, flens = ub.udp_build_np(ring, stride, frame_off, ub.make_channels(tmpl), pay, len(pay), offs, lens, chans, mode)
    rec = un.udp_classify_np(got, stride, frame_off, subs)
    want = un.MATCH | un.IP_OK | (un.NOCSUM if mode == ub.UB_PLAIN else un.UDP_OK)
    assert (flens != 0).all()
    assert (rec["flags"] == want).all(), np.flatnonzero(rec["flags"] != want)[:8]
    assert (rec["sub_id"] == chans).all()
    assert (rec["payload_len"] == lens).all()
    for i in (0, 1, 2, 3, 17, n - 1):
        at = i * stride + frame_off + 42
        assert bytes(got[at:at + int(lens[i])]) == bytes(pay[int(offs[i]):int(offs[i]) + int(lens[i])])


@pytest.mark.parametrize("length", [64, 65])
def test_a_checksum_that_computes_to_zero_is_sent_as_ffff(length):
    """One message per parity of len whose RFC 768 sum is 0xFFFF before the complement: payload word 0 is fixed up
    to the complement of everything else's sum."""
    tmpl, _ = _dest_templates(1)
    rng = np.random.default_rng(length)
    p = bytearray(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
    p[0:2] = b"\0\0"
    f = ub.build_frame(tmpl[0], bytes(p), ub.UB_CSUM)
    rest = int.from_bytes(f[40:42], "big")  # ~sum of everything else (0xFFFF only if that sum is 0, which it is not)
    assert rest != 0xFFFF
    p[0:2] = rest.to_bytes(2, "big")  # sum becomes S + ~S = 0xFFFF, the checksum computes to 0
    ring = np.full(256, 0x5A, np.uint8)
    got, flens = ub.udp_build_np(ring, 256, 2, ub.make_channels(tmpl), np.frombuffer(bytes(p), np.uint8), length,
                                 np.array([0], np.uint64), np.array([length], np.uint16), None, ub.UB_CSUM)
    assert int(flens[0]) == 42 + length
    assert bytes(got[2 + 40:2 + 42]) == b"\xff\xff"
    rec = un.udp_classify_np(got, 256, 2, un.make_subs([_dest_templates(1)[1][0]]))
    assert rec["flags"][0] == un.MATCH | un.IP_OK | un.UDP_OK


def test_refusal_rules():
    r = ub.refused
    assert not r(2048 - 8 - 42, 0, 0, 2048, 8, 1, 4096) and r(2048 - 8 - 42 + 1, 0, 0, 2048, 8, 1, 4096)
    assert r(10, 1, 0, 2048, 8, 1, 4096) and not r(10, 0, 4086, 2048, 8, 1, 4096) and r(10, 0, 4087, 2048, 8, 1, 4096)
    assert not r(0, 0, 4096, 2048, 8, 1, 4096) and r(1, 0, 4096, 2048, 8, 1, 4096) and r(0, 0, 4097, 2048, 8, 1, 4096)
    assert r(5, 0, (1 << 64) - 2, 2048, 8, 1, 4096)  # no 64-bit wrap
    assert not r(65493, 0, 0, 65536, 0, 1, 1 << 20) and r(65494, 0, 0, 65536, 0, 1, 1 << 20)  # frame_lens is 16 bits


def test_constants_and_layout_equal_the_header():
    hdr = open(os.path.join(ROOT, "include", "pollnet_amd.h")).read()
    for name, val in (("PN_UB_EFVI", ub.UB_EFVI), ("PN_UB_PLAIN", ub.UB_PLAIN), ("PN_UB_CSUM", ub.UB_CSUM),
                      ("PN_UDP_MAX_CHANNELS", 4096)):
        m = re.search(r"#define %s\s+(\d+)u" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(pa, name), name
    assert pa.UDP_CHANNEL_DTYPE == ub.UDP_CHANNEL_DTYPE and pa.UDP_CHANNEL_DTYPE.itemsize == 48
    assert pa.UDP_CHANNEL_DTYPE.fields["_pad"][1] == 42
    assert re.search(r"#define PN_ABI_VERSION 1\b", hdr)


def test_new_symbols_are_declared_and_exported():
    from test_abi import declared_functions, exported_functions

    new = {"pn_udp_set_channels", "pn_udp_build"}
    assert new <= set(declared_functions()) and new <= set(exported_functions(pa.LIB_PATH))
    lib = ctypes.CDLL(pa.LIB_PATH)
    lib.pn_udp_build.restype = ctypes.c_int
    lib.pn_udp_set_channels.restype = ctypes.c_int
    lib.pn_last_error.restype = ctypes.c_char_p
    lib.pn_last_error.argtypes = [ctypes.c_void_p]
    assert lib.pn_udp_set_channels(None, None, 0) == -1 and b"pn_udp_set_channels" in lib.pn_last_error(None)
    assert hasattr(pa.RxContext, "udp_set_channels") and hasattr(pa.RxContext, "udp_build")


def test_template_is_init_udp_pkts():
    """make_template against Efvi's init_udp_pkt fields written out by hand (Efvi.h:597-644)."""
    t = ub.make_template(bytes([0, 0x0F, 0x53, 1, 2, 3]), bytes([1, 0, 0x5E, 1, 2, 3]), un.ip4("10.0.0.1"),
                         un.ip4("239.1.2.3"), 1000, 2000)
    assert t.hex() == ("01005e010203" "000f53010203" "0800" "4500" "0000" "0000" "4000" "4011" "0000" "0a000001"
                       "ef010203" "03e8" "07d0" "0008" "0000")
