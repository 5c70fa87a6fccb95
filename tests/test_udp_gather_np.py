"""tests/udp_gather_np.py pinned before any GPU test trusts it (CPU only): one case worked out by hand, the round
trip through the build and classify models (messages -> udp_build_np -> udp_classify_np -> udp_gather_np gives the
messages back), forged records, and the capacity rule.  And the surface: RxContext has the two methods and the
library exports the two entry points."""
import ctypes

import numpy as np
import pytest

import pollnet_amd as pa

import udp_build_np as ub
import udp_gather_np as ug
import udp_np as un
from test_udp_build_np import _dest_templates

DELIVER_OK = un.MATCH | un.IP_OK | un.UDP_OK


def _canaries(n, pay_bytes, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 256, pay_bytes, dtype=np.uint8), rng.integers(1, 1 << 62, n).astype(np.uint64),
            rng.integers(1, 1 << 16, n).astype(np.uint16), rng.integers(1, 1 << 32, n).astype(np.uint32),
            rng.integers(1, 1 << 32, n).astype(np.uint32))


def _rec(sub, plen, flags, poff=42):
    r = np.zeros(1, un.UDP_RESULT_DTYPE)
    r[0] = (sub, 0x0100000A, 0x1234, poff, plen, flags)
    return r[0]


def test_the_surface_exists():
    """Fails before the gather path: no such method, no such export."""
    assert hasattr(pa.RxContext, "udp_gather") and hasattr(pa.RxContext, "udp_gather_indexed")
    lib = ctypes.CDLL(pa.LIB_PATH)
    assert hasattr(lib, "pn_udp_gather") and hasattr(lib, "pn_udp_gather_indexed")
    assert pa.UDP_GATHER_TOTAL_DTYPE == ug.UDP_GATHER_TOTAL_DTYPE and pa.UDP_GATHER_TOTAL_DTYPE.itemsize == 16
    assert pa.PN_UDP_GATHER_ALIGN == ug.ALIGN == 16


def test_five_frames_three_taken_by_hand():
    """Slots of 128 B, frame_off 2.  Frames 0, 2 and 4 are taken with 0, 1 and 17 payload bytes; frame 1 is not UDP,
    frame 3 matched but its IPv4 checksum failed.  By hand: message 0 is empty at offset 0 and takes no room; message
    1 is one byte at offset 0, padded to 16; message 2 is 17 bytes at offset 16, padded to 32; 48 bytes in all."""
    stride, frame_off, n = 128, 2, 5
    ring = np.full(n * stride, 0xEE, np.uint8)  # non-zero after every datagram: the pad must not be a copy
    ring[2 * stride + frame_off + 42] = 0xA1
    ring[4 * stride + frame_off + 42:4 * stride + frame_off + 42 + 17] = np.arange(0xB0, 0xB0 + 17)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    rec[0] = _rec(7, 0, DELIVER_OK)
    rec[1] = _rec(un.NO_SUB, 50, un.IP_OK | un.NOT_UDP)
    rec[2] = _rec(3, 1, un.MATCH | un.IP_OK | un.NOCSUM)
    rec[3] = _rec(4, 20, un.MATCH | un.UDP_OK)
    rec[4] = _rec(9, 17, un.MATCH | un.IP_OK | un.UDP_UNCHECKED)
    p0, o0, l0, s0, x0 = _canaries(n, 96)
    pay, offs, lens, subs, src, total = ug.udp_gather_np(ring, ug.strided(stride, frame_off), stride - frame_off, rec,
                                                         64, p0, o0, l0, s0, x0)
    assert tuple(total[0]) == (48, 3, 3)
    assert list(offs[:3]) == [0, 0, 16] and list(lens[:3]) == [0, 1, 17]
    assert list(subs[:3]) == [7, 3, 9] and list(src[:3]) == [0, 2, 4]
    want = p0.copy()
    want[0:16] = [0xA1] + [0] * 15
    want[16:48] = list(range(0xB0, 0xB0 + 17)) + [0] * 15
    assert np.array_equal(pay, want)  # bytes 48.. keep the canary
    for got, was in ((offs, o0), (lens, l0), (subs, s0), (src, x0)):
        assert np.array_equal(got[3:], was[3:])  # entries j >= n_msgs keep their value
    # src_index not given: the rest is the same
    pay2, offs2, lens2, subs2, src2, total2 = ug.udp_gather_np(ring, ug.strided(stride, frame_off), stride - frame_off,
                                                               rec, 64, p0, o0, l0, s0)
    assert src2 is None and np.array_equal(pay2, pay) and np.array_equal(offs2, offs) and total2 == total


@pytest.mark.parametrize("frame_off", [8, 2, 0])
def test_messages_come_back_through_build_classify_gather(frame_off):
    """udp_build_np (CSUM) -> udp_classify_np -> udp_gather_np: the original messages, zero-padded, sub_ids equal to
    the channel numbers; built again from the gathered arrays, the same ring."""
    stride, n, n_ch = 2048, 120, 32
    tmpl, pairs = _dest_templates(n_ch)
    chans, subs = ub.make_channels(tmpl), un.make_subs(pairs)
    rng = np.random.default_rng(frame_off)
    room = stride - frame_off - 42
    lens = rng.integers(0, room + 1, n).astype(np.uint16)
    lens[:6] = (0, 1, 15, 16, 17, room)
    src_pay = rng.integers(1, 256, 1 << 16, dtype=np.uint8)
    offs = np.array([rng.integers(0, len(src_pay) - int(ln) + 1) for ln in lens], np.uint64)
    ch = rng.integers(0, n_ch, n).astype(np.uint32)
    ring0 = rng.integers(1, 256, n * stride, dtype=np.uint8)
    ring, flens = ub.udp_build_np(ring0, stride, frame_off, chans, src_pay, len(src_pay), offs, lens, ch, ub.UB_CSUM)
    rec = un.udp_classify_np(ring, stride, frame_off, subs)
    assert un.deliver(rec["flags"]).all()
    need = sum(ug.pad16(ln) for ln in lens)
    p0, o0, l0, s0, x0 = _canaries(n, need + 64)
    pay, g_offs, g_lens, g_subs, g_src, total = ug.udp_gather_np(ring, ug.strided(stride, frame_off),
                                                                 stride - frame_off, rec, need, p0, o0, l0, s0, x0)
    assert tuple(total[0]) == (need, n, n)
    assert np.array_equal(g_lens, lens) and np.array_equal(g_subs, ch) and np.array_equal(g_src, np.arange(n))
    assert (g_offs % 16 == 0).all() and np.array_equal(pay[need:], p0[need:])
    for i in range(n):
        o, ln = int(g_offs[i]), int(lens[i])
        assert np.array_equal(pay[o:o + ln], src_pay[int(offs[i]):int(offs[i]) + ln])
        assert not pay[o + ln:o + ug.pad16(ln)].any()
    again, flens2 = ub.udp_build_np(ring0, stride, frame_off, chans, pay, need, g_offs, g_lens, g_subs, ub.UB_CSUM)
    assert np.array_equal(again, ring) and np.array_equal(flens2, flens)


def test_forged_records_are_not_taken():
    """payload_len past avail and payload_off of 40: a DELIVER flag alone takes nothing."""
    stride, frame_off, n = 256, 8, 6
    avail = stride - frame_off
    ring = np.random.default_rng(1).integers(1, 256, n * stride, dtype=np.uint8)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    rec[0] = _rec(1, avail - 42, DELIVER_OK)          # ends exactly at avail: taken
    rec[1] = _rec(2, avail - 41, DELIVER_OK)          # one byte past avail
    rec[2] = _rec(3, 65535, DELIVER_OK)
    rec[3] = _rec(4, 10, DELIVER_OK, poff=40)
    rec[4] = _rec(5, 10, DELIVER_OK, poff=0)
    rec[5] = _rec(6, 10, DELIVER_OK)
    p0, o0, l0, s0, x0 = _canaries(n, 512)
    pay, offs, lens, subs, src, total = ug.udp_gather_np(ring, ug.strided(stride, frame_off), avail, rec, 512, p0, o0,
                                                         l0, s0, x0)
    assert tuple(total[0]) == (ug.pad16(avail - 42) + 16, 2, 2)
    assert list(src[:2]) == [0, 5] and list(subs[:2]) == [1, 6]
    # indexed: an offset outside the class is not taken either, whatever its record says
    offsets = np.array([i * stride + frame_off for i in range(n)], np.uint64)
    offsets[5] += 2
    _, _, _, _, src_i, total_i = ug.udp_gather_np(ring, ug.indexed(offsets, frame_off), avail, rec, 512, p0, o0, l0,
                                                  s0, x0)
    assert tuple(total_i[0]) == (ug.pad16(avail - 42), 1, 1) and src_i[0] == 0


@pytest.mark.parametrize("cap,fit", [(0, 1), (16, 2), (32, 2), (48, 4), (64, 4), (80, 5), (96, 5)])
def test_capacity(cap, fit):
    """Lengths 0, 16, 17, 0, 30: ends 0, 16, 48, 48, 80 (an empty message fits where the one before it ends).  A message that does not fit is indexed, not copied; the
    copied ones are a prefix; n_bytes reports the need whatever the capacity."""
    stride, frame_off, n = 128, 0, 5
    ring = np.random.default_rng(2).integers(1, 256, n * stride, dtype=np.uint8)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    for i, ln in enumerate((0, 16, 17, 0, 30)):
        rec[i] = _rec(i, ln, DELIVER_OK)
    p0, o0, l0, s0, x0 = _canaries(n, 128)
    pay, offs, lens, subs, src, total = ug.udp_gather_np(ring, ug.strided(stride, frame_off), stride, rec, cap, p0, o0,
                                                         l0, s0, x0)
    assert tuple(total[0]) == (80, 5, fit)
    assert list(offs) == [0, 0, 16, 48, 48] and list(lens) == [0, 16, 17, 0, 30]
    ends = [0, 16, 48, 48, 80]
    written = max([e for e in ends if e <= cap], default=0)
    assert np.array_equal(pay[written:], p0[written:])
    if cap >= 16:
        assert np.array_equal(pay[0:16], ring[stride + 42:stride + 58])
