"""tests/udp_demux_np.py pinned before any GPU test trusts it (CPU only): one case worked out by hand, the argsort
identity against tests/udp_gather_np.py on random rings, the capacity rule, the round trip through the build and
classify models, and the vectorised restatement against the loops.  And the surface: RxContext has the two methods and
the library exports the two entry points."""
import ctypes

import numpy as np
import pytest

import pollnet_amd as pa

import udp_build_np as ub
import udp_demux_np as ud
import udp_gather_np as ug
import udp_np as un
from test_udp_build_np import _dest_templates

OK = un.MATCH | un.IP_OK | un.UDP_OK


def canaries(n, n_subs, pay_bytes, seed=5):
    """payloads, offs, lens, subs, src, sub_first (n_subs + 1 and three guard entries), sub_bytes (the same)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 256, pay_bytes, dtype=np.uint8), rng.integers(1, 1 << 62, n).astype(np.uint64),
            rng.integers(1, 1 << 16, n).astype(np.uint16), rng.integers(1 << 20, 1 << 32, n).astype(np.uint32),
            rng.integers(1 << 28, 1 << 32, n).astype(np.uint32),
            rng.integers(1 << 28, 1 << 32, n_subs + 4).astype(np.uint32),
            rng.integers(1 << 50, 1 << 62, n_subs + 4).astype(np.uint64))


def _rec(sub, plen, flags, poff=42):
    r = np.zeros(1, un.UDP_RESULT_DTYPE)
    r[0] = (sub, 0x0100000A, 0x1234, poff, plen, flags)
    return r[0]


def random_records(n, room, n_ids, seed, take=0.75):
    """n records by hand: lengths 0 .. room, sub_ids below n_ids, about `take` of them with a DELIVER flag set."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    lens = rng.integers(0, room + 1, n)
    lens[::7] = np.resize(np.array([0, 1, 15, 16, 17, room - 1, room]), len(lens[::7]))
    rec["sub_id"] = rng.integers(0, n_ids, n)
    rec["payload_off"] = 42
    rec["payload_len"] = lens
    good = np.array([OK, un.MATCH | un.IP_OK | un.NOCSUM, un.MATCH | un.IP_OK | un.UDP_UNCHECKED], np.uint16)
    bad = np.array([un.MATCH | un.IP_OK, un.IP_OK | un.NOT_UDP, un.MATCH | un.UDP_OK, 0], np.uint16)
    rec["flags"] = np.where(rng.random(n) < take, good[np.arange(n) % 3], bad[np.arange(n) % 4])
    return rec


def test_the_surface_exists():
    """Fails before the demux path: no such method, no such export."""
    assert hasattr(pa.RxContext, "udp_demux") and hasattr(pa.RxContext, "udp_demux_indexed")
    lib = ctypes.CDLL(pa.LIB_PATH)
    assert hasattr(lib, "pn_udp_demux") and hasattr(lib, "pn_udp_demux_indexed")
    assert pa.PN_UDP_DEMUX_MAX_N == 1 << 24


def test_six_frames_three_subscriptions_by_hand():
    """Slots of 128 B, frame_off 2, n_subs 3.  Frame 0: sub 2, 17 bytes.  Frame 1: sub 0, 1 byte.  Frame 2: sub 3 ==
    n_subs, DELIVER: skipped.  Frame 3: sub 2, 0 bytes.  Frame 4: not UDP.  Frame 5: sub 0, 17 bytes.  Subscription 1
    gets nothing.  Grouped: sub 0 = frames 1, 5 at bytes 0 and 16; sub 2 = frames 0, 3 at 48 and 80; 80 bytes."""
    stride, frame_off, n, n_subs = 128, 2, 6, 3
    ring = np.full(n * stride, 0xEE, np.uint8)
    at = lambda i: i * stride + frame_off + 42  # noqa: E731
    ring[at(0):at(0) + 17] = np.arange(0xA0, 0xA0 + 17)
    ring[at(1)] = 0xB1
    ring[at(5):at(5) + 17] = np.arange(0xC0, 0xC0 + 17)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    rec[0] = _rec(2, 17, OK)
    rec[1] = _rec(0, 1, un.MATCH | un.IP_OK | un.NOCSUM)
    rec[2] = _rec(3, 9, OK)
    rec[3] = _rec(2, 0, un.MATCH | un.IP_OK | un.UDP_UNCHECKED)
    rec[4] = _rec(un.NO_SUB, 50, un.IP_OK | un.NOT_UDP)
    rec[5] = _rec(0, 17, OK)
    c = canaries(n, n_subs, 128)
    pay, offs, lens, subs, src, first, sbytes, total = ud.udp_demux_np(ring, ug.strided(stride, frame_off),
                                                                       stride - frame_off, rec, n_subs, 96, *c)
    assert tuple(total[0]) == (80, 4, 4)
    assert list(src[:4]) == [1, 5, 0, 3] and list(subs[:4]) == [0, 0, 2, 2]
    assert list(lens[:4]) == [1, 17, 17, 0] and list(offs[:4]) == [0, 16, 48, 80]
    assert list(first[:4]) == [0, 2, 2, 4] and list(sbytes[:4]) == [0, 48, 48, 80]
    want = c[0].copy()
    want[0:16] = [0xB1] + [0] * 15
    want[16:48] = list(range(0xC0, 0xC0 + 17)) + [0] * 15
    want[48:80] = list(range(0xA0, 0xA0 + 17)) + [0] * 15
    assert np.array_equal(pay, want)  # bytes 80.. keep the canary
    for got, was in ((offs, c[1]), (lens, c[2]), (subs, c[3]), (src, c[4])):
        assert np.array_equal(got[4:], was[4:])  # entries j >= n_msgs keep their value
    assert np.array_equal(first[4:], c[5][4:]) and np.array_equal(sbytes[4:], c[6][4:])  # and those past n_subs
    # src_index not given: the rest is the same
    c2 = c[:4] + (None,) + c[5:]
    out2 = ud.udp_demux_np(ring, ug.strided(stride, frame_off), stride - frame_off, rec, n_subs, 96, *c2)
    assert out2[4] is None and np.array_equal(out2[0], pay) and np.array_equal(out2[1], offs) and out2[7] == total


def argsort_identity(gather_out, demux_out, n_subs, buf_cmp=True):
    """The header's identity: with (L, S, I) the gather's arrays restricted to S < n_subs and pi the stable argsort of
    S, the demux's arrays are L[pi], S[pi], I[pi], pay_offs the running sum, and every copied message's bytes equal."""
    g_pay, g_offs, g_lens, g_subs, g_src, g_total = gather_out
    pay, offs, lens, subs, src, first, sbytes, total = demux_out
    m = int(g_total[0]["n_msgs"])
    keep = np.flatnonzero(g_subs[:m] < n_subs)
    pi = keep[np.argsort(g_subs[keep], kind="stable")]
    k = len(pi)
    assert int(total[0]["n_msgs"]) == k
    assert np.array_equal(lens[:k], g_lens[pi]) and np.array_equal(subs[:k], g_subs[pi])
    assert np.array_equal(src[:k], g_src[pi])
    pad = (g_lens[pi].astype(np.int64) + 15) // 16 * 16
    assert np.array_equal(offs[:k], (np.cumsum(pad) - pad).astype(np.uint64))
    assert int(total[0]["n_bytes"]) == int(pad.sum())
    assert np.array_equal(first[:n_subs + 1], np.searchsorted(g_subs[pi], np.arange(n_subs + 1)))
    assert np.array_equal(sbytes[:n_subs + 1], np.concatenate([offs[:k], [pad.sum()]]).astype(np.uint64)[first[:n_subs + 1]])
    if buf_cmp:
        g_fit = int(g_total[0]["n_fit"])
        for j in range(int(total[0]["n_fit"])):
            if pi[j] < g_fit:
                a, b, w = int(offs[j]), int(g_offs[pi[j]]), int(pad[j])
                assert np.array_equal(pay[a:a + w], g_pay[b:b + w]), j


@pytest.mark.parametrize("n,n_subs,n_ids,seed", [(1, 1, 1, 0), (40, 1, 3, 1), (200, 7, 9, 2), (300, 64, 64, 3),
                                                 (500, 4096, 5000, 4), (257, 300, 300, 5)])
def test_argsort_identity_against_the_gather_model(n, n_subs, n_ids, seed):
    stride, frame_off = 256, 6
    avail = stride - frame_off
    ring = np.random.default_rng(seed).integers(1, 256, n * stride, dtype=np.uint8)
    rec = random_records(n, avail - 42, n_ids, seed)
    cap = n * ug.pad16(avail)
    c = canaries(n, n_subs, cap + 64, seed)
    g = ug.udp_gather_np(ring, ug.strided(stride, frame_off), avail, rec, cap, *c[:5])
    d = ud.udp_demux_np(ring, ug.strided(stride, frame_off), avail, rec, n_subs, cap, *c)
    argsort_identity(g, d, n_subs)
    # and the vectorised restatement gives the loops' outputs, whole
    eth = np.arange(n, dtype=np.int64) * stride + frame_off
    f = ud.udp_demux_fast_np(ring, eth, avail, rec, n_subs, cap, *c)
    for a, b in zip(d, f):
        assert np.array_equal(a, b)


def test_the_fast_model_equals_the_loops_indexed_and_short_of_capacity():
    stride, frame_off, n, n_subs = 128, 4, 300, 11
    avail = stride - frame_off
    ring = np.random.default_rng(8).integers(1, 256, n * stride, dtype=np.uint8)
    rec = random_records(n, avail - 42, 13, 8)
    offsets = (np.arange(n, dtype=np.uint64)[::-1] * stride + frame_off).copy()
    offsets[::10] += 2
    eth = np.where(offsets % 16 == frame_off, offsets.astype(np.int64), -1)
    need = sum(ug.pad16(r["payload_len"]) for i, r in enumerate(rec) if eth[i] >= 0 and ud.taken(r, avail, n_subs))
    for cap in (0, 16, (need // 2) & ~15, need - 16, need):
        c = canaries(n, n_subs, need + 64, cap)
        d = ud.udp_demux_np(ring, ug.indexed(offsets, frame_off), avail, rec, n_subs, cap, *c)
        f = ud.udp_demux_fast_np(ring, eth, avail, rec, n_subs, cap, *c)
        for a, b in zip(d, f):
            assert np.array_equal(a, b)
        assert int(d[7][0]["n_bytes"]) == need


# sub 0: 16, 17 (ends 16, 48); sub 1: 0, 30, 0 (ends 48, 80, 80); sub 2: nothing; sub 3: 0, 5 (ends 80, 96)
CAP_SUBS = (0, 1, 3, 0, 1, 1, 3)
CAP_LENS = (16, 0, 0, 17, 30, 0, 5)
CAP_CASES = [(0, 0, "zero"), (96, 7, "exact"), (80, 6, "one block short"),
             (64, 3, "inside subscription 1: its 30 bytes cross, the empty messages after them do not fit"),
             (48, 3, "on the boundary of subscriptions 0 and 1: the empty message that starts 1 fits"),
             (32, 1, "inside subscription 0"), (16, 1, "the first message exactly")]


def capacity_case():
    stride, n = 128, len(CAP_SUBS)
    ring = np.random.default_rng(2).integers(1, 256, n * stride, dtype=np.uint8)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    for i, (s, ln) in enumerate(zip(CAP_SUBS, CAP_LENS)):
        rec[i] = _rec(s, ln, OK)
    return ring, rec, stride


@pytest.mark.parametrize("cap,fit,why", CAP_CASES)
def test_capacity(cap, fit, why):
    """A message that does not fit is indexed, not copied; the copied ones are a prefix in grouped order; n_bytes
    reports the need whatever the capacity."""
    ring, rec, stride = capacity_case()
    n = len(rec)
    c = canaries(n, 4, 160)
    pay, offs, lens, subs, src, first, sbytes, total = ud.udp_demux_np(ring, ug.strided(stride, 0), stride, rec, 4, cap,
                                                                       *c)
    assert tuple(total[0]) == (96, 7, fit), why
    assert list(src) == [0, 3, 1, 4, 5, 2, 6]
    assert list(offs) == [0, 16, 48, 48, 80, 80, 80] and list(lens) == [16, 17, 0, 30, 0, 0, 5]
    assert list(first[:5]) == [0, 2, 5, 5, 7] and list(sbytes[:5]) == [0, 48, 80, 80, 96]
    ends = [16, 48, 48, 80, 80, 80, 96]
    written = max([e for e in ends[:fit]], default=0)
    assert np.array_equal(pay[written:], c[0][written:])
    if fit >= 1:
        assert np.array_equal(pay[0:16], ring[42:58])


@pytest.mark.parametrize("frame_off", [8, 2])
def test_each_channel_comes_back_in_order_through_build_classify_demux_build(frame_off):
    """udp_build_np (CSUM) -> udp_classify_np -> udp_demux_np: each channel's messages, contiguous and in the order
    they were sent; built again from the demuxed arrays, each channel's frames in order."""
    stride, n, n_ch = 2048, 150, 12
    tmpl, pairs = _dest_templates(n_ch)
    chans, subs_tbl = ub.make_channels(tmpl), un.make_subs(pairs)
    rng = np.random.default_rng(frame_off)
    room = stride - frame_off - 42
    lens = rng.integers(0, room + 1, n).astype(np.uint16)
    lens[:6] = (0, 1, 15, 16, 17, room)
    src_pay = rng.integers(1, 256, 1 << 16, dtype=np.uint8)
    offs = np.array([rng.integers(0, len(src_pay) - int(ln) + 1) for ln in lens], np.uint64)
    ch = rng.integers(0, n_ch - 1, n).astype(np.uint32)  # the last channel sends nothing
    ring0 = rng.integers(1, 256, n * stride, dtype=np.uint8)
    ring, flens = ub.udp_build_np(ring0, stride, frame_off, chans, src_pay, len(src_pay), offs, lens, ch, ub.UB_CSUM)
    rec = un.udp_classify_np(ring, stride, frame_off, subs_tbl)
    assert un.deliver(rec["flags"]).all()
    need = sum(ug.pad16(ln) for ln in lens)
    c = canaries(n, n_ch, need + 64)
    pay, d_offs, d_lens, d_subs, d_src, first, sbytes, total = ud.udp_demux_np(
        ring, ug.strided(stride, frame_off), stride - frame_off, rec, n_ch, need, *c)
    assert tuple(total[0]) == (need, n, n)
    order = np.argsort(ch, kind="stable")
    assert np.array_equal(d_src, order) and np.array_equal(d_subs, ch[order]) and np.array_equal(d_lens, lens[order])
    assert first[n_ch - 1] == first[n_ch] == n and sbytes[n_ch - 1] == sbytes[n_ch] == need
    for j in range(n):
        o, ln, i = int(d_offs[j]), int(d_lens[j]), int(order[j])
        assert np.array_equal(pay[o:o + ln], src_pay[int(offs[i]):int(offs[i]) + ln])
        assert not pay[o + ln:o + ug.pad16(ln)].any()
    again, flens2 = ub.udp_build_np(ring0, stride, frame_off, chans, pay, need, d_offs, d_lens, d_subs, ub.UB_CSUM)
    assert np.array_equal(flens2, flens[order])
    for j in range(n):  # the frame's own bytes (what follows them in a slot is the slot's, not the frame's)
        got, want = again.reshape(n, stride)[j], ring.reshape(n, stride)[order[j]]
        assert np.array_equal(got[frame_off:frame_off + flens2[j]], want[frame_off:frame_off + flens2[j]]), j
    for s in range(n_ch):
        mine = np.flatnonzero(ch == s)
        assert np.array_equal(d_src[first[s]:first[s + 1]], mine)
