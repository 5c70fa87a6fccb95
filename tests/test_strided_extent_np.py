"""CPU: the rings of tests/strided_np.py hold the cases tests/test_gpu_strided_extent.py is about, and the expected
records are sound -- so the GPU file asserts nothing about its own inputs and cannot pass vacuously.  The frame
builder against frames.make_frame; every swept length present once; poison everywhere outside the frames; the
oracle's verdicts on the sweep; records that depend on the bytes behind a frame only where the reference sums
one (odd lengths); every stream boundary of `BOUNDARIES` reached, or exempted by name in `EXEMPT`; the TX and UDP
forms of the same rings."""
import numpy as np
import pytest

from oracle import pyoracle as orc

import indexed_np as ixn
import strided_np as sn
import udp_np as un
from frames import make_frame

# Summed extents E a ring must hold, by name: relative to the slot's s0 (`s0+d`), to the window (`E`), or to
# the slot (`last word`).  Every s0 + d with d = 2 mod 4 ends a half-dword into the last dword loaded (the
# 2-mod-4 correction), every d = 0 mod 4 on a dword; e16 == s0 + 1024 - 4, + 0, + 4 (the wave gate, the second KiB's
# first load) is E = s0 + 1018 .. s0 + 1028.  `pad@s0+d`: an odd tot_len whose pad byte -- the byte behind the segment
# that the reference sums -- lies at window offset s0 + d; E is even, so that offset is odd: the bytes at s0,
# s0 + 1024 and s0 + 2048 themselves are never a pad byte, and the ring holds the ones on either side of them.
S0_REL = [-2, 0, 2, 1018, 1020, 1022, 1024, 1026, 1028, 2046, 2048, 2050, 3070, 3072, 3074]
WINDOW = [110, 112, 114]
PAD_REL = [-1, 1, 1023, 1025, 2047, 2049]


def _fmt(d):
    return "s0%+d" % d if d else "s0"


BOUNDARIES = ([_fmt(d) for d in S0_REL] + ["E%d" % e for e in WINDOW] + ["pad@" + _fmt(d) for d in PAD_REL]
              + ["last word", "pad@last byte"])

# What a layout's slots cannot reach: E lies in [MIS + 40, MIS + avail - 14].  Below it: s0 <= 32 and a boundary at
# s0 itself.  Above it: the boundaries 2 KiB (3 KiB) past s0 in slots of up to 2 KiB (the 4 KiB ones: 3 KiB + MIS +
# s0 + 2 still fits at frame_off 2, s0 112).
_2K = {"s0+2046", "s0+2048", "s0+2050", "pad@s0+2047", "pad@s0+2049", "s0+3070", "s0+3072", "s0+3074"}
_AT_S0 = {"s0-2", "s0", "s0+2", "pad@s0-1", "pad@s0+1"}
EXEMPT = {(2, 256): _2K | {"s0+1018", "s0+1020", "s0+1022", "s0+1024", "s0+1026", "s0+1028", "pad@s0+1023", "pad@s0+1025"}}
for _l in sn.LAYOUTS:
    if _l[1] <= 2064 and _l != (2, 256):
        EXEMPT[_l] = set(_2K)
for _l in ((0, 2048), (114, 2048), (98, 2048)):  # s0 = 0, 0, 16: below the bare headers
    EXEMPT[_l] |= _AT_S0
for _l in ((0, 2048), (2, 2064)):  # MIS + avail - 14 = 2048 and s0 = 0: the longest frames end 2 KiB past s0
    EXEMPT[_l] -= {"s0+2046", "s0+2048", "pad@s0+2047"}
for _l in sn.LAYOUTS:
    EXEMPT.setdefault(_l, set())


def reached(ring):
    """(names reached, names the layout cannot reach), over the swept frames of a ring."""
    e, s0, tot = ring.ext[ring.swept], ring.s0[ring.swept], ring.tot[ring.swept]
    lo, hi = ring.mis + 40, ring.mis + ring.avail - 14
    odd = tot % 2 == 1
    hit, cannot = set(), set()

    def note(name, at, want):
        """at: frames at the boundary; want: the E the boundary needs, per s0 value."""
        if at.any():
            hit.add(name)
        if not ((want >= lo) & (want <= hi)).any():
            cannot.add(name)

    s0v = np.unique(s0)
    for d in S0_REL:
        note(_fmt(d), e == s0 + d, s0v + d)
    for w in WINDOW:
        note("E%d" % w, e == w, np.array([w]))
    for d in PAD_REL:
        note("pad@" + _fmt(d), odd & (e - 1 == s0 + d), s0v + d + 1)
    note("last word", e == hi, np.array([hi]))
    note("pad@last byte", odd & (ring.frame_off + 14 + tot == ring.stride - 1), np.array([hi]))
    return hit, cannot


def coverage_ring(frame_off, stride):
    """The ring whose coverage counts: on the 128-B grid s0 is one value and the order does not matter; off it,
    the shuffled ring 8 times over (sn.tile), where every frame meets every s0."""
    r = sn.sweep_ring(frame_off, stride, "shuffled")
    return sn.tile(r, 8) if stride % 128 else r


def test_frame_builder_equals_make_frame():
    rng = np.random.default_rng(5)
    lens = [0, 1, 2, 3, 7, 1459, 1460] + rng.integers(0, 2000, 193).tolist()
    assert len(lens) == 200 and any(v % 2 for v in lens)
    seen = set()
    for k, plen in enumerate(lens):
        ihl, doff = (6 if k % 3 == 1 else 5), (8 if k % 4 == 2 else 5)
        seen.add((ihl, doff))
        src, sport = ixn.SOURCES[k % 3]
        pay = rng.integers(0, 256, plen, dtype=np.uint8)
        tl = None if k % 10 else 19 + k
        got = sn.build_frame(src, sport, 77 * k + 0xFFFFFF00, pay, ihl, doff, tl)
        ref = make_frame(src=src, sport=sport, seq=77 * k + 0xFFFFFF00, payload=pay.tobytes(), ihl=ihl, doff=doff,
                         ip_opts=sn.IP_OPTS, tcp_opts=sn.TCP_OPTS, tot_len=tl)
        assert got.tobytes() == ref, (k, plen, ihl, doff)
    assert seen == {(5, 5), (6, 5), (5, 8), (6, 8)}


def test_geometry():
    assert sn.geometry(2, 2048, 5) == (0, 16, 112) and sn.geometry(0, 2048, 0) == (14, 0, 0)
    for off, s0 in ((18, 96), (50, 64), (98, 16), (114, 0)):
        assert sn.geometry(off, 2048, 3)[2] == s0
    assert sorted({(off + 14) % 16 for off, _ in sn.LAYOUTS}) == list(range(0, 16, 2))
    for off, stride in sn.OFF_GRID:
        assert stride % 16 == 0 and stride % 128 in (16, 48, 80)
        assert sorted(sn.geometry(off, stride, np.arange(8))[2].tolist()) == list(range(0, 128, 16))
    assert [s % 128 for _, s in sn.OFF_GRID] == [16, 48, 80]
    assert sn.extent(41, 6) == 48 and sn.extent(40, 0) == 40


@pytest.mark.parametrize("frame_off,stride", sn.LAYOUTS)
def test_sweep_lengths(frame_off, stride):
    avail = stride - frame_off
    tots = sn.sweep_lengths(frame_off, stride)
    assert tots == sorted(set(tots)) and tots[0] == 40 and tots[-1] == avail - 14
    if stride <= 4096:
        assert tots == list(range(40, avail - 13))
    else:
        mis, _, s0 = sn.geometry(frame_off, stride, 0)
        have = set(tots)
        assert set(range(40, 401)) <= have and set(range(avail - 14 - 39, avail - 13)) <= have
        t = np.arange(40, avail - 13)
        for k in range((mis + avail - 14 - int(s0)) // 1024 + 1):
            band = t[np.abs(sn.extent(t, mis) - int(s0) - 1024 * k) <= 20].tolist()
            assert set(band) <= have and (k == 0 or len(band) == 42), k
    for order in sn.ORDERS:
        r = sn.sweep_ring(frame_off, stride, order)
        assert sorted(r.tot[r.swept].tolist()) == tots, "a swept tot_len is missing or doubled"
        assert sorted(r.tot[~r.swept].tolist()) == sorted(sn.unsummed_lengths(frame_off, stride))
    asc, alt = sn.sweep_ring(frame_off, stride, "ascending"), sn.sweep_ring(frame_off, stride, "alternating")
    assert asc.tot[:len(tots)].tolist() == tots
    assert alt.tot[:4].tolist() == [tots[0], tots[-1], tots[1], tots[-2]]
    b = alt.tot[:len(tots) // 8 * 8].reshape(-1, 8)  # every batch of 8 holds frames from both halves of the sweep
    mid = tots[len(tots) // 2]
    assert ((b.min(1) <= mid) & (b.max(1) >= mid)).all() and b[0].max() - b[0].min() >= tots[-1] - 44


@pytest.mark.parametrize("frame_off,stride", sn.LAYOUTS)
@pytest.mark.parametrize("order", sn.ORDERS)
def test_ring_poison_and_verdicts(frame_off, stride, order):
    r = sn.sweep_ring(frame_off, stride, order)
    e, m = ixn.conn_entries()
    # no byte outside a frame is 0x00 or 0xFF (an appended frame: outside its headers -- its length field does
    # not say where it ends, and its payload is poison as well)
    col = np.arange(stride)[None, :]
    end = (frame_off + np.where(r.swept, 14 + r.tot, 54))[:, None]
    outside = r.slots[(col < frame_off) | (col >= end)]
    assert outside.min() >= 1 and outside.max() <= 254 and len(outside) > r.n * 14
    fl = r.exp["flags"]
    ok, rfc, trunc = (fl & ixn.TCP_OK) != 0, (fl & ixn.RFC_TCP_OK) != 0, (fl & ixn.TRUNC) != 0
    good, even = r.swept & ~r.corrupt, r.tot % 2 == 0
    assert (ok & rfc & (r.exp["tcp_fold"] == 0))[good & even].all()
    assert (rfc & ~ok)[good & ~even].all()  # the reference sums the poisoned byte behind the segment
    assert not trunc[r.swept].any()
    assert (trunc | ((r.tot < 40) & ~ok))[~r.swept].all() and trunc[~r.swept].sum() == 5
    assert (~ok & ~rfc)[r.corrupt].all() and r.corrupt.sum() >= r.n // 10
    assert np.array_equal(r.exp["payload_off"].astype(np.int64) + r.exp["payload_len"], 14 + np.minimum(r.tot, 1500))
    assert (r.ihl[r.swept] == 6).any() and ((r.exp["payload_off"] == 66) & (r.ihl == 5)).any()
    for bit in (ixn.HIT, ixn.TW):
        assert (fl & bit).any()
    assert not (fl & (ixn.BADOFF | ixn.TCP_UNCHECKED)).any()
    # the release path's records: both statements of them agree
    unv = orc.classify_batch(r.slots, stride, frame_off, r.n, e, m, ixn.MAX_CONN, unverified=True)
    rel = ixn.release(r.exp)
    assert np.array_equal(unv, rel)


@pytest.mark.parametrize("frame_off,stride", sn.LAYOUTS)
def test_tail_independence(frame_off, stride):
    """Everything outside the frames zeroed: exactly the records of the odd lengths change (the reference sums
    the byte behind them).  A GPU mismatch on an even length is an over-read or a short sum, never the input."""
    r = sn.sweep_ring(frame_off, stride, "shuffled")
    z = r.slots.copy()
    col = np.arange(stride)[None, :]
    end = (frame_off + 14 + np.where(r.swept, r.tot, stride))[:, None]
    z[(col < frame_off) | (col >= end)] = 0
    e, m = ixn.conn_entries()
    exp0 = orc.classify_batch(z, stride, frame_off, r.n, e, m, ixn.MAX_CONN)
    changed = exp0 != r.exp
    assert np.array_equal(changed, r.swept & (r.tot % 2 == 1))
    # and with the pad byte zero, an uncorrupted odd length verifies under the reference's sum too
    odd = r.swept & ~r.corrupt & (r.tot % 2 == 1)
    assert ((exp0["flags"][odd] & ixn.TCP_OK) != 0).all()


@pytest.mark.parametrize("frame_off,stride", sn.LAYOUTS)
def test_boundaries_are_reached(frame_off, stride):
    ring = coverage_ring(frame_off, stride)
    e = ring.ext[ring.swept]
    assert e.min() == ring.mis + 40 and e.max() == ring.mis + ring.avail - 14
    hit, cannot = reached(ring)
    assert cannot == EXEMPT[(frame_off, stride)], sorted(cannot ^ EXEMPT[(frame_off, stride)])
    missing = [b for b in BOUNDARIES if b not in hit and b not in cannot]
    assert not missing, missing
    assert not hit & cannot


def test_every_boundary_is_reached_somewhere():
    """No boundary is exempt in every layout, and both parities of the extent (0 and 2 mod 4) occur at each kind."""
    for b in BOUNDARIES:
        assert any(b not in EXEMPT[l] for l in sn.LAYOUTS), b
    assert {d % 4 for d in S0_REL} == {0, 2} and {w % 4 for w in WINDOW} == {0, 2}
    for l in sn.LAYOUTS:
        r = sn.sweep_ring(*l, "ascending")
        assert {0, 2} <= set((r.ext[r.swept] % 4).tolist())


@pytest.mark.parametrize("frame_off,stride", sn.TILED)
def test_tiling_moves_lanes(frame_off, stride):
    r = sn.sweep_ring(frame_off, stride, "shuffled")
    t = sn.tile(r, 5)
    m = t.n // 5
    assert m % 2 == 1 and m >= r.n - 1 and np.array_equal(t.tot[:m], t.tot[m:2 * m])
    assert len({(k * m) % 64 for k in range(5)}) == 5
    assert np.array_equal(t.exp[m:2 * m], r.exp[:m]) and np.array_equal(t.slots[3 * m + 5], r.slots[5])
    if stride % 128:
        assert not np.array_equal(t.s0[:m], t.s0[m:2 * m])


@pytest.mark.parametrize("frame_off,stride", [(2, 2048), (18, 2048)])
def test_band_subset(frame_off, stride):
    r = sn.sweep_ring(frame_off, stride, "shuffled")
    sub = r.take(sn.band_subset(r))
    assert sub.n <= 1024 and (~sub.swept).sum() == 7
    assert reached(sub)[0] == reached(r)[0]


@pytest.mark.parametrize("frame_off,stride", [(14, 2048), (2, 2048), (34, 4096), (2, 2064)])
def test_tx_fill_restores_the_ring(frame_off, stride):
    """A sender's ring (IHL 5, nothing flipped) with both checksum fields scrambled: the TX contract recomputed
    from the bytes gives back the built ring, poison included; RFC 793's zero pad, so odd lengths too."""
    r = sn.sweep_ring(frame_off, stride, "shuffled", True)
    assert not r.corrupt.any() and (r.ihl == 5).all()
    s = scrambled(r)
    assert ((s != r.slots).any(1) == r.swept).all()
    orc.tx_fill_batch(s, stride, frame_off, r.n, None, orc.TX_TCP)
    assert np.array_equal(s, r.slots)


def scrambled(ring, tot_too=False):
    """A copy with the IP and TCP checksum fields (and tot_len) of every swept frame replaced by other bytes."""
    s = ring.slots.copy()
    rng = np.random.default_rng(ring.n)
    ip = ring.frame_off + 14
    for lo in (ip + 10, ip + 36) + ((ip + 2,) if tot_too else ()):
        old = s[:, lo:lo + 2]
        new = np.where(ring.swept[:, None], old ^ rng.integers(1, 256, old.shape, dtype=np.uint8), old)
        s[:, lo:lo + 2] = new
    return s


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("kind", ["all_summed", "compact"])
@pytest.mark.parametrize("frame_off,stride", sn.UDP_LAYOUTS)
def test_udp_ring(frame_off, stride, kind, order):
    u = sn.udp_ring(frame_off, stride, kind, 5, order)
    lens = sn.udp_lengths(frame_off, stride)
    room = stride - frame_off - 42
    assert sorted(u.plen.tolist()) == lens and lens[0] == 0 and lens[-1] == room
    if stride <= 2064:
        assert lens == list(range(room + 1))
    fl = u.exp["flags"]
    assert not (fl & un.TRUNC).any() and ((fl & un.IP_OK) != 0).all()
    summed = u.summed
    assert ((fl & un.UDP_OK) != 0)[summed & ~u.corrupt].all() and not (fl & un.UDP_OK)[u.corrupt | ~summed].any()
    assert ((fl & un.NOCSUM) != 0)[u.nocsum & ~u.unsub].all() and np.array_equal((fl & un.MATCH) != 0, ~u.unsub)
    assert u.corrupt.sum() >= summed.sum() // 12
    col = np.arange(stride)[None, :]
    outside = u.slots[(col < frame_off) | (col >= (frame_off + 42 + u.plen)[:, None])]
    assert outside.min() >= 1 and outside.max() <= 254
    if kind == "all_summed":
        assert summed.all()
    else:
        w = summed[:u.n // 8 * 8].reshape(-1, 8)
        assert len({tuple(x) for x in w.tolist()}) >= 3 and u.unsub.any() and u.nocsum.sum() == u.n // 2
    # extents on both sides of s0 + 1024 (the wave gate) and at the slot's last word, both parities
    d = u.ext[summed] - u.s0[summed]
    for v in (1018, 1020, 1022, 1024, 1026, 1028):
        assert (d == v).any() or kind == "compact", v
    assert (u.plen == room).any() and (u.plen == room - 1).any()
