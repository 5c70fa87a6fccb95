"""Inputs for the strided verifying paths (pn_classify, the resident service and the notify form, pn_tx_fill in TCP
mode, pn_udp_classify): rings that hold one frame of every segment length a slot can hold, in slots whose every
other byte is poison -- random bytes in 1..254.  A 16-bit word of such bytes is never 0x0000 or 0xFFFF, so a sum
that takes in one word too many, or one too few, always moves.

Relative to a frame's header window (which starts at ip - MIS on the ring's 16-B grid) the summed extent is
E = MIS + 20 + the segment rounded up to a word, and the kernels stream from s0 = stream_start(window) on, one of
0, 16 .. 112; `geometry` restates both for a ring whose base lies on the 128-B grid.  The lengths put E at and
around every point where the stream changes its behaviour: s0, the window end (112), s0 + 1024 (the second
stream KiB and the short-frame gate), s0 + 2048 and every further KiB (the jumbo loop), the slot's last word.

Everything here is numpy and the C oracle: no GPU call, no pollnet_amd import.  tests/test_strided_extent_np.py
shows on the CPU that the rings hold these cases; tests/test_gpu_strided_extent.py runs them."""
import functools
import struct

import numpy as np

from oracle import pyoracle as orc

import indexed_np as ixn
import udp_np as un
from frames import ip4

# (frame_off, stride)
LAYOUTS = [(2, 2048),                                                       # s0 = 112, the production layout
           (0, 2048),                                                       # per-lane windows, s0 = 0, MIS 14
           (18, 2048), (50, 2048), (98, 2048), (114, 2048),                 # s0 = 96, 64, 16, 0
           (4, 2048), (6, 2048), (8, 2048), (10, 2048), (12, 2048), (14, 2048),  # the other alignment classes
           (2, 1536), (2, 256),                                             # tight rings
           (2, 2064), (10, 1584), (6, 2000),                                # stride % 128 = 16, 48, 80
           (2, 4096), (8, 9216), (2, 65536)]                                # the jumbo loop
OFF_GRID = [(f, s) for f, s in LAYOUTS if s % 128]
TILED = [(2, 2048), (18, 2048), (2, 2064), (2, 4096)]
UDP_LAYOUTS = [(2, 2048), (0, 2048), (18, 2048), (2, 2064), (6, 4096)]
ORDERS = ("ascending", "shuffled", "alternating")

ETH = b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02\x08\x00"
DST, DPORT = ip4("10.0.0.1"), 1234
# The IP option words sum to 0xFFFB = -4 in one's complement: the reference's sum, which starts at ip + 20 whatever
# the IHL says and so takes in the 4 option bytes and a pseudo-header length 4 larger, equals RFC 793's sum.  An
# uncorrupted IHL 6 frame of even length therefore carries PN_F_TCP_OK and PN_F_RFC_TCP_OK like every other.
IP_OPTS = bytes([0x7F, 0xFD, 0x7F, 0xFE])
TCP_OPTS = bytes(range(2, 14))
BIT_LAST, BIT_STREAM = 0x04, 0x10


def geometry(frame_off, stride, slot_index):
    """(MIS, ipa_off, s0) of slot slot_index (an int or an array of them): the window starts ipa_off bytes into
    the slot and MIS bytes below the IP header; s0 is stream_start of it for a ring base on the 128-B grid."""
    mis = (frame_off + 14) % 16
    ipa_off = (frame_off + 14) & ~15
    s0 = 112 - ((np.asarray(slot_index, np.int64) * stride + ipa_off - 16) & 112)
    return mis, ipa_off, s0


def extent(tot_len, mis):
    """The summed extent relative to the window start: MIS + tot_len rounded up to a word."""
    return mis + ((np.asarray(tot_len, np.int64) + 1) & ~1)


def _be_sum(a):
    """Big-endian 16-bit word sum of a uint8 array, an odd last byte padded with zero (not folded)."""
    n = len(a) & ~1
    s = int(a[:n].view(">u2").sum(dtype=np.uint64))
    if len(a) & 1:
        s += int(a[-1]) << 8
    return s


def _csum(s):
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def build_frame(src, sport, seq, payload, ihl=5, doff=5, tot_len=None):
    """frames.make_frame(src=, sport=, seq=, payload=, ihl=, doff=, ip_opts=IP_OPTS, tcp_opts=TCP_OPTS, tot_len=)
    as a uint8 array, the checksums from vectorised word sums (make_frame's byte loop takes 10 ms at 64 KiB)."""
    hl, th = 4 * ihl, 4 * doff
    seg_len = th + len(payload)
    tl = hl + seg_len if tot_len is None else tot_len
    head = (ETH + struct.pack("!BBHHHBBH4s4s", 0x40 | ihl, 0, tl & 0xFFFF, 7, 0x4000, 64, 6, 0, ip4(src), DST)
            + IP_OPTS[:hl - 20] + struct.pack("!HHIIBBHHH", sport, DPORT, seq & 0xFFFFFFFF, 0, doff << 4, 0x18, 0xFFFF, 0, 0)
            + TCP_OPTS[:th - 20])
    f = np.empty(14 + hl + seg_len, np.uint8)
    f[:len(head)] = np.frombuffer(head, np.uint8)
    f[len(head):] = payload
    c = _csum(_be_sum(f[14:14 + hl]))
    f[24], f[25] = c >> 8, c & 0xFF
    c = _csum(_be_sum(f[26:34]) + 6 + seg_len + _be_sum(f[14 + hl:]))
    f[14 + hl + 16], f[14 + hl + 17] = c >> 8, c & 0xFF
    return f


def _bands(frame_off, stride, lo, hi, head):
    """Every length in [lo, hi] for a slot of up to 4 KiB.  Above: lo .. head, every length whose extent lies
    within 20 of s0 + 1024 k for every k the slot holds, and the last 40 lengths."""
    if stride <= 4096:
        return list(range(lo, hi + 1))
    assert stride % 128 == 0  # one s0 for the whole ring
    mis, _, s0 = geometry(frame_off, stride, 0)
    t = np.arange(lo, hi + 1)
    d = (extent(t, mis) - int(s0)) % 1024
    keep = (t <= head) | (t > hi - 40) | (d <= 20) | (d >= 1024 - 20)
    return t[keep].tolist()


def sweep_lengths(frame_off, stride):
    """The swept tot_len values of a TCP ring, ascending: every frame of them is summed."""
    return _bands(frame_off, stride, 40, stride - frame_off - 14, 400)


def unsummed_lengths(frame_off, stride):
    """tot_len values appended to every TCP ring: below the headers, or past the slot (PN_F_TRUNC)."""
    avail = stride - frame_off
    return [0, 19, 20, 39, avail - 13, avail - 12, 65535]


def udp_lengths(frame_off, stride):
    """The payload lengths of a UDP ring, ascending: 0 .. room for a slot of about 2 KiB, the bands above."""
    room = stride - frame_off - 42
    if stride <= 2048 or stride % 128:
        assert room <= 2048
        return list(range(room + 1))
    mis, _, s0 = geometry(frame_off, stride, 0)
    t = np.arange(room + 1)
    d = (extent(28 + t, mis) - int(s0)) % 1024
    keep = (t <= 360) | (t > room - 40) | (d <= 20) | (d >= 1024 - 20)
    return t[keep].tolist()


def _order(n_swept, n_extra, order, seed):
    """Positions of the ascending swept frames (0 .. n_swept - 1) and the appended ones behind them."""
    n = n_swept + n_extra
    if order == "ascending":
        return np.arange(n)
    if order == "shuffled":
        return np.random.default_rng(seed).permutation(n)
    assert order == "alternating"
    a = np.empty(n_swept, np.int64)
    a[0::2] = np.arange((n_swept + 1) // 2)
    a[1::2] = n_swept - 1 - np.arange(n_swept // 2)
    return np.concatenate([a, np.arange(n_swept, n)])


class Ring:
    """A TCP ring and what the builder knows of each slot: tot_len, swept (or appended), corrupt, ihl."""

    def __init__(self, frame_off, stride, slots, tot, swept, corrupt, ihl, exp=None):
        self.frame_off, self.stride, self.avail = frame_off, stride, stride - frame_off
        self.slots, self.tot, self.swept, self.corrupt, self.ihl = slots, tot, swept, corrupt, ihl
        self._exp = exp
        for a in (slots, tot, swept, corrupt, ihl):
            a.setflags(write=False)

    @property
    def n(self):
        return len(self.tot)

    @property
    def mis(self):
        return (self.frame_off + 14) % 16

    @property
    def s0(self):
        return geometry(self.frame_off, self.stride, np.arange(self.n))[2]

    @property
    def ext(self):
        return extent(self.tot, self.mis)

    @property
    def exp(self):
        """The oracle's records."""
        if self._exp is None:
            e, m = ixn.conn_entries()
            self._exp = orc.classify_batch(self.slots, self.stride, self.frame_off, self.n, e, m, ixn.MAX_CONN, threads=8)
            self._exp.setflags(write=False)
        return self._exp

    def take(self, idx):
        """The ring of slots idx (copies): records follow their frames, s0 follows the new slot index."""
        idx = np.asarray(idx)
        return Ring(self.frame_off, self.stride, np.ascontiguousarray(self.slots[idx]), self.tot[idx], self.swept[idx],
                    self.corrupt[idx], self.ihl[idx], self.exp[idx])

    def describe(self, i):
        """Frame i for a failure message."""
        s0 = int(self.s0[i])
        return (f"frame {i}: tot_len {int(self.tot[i])}, extent {int(self.ext[i])}, s0 {s0}, lane {i % 64} (of 8: {i % 8}), "
                f"ihl {int(self.ihl[i])}, corrupt {bool(self.corrupt[i])}, layout (frame_off {self.frame_off}, stride {self.stride})")


def tcp_ring(frame_off, stride, tots, order, seed, plain=False):
    """One valid frame of every tot_len in `tots` (ascending) and the unsummed_lengths behind them, placed as
    `order` says, in slots of poison.  By slot index i: the source is SOURCES[i % 3]; every 7th frame has IHL 6,
    every 5th doff 8 (from tot_len 60 on); every 11th a bit flipped in its last byte; every 13th a bit flipped in
    the first byte the stream loads (window offset s0), or the first segment byte where that lies above it,
    when the frame reaches that far.  plain: IHL 5 and no flipped bits (what a sender's ring holds: pn_tx_fill)."""
    avail = stride - frame_off
    extra = unsummed_lengths(frame_off, stride)
    pos = _order(len(tots), len(extra), order, seed)
    all_tot = np.array(list(tots) + extra, np.int64)[pos]
    swept = (pos < len(tots))
    n = len(all_tot)
    rng = np.random.default_rng(seed + 1)
    slots = rng.integers(1, 255, (n, stride), dtype=np.uint8)
    mis, ipa_off, s0 = geometry(frame_off, stride, np.arange(n))
    corrupt, ihls = np.zeros(n, bool), np.full(n, 5, np.int64)
    for i in range(n):
        tot = int(all_tot[i])
        src, sport = ixn.SOURCES[i % 3]
        seq = int(rng.integers(1 << 32))
        if swept[i]:
            ihl = 6 if (not plain and i % 7 == 6 and tot >= 60) else 5
            doff = 8 if (i % 5 == 4 and tot >= 60) else 5
            f = build_frame(src, sport, seq, rng.integers(1, 255, tot - 4 * ihl - 4 * doff, dtype=np.uint8), ihl, doff)
            assert len(f) == 14 + tot
            ihls[i] = ihl
        else:  # a whole frame with another length in its header: as long as the slot when the length says longer
            real = avail - 14 if avail - 13 <= tot < 65535 else min(avail - 14, 240)
            f = build_frame(src, sport, seq, rng.integers(1, 255, real - 40, dtype=np.uint8), tot_len=tot)
        slots[i, frame_off:frame_off + len(f)] = f
        if plain or not swept[i]:
            continue
        if i % 11 == 10:
            slots[i, frame_off + 13 + tot] ^= BIT_LAST
            corrupt[i] = True
        if i % 13 == 12:
            p = max(ipa_off + int(s0[i]), frame_off + 14 + 4 * int(ihls[i]))
            if p < frame_off + 14 + tot:
                slots[i, p] ^= BIT_STREAM
                corrupt[i] = True
    return Ring(frame_off, stride, slots, all_tot, swept, corrupt, ihls)


def _seed(frame_off, stride):
    return 100003 * frame_off + stride


@functools.lru_cache(maxsize=3)
def sweep_ring(frame_off, stride, order, plain=False):
    """tcp_ring over sweep_lengths(frame_off, stride), seeded by the layout."""
    return tcp_ring(frame_off, stride, sweep_lengths(frame_off, stride), order, _seed(frame_off, stride), plain)


def tile(ring, reps):
    """`reps` copies of the ring, one behind the other.  The copied length is odd (an even ring goes without its
    last slot), so every repeat -- up to 64 of them -- starts on another lane of a wave, and at a stride off the
    128-B grid every frame meets all eight s0 values within 8 repeats."""
    m = ring.n - (ring.n % 2 == 0)
    starts = (np.arange(reps) * m) % 64
    assert m % 2 == 1 and len(set(starts[:64].tolist())) == min(reps, 64)
    return ring.take(np.tile(np.arange(m), reps))


def band_subset(ring, limit=1024):
    """Indices of the frames whose extent lies within 20 of a stream boundary (s0, the window end, every KiB from
    s0 on), the 40 longest, and the appended ones: a batch for the entry points that take at most `limit` frames."""
    d = (ring.ext - ring.s0) % 1024
    near = (d <= 20) | (d >= 1004) | (np.abs(ring.ext - 112) <= 20) | (ring.tot > ring.avail - 14 - 40)
    idx = np.flatnonzero(near | ~ring.swept)
    assert 0 < len(idx) <= limit
    return idx


# ---------------------------------------------------------------- UDP ----
UDP_SRC = ip4("10.1.2.3")
UDP_PAIRS = [(ip4("239.1.0.10"), 20000), (ip4("239.1.0.11"), 20007), (ip4("239.1.1.10"), 20014), (ip4("10.0.0.1"), 4000)]


def udp_subs():
    return un.make_subs(UDP_PAIRS)


class UdpRing:
    """A UDP ring: plen (payload bytes), summed (subscribed, with a checksum), nocsum, unsub, corrupt per slot."""

    def __init__(self, frame_off, stride, slots, plen, nocsum, unsub, corrupt, exp=None):
        self.frame_off, self.stride, self.avail = frame_off, stride, stride - frame_off
        self.slots, self.plen, self.nocsum, self.unsub, self.corrupt = slots, plen, nocsum, unsub, corrupt
        self._exp = exp
        for a in (slots, plen, nocsum, unsub, corrupt):
            a.setflags(write=False)

    @property
    def n(self):
        return len(self.plen)

    @property
    def summed(self):
        return ~self.nocsum & ~self.unsub

    @property
    def s0(self):
        return geometry(self.frame_off, self.stride, np.arange(self.n))[2]

    @property
    def ext(self):
        return extent(28 + self.plen, (self.frame_off + 14) % 16)

    @property
    def exp(self):
        """The numpy model's records (tests/udp_np.py)."""
        if self._exp is None:
            self._exp = un.udp_classify_np(self.slots, self.stride, self.frame_off, udp_subs())
            self._exp.setflags(write=False)
        return self._exp

    def take(self, idx):
        idx = np.asarray(idx)
        return UdpRing(self.frame_off, self.stride, np.ascontiguousarray(self.slots[idx]), self.plen[idx], self.nocsum[idx],
                       self.unsub[idx], self.corrupt[idx], self.exp[idx])

    def describe(self, i):
        return (f"datagram {i}: payload {int(self.plen[i])}, extent {int(self.ext[i])}, s0 {int(self.s0[i])}, lane {i % 64}, "
                f"nocsum {bool(self.nocsum[i])}, unsub {bool(self.unsub[i])}, corrupt {bool(self.corrupt[i])}, "
                f"layout (frame_off {self.frame_off}, stride {self.stride})")


@functools.lru_cache(maxsize=4)
def udp_ring(frame_off, stride, kind, seed, order="ascending"):
    """One datagram of every payload length of udp_lengths in slots of poison, payload bytes in 1..254.
    kind "all_summed": every datagram is subscribed and carries a valid checksum.  kind "compact": every 2nd
    datagram has checksum 0 and every 3rd of the rest goes to a port nobody subscribed to, so every wave compacts
    another subset.  Every 11th summed datagram with a payload has a bit flipped in its last payload byte."""
    assert kind in ("all_summed", "compact")
    lens = udp_lengths(frame_off, stride)
    plen = np.array(lens, np.int64)[_order(len(lens), 0, order, seed)]
    n = len(plen)
    rng = np.random.default_rng(seed + 2)
    slots = rng.integers(1, 255, (n, stride), dtype=np.uint8)
    nocsum, unsub, corrupt = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    rest = summed = 0
    for i in range(n):
        p = int(plen[i])
        ip, port = UDP_PAIRS[i % len(UDP_PAIRS)]
        if kind == "compact":
            if i % 2 == 1:
                nocsum[i] = True
            else:
                unsub[i] = rest % 3 == 2
                rest += 1
        un.put_udp_frame(slots[i], frame_off, rng.integers(1, 255, p, dtype=np.uint8).tobytes(), UDP_SRC, ip, 1024 + i % 60000,
                         port + int(unsub[i]), udp_csum=0 if nocsum[i] else "valid")
        if not nocsum[i] and not unsub[i]:
            if summed % 11 == 10 and p > 0:
                slots[i, frame_off + 41 + p] ^= BIT_LAST
                corrupt[i] = True
            summed += 1
    return UdpRing(frame_off, stride, slots, plen, nocsum, unsub, corrupt)
