"""Inputs and expected records for pn_classify_indexed where the readable extent `avail` ends inside (or right
at the end of) the 112-B header window: hand-built TCP frames (tests/golden/frames.py) placed in a packed or a
spaced buffer, every record computed one frame at a time by the C oracle on buf[o:o + avail].

For the launch's class eth_mod16 the kernel's window starts at eth + 14 - MIS, MIS = (eth_mod16 + 14) % 16, and
its 16-B chunks lie on the buffer's 16-B grid.  `Geometry` names the chunk avail ends in; the edge list puts
summed extents (34 + the segment rounded up to a word = 14 + tot_len rounded up) at, inside and one word past it.
Everything here is numpy and the oracle: no GPU, no pollnet_amd import."""
import functools

import numpy as np

from oracle import pyoracle as orc

from frames import ip4, make_frame

IP_OK, TCP_OK, HIT, TW, IHL_NE_5 = 0x0001, 0x0002, 0x0004, 0x0008, 0x0200
RFC_TCP_OK, TRUNC, BADOFF, TCP_UNCHECKED = 0x0800, 0x2000, 0x4000, 0x8000
PN_MISS = 0xFFFFFFFF

MAX_CONN, MAX_TW = 16, 16
SRC_HIT, SRC_TW, SRC_MISS = ("10.0.0.2", 40000), ("10.0.0.3", 40001), ("10.9.9.9", 50000)
SOURCES = (SRC_HIT, SRC_TW, SRC_MISS)


def _key(src):
    ip, port = src
    return orc.conn_hash_key(int.from_bytes(ip4(ip), "little"), int.from_bytes(port.to_bytes(2, "big"), "little"))


@functools.lru_cache(maxsize=None)
def conn_entries():
    """(entries, mask): SRC_HIT is connection 3, SRC_TW a TIME_WAIT entry (conn_id >= MAX_CONN), SRC_MISS unknown."""
    t = orc.Table(MAX_CONN, MAX_TW)
    assert t.add(_key(SRC_HIT), 3) == 0 and t.add(_key(SRC_TW), MAX_CONN + 2) == 0
    for j in range(6):  # neighbours, so that lookups walk a populated table
        assert t.add(_key(("10.0.%d.7" % (j + 1), 41000 + j)), 4 + j) == 0
    e = t.entries()
    e.setflags(write=False)
    return e, t.mask


def badoff_record():
    r = np.zeros(1, orc.RESULT_DTYPE)
    r["conn_id"], r["flags"] = PN_MISS, BADOFF
    return r[0]


def release(exp):
    """The oracle's full records as pn_set_verify(ctx, 0) reports them (tests/test_gpu_soak.py: release())."""
    r = exp.copy()
    chk = (r["flags"] & BADOFF) == 0
    r["flags"][chk] = (r["flags"][chk] & ~np.uint16(TCP_OK | RFC_TCP_OK)) | np.uint16(TCP_UNCHECKED)
    r["tcp_fold"][chk] = 0xFFFF
    return r


class Geometry:
    """Where avail ends relative to the window's 16-B chunks, for one (eth_mod16, avail)."""

    def __init__(self, eth_mod16, avail):
        self.mis = (eth_mod16 + 14) % 16
        self.c0 = 14 - self.mis                                  # chunk 0's first byte, relative to eth
        self.cs = self.c0 + 16 * ((avail - self.c0) // 16)       # first byte of the chunk avail ends in
        self.partial = self.cs != avail                          # avail ends inside a chunk
        self.in_window = self.cs < self.c0 + 112                 # and that chunk belongs to the window
        self.lo = self.cs if self.partial else avail - 16        # extents in (lo, avail] end in avail's last chunk
        self.reachable = (avail & ~1) > self.cs                  # an even extent fits inside a partial chunk


def extent(tot_len):
    """34 + seg_even, the last summed byte + 1 relative to eth (PN_F_TRUNC when it exceeds avail)."""
    return 34 + ((((tot_len - 20) & 0xFFFF) + 1) & ~1)


def _payload(rng, n):
    return rng.integers(1, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def edge_frames(eth_mod16, avail):
    """The edge list for one (eth_mod16, avail): a tuple of (name, frame bytes, tot_len, corrupted).  Frames are
    complete (14 + tot_len bytes, or what make_frame built when tot_len is set by hand)."""
    g = Geometry(eth_mod16, avail)
    rng = np.random.default_rng(1000 * avail + eth_mod16)
    ev = avail & ~1
    out = []
    k = [0]

    def natural(name, tot, corrupt_at=None, **kw):
        src, sport = SOURCES[k[0] % 3]
        k[0] += 1
        f = bytearray(make_frame(src=src, sport=sport, seq=int(rng.integers(1 << 32)), payload=_payload(rng, tot - 40), **kw))
        assert len(f) == 14 + tot
        if corrupt_at is not None:
            assert 54 <= corrupt_at < 14 + tot
            f[corrupt_at] ^= 0x10
        out.append((name, bytes(f), tot, corrupt_at is not None))

    # summed extents at avail, one word below it, every even one in the chunk avail ends in, 2 and 0 mod 4 (as the
    # stream sees them: relative to the window start) at a small size
    exts = [ev, ev - 2] + [e for e in range(g.lo + 1, avail + 1) if e % 2 == 0]
    small = [e for e in range(60, 68, 2) if (e - 14 + g.mis) % 4 == 2][:1] + [e for e in range(60, 68, 2) if (e - 14 + g.mis) % 4 == 0][:1]
    seen = set()
    for e in exts + small:
        if e not in seen and 54 <= e <= avail:
            seen.add(e)
            natural("extent %d" % e, e - 14)
    natural("odd tot_len, pad byte %d" % (ev - 1), ev - 15)
    natural("odd tot_len 55", 55)
    natural("extent %d: one word past avail" % (ev + 2), ev - 12)
    natural("corrupt byte %d of extent %d" % (ev - 3, ev), ev - 14, corrupt_at=ev - 3)
    natural("corrupt byte %d of extent %d" % (ev - 3, ev - 2), ev - 16, corrupt_at=ev - 3)
    natural("no payload", 40)
    for name, src in (("hit", SRC_HIT), ("time_wait", SRC_TW), ("miss", SRC_MISS)):
        out.append((name, make_frame(src=src[0], sport=src[1], seq=7, flags=0x12, payload=_payload(rng, 7)), 47, False))
    # header lengths set by hand: IP options shift the real TCP header (the kernel reads it at ip + 20), TCP options
    for name, kw, plen in (("ihl 6", {"ihl": 6}, 20), ("ihl 15", {"ihl": 15}, 2), ("doff 6", {"doff": 6}, 10),
                           ("doff 15", {"doff": 15}, 0)):
        opts = bytes(rng.integers(1, 256, 40, dtype=np.uint8))
        f = make_frame(payload=_payload(rng, plen), ip_opts=opts, tcp_opts=opts, **kw)
        out.append((name, f, len(f) - 14, False))
    for tot in (0, 19, 20):
        out.append(("tot_len %d" % tot, make_frame(payload=_payload(rng, 30), tot_len=tot), tot, False))
    return tuple(out)


class Case:
    """One launch: the buffer, the offsets, the oracle's records and what the builder knows about each frame."""

    def __init__(self, buf, offsets, eth_mod16, avail, edges, which):
        self.buf, self.offsets, self.eth_mod16, self.avail = buf, offsets, eth_mod16, avail
        self.names = [edges[j][0] for j in which]
        self.tot_len = np.array([edges[j][2] for j in which], np.int64)
        self.corrupt = np.array([edges[j][3] for j in which], bool)
        self.exp = expected(buf, offsets, avail)
        for a in (self.buf, self.offsets, self.exp, self.tot_len, self.corrupt):
            a.setflags(write=False)

    @property
    def n(self):
        return len(self.offsets)

    @property
    def extents(self):
        return np.array([extent(int(t)) for t in self.tot_len], np.int64)

    @property
    def win_phase(self):
        """(win - 16) & 112 for a base on the 128-B grid: which 16-B phase of a line the window block starts at."""
        g = Geometry(self.eth_mod16, self.avail)
        return (self.offsets.astype(np.int64) + 14 - g.mis - 16) & 112


def expected(buf, offsets, avail):
    """The oracle's record of buf[o:o + avail] for every offset, one frame at a time."""
    e, m = conn_entries()
    exp = np.empty(len(offsets), orc.RESULT_DTYPE)
    for i, o in enumerate(offsets):
        o = int(o)
        assert o + avail <= len(buf)
        exp[i] = orc.classify_frame(buf[o:o + avail].tobytes(), avail, e, m, MAX_CONN)
    return exp


@functools.lru_cache(maxsize=None)
def packed(eth_mod16, avail, lead=0, reps=8, drop=0):
    """The edge list `reps` times over (waves mix the edges), frames back to back at the next 16-B boundary plus
    the class, in random bytes; the buffer extends avail bytes past the last Ethernet header.  lead: 16-B chunks
    before the first frame (0: it starts at base + eth_mod16).  drop: frames left off the end (a ragged last wave)."""
    edges = edge_frames(eth_mod16, avail)
    which = (list(range(len(edges))) * reps)[:len(edges) * reps - drop]
    offs, cur = [], 16 * lead
    for j in which:
        offs.append(cur + eth_mod16)
        cur += (eth_mod16 + len(edges[j][1]) + 15) & ~15
    size = (max(offs[-1] + avail, cur) + 31) & ~15
    buf = np.random.default_rng(7 + 16 * avail + eth_mod16).integers(0, 256, size, dtype=np.uint8)
    for o, j in zip(offs, which):
        f = edges[j][1]
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return Case(buf, np.array(offs, np.uint64), eth_mod16, avail, edges, which)


def spaced_stride(avail):
    """The smallest S >= avail + 32 with S % 128 == 16: consecutive frames walk the eight 16-B phases of a line."""
    return avail + 32 + (16 - (avail + 32)) % 128


@functools.lru_cache(maxsize=None)
def spaced(eth_mod16, avail, fill_seed):
    """Frame i at i*S + eth_mod16, each edge 8 times in a row (once per phase).  Each frame owns its whole
    [eth, eth + avail): the frame cut at avail, then bytes that depend on (eth_mod16, avail) only.  Every other
    byte of the buffer comes from fill_seed."""
    edges = edge_frames(eth_mod16, avail)
    which = [j for j in range(len(edges)) for _ in range(8)]
    S = spaced_stride(avail)
    assert S % 128 == 16 and S >= avail + 32
    offs = np.arange(len(which), dtype=np.uint64) * np.uint64(S) + np.uint64(eth_mod16)
    buf = np.random.default_rng(fill_seed).integers(0, 256, len(which) * S + 16, dtype=np.uint8)
    tail = np.random.default_rng(3 + 16 * avail + eth_mod16)
    for j in range(len(edges)):
        img = tail.integers(1, 256, avail, dtype=np.uint8)
        f = np.frombuffer(edges[j][1], np.uint8)[:avail]
        img[:len(f)] = f
        for i in range(8 * j, 8 * j + 8):
            buf[int(offs[i]):int(offs[i]) + avail] = img
    return Case(buf, offs, eth_mod16, avail, edges, which)


@functools.lru_cache(maxsize=None)
def small_slots(stride, frame_off, n=200):
    """n strided slots of random bytes, a frame in each: extents at the slot end, in its last 16 bytes, one word
    past it (TRUNC), odd lengths whose pad byte is the slot's last, small ones, a corrupted byte every 11th."""
    avail = stride - frame_off
    rng = np.random.default_rng(stride * 131 + frame_off)
    slots = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    tots = [avail - 14 - 2 * q for q in range(8)] + [avail - 15, avail - 17, avail - 12, 40, 41, 60, 47]
    for i in range(n):
        tot = tots[i % len(tots)]
        src, sport = SOURCES[i % 3]
        f = bytearray(make_frame(src=src, sport=sport, seq=int(rng.integers(1 << 32)), payload=_payload(rng, tot - 40)))
        if i % 11 == 5:
            f[len(f) - 1 - int(rng.integers(min(12, tot - 40) or 1))] ^= 0x04
        f = f[:avail]
        slots[i, frame_off:frame_off + len(f)] = np.frombuffer(bytes(f), np.uint8)
    slots.setflags(write=False)
    return slots
