"""Conn tables, lookup keys and waves built to reach every tier of the classify kernels' conn-table probe
(probe_finish, pollnet_amd/csrc/rx_classify.hpp: the home slot, K_AHEAD further entries per lane, then a
wave-cooperative walk of K_WAVE entries per round trip) at every wave width, and subscription sets that give the
UDP probe (udp_probe, udp_classify.hpp) long chains and a chain that wraps.

`find` is findConnEntry in plain Python.  It is the coverage tool -- tests/test_probe_np.py uses it to show what a
batch reaches -- and never the expectation: the GPU tests compare with the C oracle's records.  A frame is built
from its key (connHashKey is a bijection between 48-bit keys and (source ip, source port)), valid in every other
respect, so two records of a batch differ through the probe alone.

Numpy, the oracle and tests/golden/frames.py; pollnet_amd is imported only for the table its own ConnTable builds."""
import functools

import numpy as np

from oracle import pyoracle as orc

import udp_np as un
from frames import make_frame

EMPTY = 1 << 63
PN_MISS = 0xFFFFFFFF
HIT, TW = 0x0004, 0x0008

# ---- the kernel's constants, restated once ----
K_AHEAD, K_WAVE = 2, 64   # probe_finish: entries fetched per lane past the home slot; entries per cooperative round trip
WAVES_FULL = 1024         # frames_per_wave (frame_pass.hpp): a wave's width halves while the batch has fewer waves
SVC_WAVES = 64            # kLatWaves (rx_service.hip): svc_fpw doubles a group while a post has more groups
WIDTHS = (8, 16, 32, 64)


def frames_per_wave(n):
    fpw = 64
    while fpw > 8 and (n + fpw - 1) // fpw < WAVES_FULL:
        fpw >>= 1
    return fpw


def svc_fpw(n, verify):
    fpw = 8 if verify else 64
    while fpw < 64 and (n + fpw - 1) // fpw > SVC_WAVES:
        fpw <<= 1
    return fpw


def width_range(w):
    """(lowest, highest) n at which pn_classify runs w frames per wave (highest None: no limit)."""
    lo = 1 if w == 8 else (WAVES_FULL - 1) * w + 1
    return lo, (None if w == 64 else (WAVES_FULL - 1) * 2 * w)


def batch_sizes(w):
    """Two n of width w: the last wave has 1 live frame, and w - 1."""
    lo, hi = width_range(w)
    if w == 8:  # the top of the range: a batch must hold every wave once
        return hi - (hi - 1) % w, hi - (hi - (w - 1)) % w
    return lo + (1 - lo) % w, lo + (w - 1 - lo) % w


def _depth_classes():
    """The first two and the last two depths each tier and each round trip finds, up to the third round trip."""
    d = [0] + list(range(1, K_AHEAD + 1))
    for r in range(3):
        first = K_AHEAD + 1 + r * K_WAVE
        d += [first, first + 1] + ([first + K_WAVE - 2, first + K_WAVE - 1] if r < 2 else [])
    return tuple(sorted(set(d)))


DEPTHS = _depth_classes()
# run lengths: a run of R ends its misses at depth R, so these put a run's end on each side of every tier boundary
LENGTHS = (1, 2, 3, 4, K_WAVE + 2, K_WAVE + 3, K_WAVE + 4, 2 * K_WAVE + 2, 2 * K_WAVE + 3, 2 * K_WAVE + 4, 200)
END_DEPTHS = tuple(d for d in DEPTHS if d in LENGTHS)


def tier(depth):
    return 1 if depth == 0 else 2 if depth <= K_AHEAD else 3


def round_trip(depth):
    """The cooperative round trip that finds the stop entry (0: tiers 1 and 2)."""
    return 0 if depth <= K_AHEAD else (depth - K_AHEAD - 1) // K_WAVE + 1


# ---- keys and frames ----
def key_to_src(key):
    """Inverse of connHashKey (Core.h:167-172): (dotted ip, host-order port) of a 48-bit key."""
    ip = (key >> 15) & 0xFFFFFFFF
    port = (key & 0x7FFF) | (((key >> 47) & 1) << 15)
    return "%d.%d.%d.%d" % (ip >> 24, (ip >> 16) & 255, (ip >> 8) & 255, ip & 255), port


def src_to_key(ip, port):
    b = bytes(int(x) for x in ip.split("."))
    return orc.conn_hash_key(int.from_bytes(b, "little"), int.from_bytes(port.to_bytes(2, "big"), "little"))


FRAME_W = 64  # bytes a frame's image takes in its slot: the frame (55 .. 63 bytes), then non-zero bytes


@functools.lru_cache(maxsize=None)
def frame_image(key):
    """FRAME_W bytes: a valid IPv4/TCP frame from the key's source, 1 .. 9 payload bytes, random non-zero bytes
    behind it (an odd length's pad byte among them)."""
    ip, port = key_to_src(key)
    rng = np.random.default_rng(key)
    f = make_frame(src=ip, sport=port, seq=int(rng.integers(1 << 32)), payload=rng.integers(1, 256, 1 + key % 9, dtype=np.uint8).tobytes())
    img = rng.integers(1, 255, FRAME_W, dtype=np.uint8)
    img[:len(f)] = np.frombuffer(f, np.uint8)
    return img


def slots_of(images, idx, stride, frame_off):
    """(len(idx), stride) slots: image idx[i] at frame_off, zeros elsewhere."""
    s = np.zeros((len(idx), stride), np.uint8)
    s[:, frame_off:frame_off + images.shape[1]] = images[idx]
    return s


# ---- the model ----
def find(keys, mask, key):
    """findConnEntry bounded at the array end: (e, hit, depth = e - home).  keys: the entries' keys, a list."""
    home = e = key & mask
    n = len(keys)
    while e < n and keys[e] < key:
        e += 1
    return e, e < n and keys[e] == key, e - home


def _run_end(keys, mask, p):
    """How the run entry p lies in ends: 'a' on an EmptyKey, 'b' at the array end, 'c' on another home slot's key."""
    n = len(keys)
    if p >= n:
        return "b"
    if keys[p] == EMPTY:
        return "a"
    h = keys[p] & mask
    while p < n and keys[p] != EMPTY and keys[p] & mask == h:
        p += 1
    return "b" if p == n else "a" if keys[p] == EMPTY else "c"


HI_FIELD = 0x7FFF << 32  # bits 32..46: the high word without the port's top bit
B47 = 1 << 47
LO_FIELD = 0x7FFF        # bits 0..14


def diff_class(a, b):
    x = a ^ b
    if x == B47:
        return "b47"
    if x and x & ~HI_FIELD == 0:
        return "hi"
    if x and x & ~LO_FIELD == 0:
        return "lo"
    return ""


MAX_CONN = 4096
CID_EDGES = (0, MAX_CONN - 1, MAX_CONN, MAX_CONN + 1, 0xFFFFFFFE, 0xFFFFFFFF)


class Table:
    """Entries, mask, max_conn, the lookup keys aimed at it, and the model's verdict on each lookup."""

    def __init__(self, name, entries, mask, max_conn, lookups):
        self.name, self.entries, self.mask, self.max_conn = name, entries, mask, max_conn
        self.keys = [int(k) for k in entries["key"]]
        self.lookups = sorted(set(lookups))
        n = len(self.lookups)
        self.e, self.depth, self.home = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.hit, self.cid = np.zeros(n, bool), np.full(n, PN_MISS, np.uint32)
        self.outcome, self.ending, self.decided = [], [], []
        cids = entries["conn_id"]
        for i, k in enumerate(self.lookups):
            e, hit, d = find(self.keys, mask, k)
            self.e[i], self.hit[i], self.depth[i], self.home[i] = e, hit, d, k & mask
            if hit:
                self.cid[i] = cids[e]
            at_end = e >= len(self.keys) or self.keys[e] == EMPTY or self.keys[e] & mask != k & mask
            self.outcome.append("hit" if hit else "end" if at_end else "larger")
            # how the run ends: for a stop inside a run that run, for a miss at a run's end the way it stopped
            if hit or not at_end:
                self.ending.append(_run_end(self.keys, mask, e))
            else:
                self.ending.append("b" if e >= len(self.keys) else "a" if self.keys[e] == EMPTY else "c")
            # the last entry walked past: the comparison that had to say "smaller" differs from the key in one field
            self.decided.append(diff_class(self.keys[e - 1], k) if d > 0 else "")
        self.tw = self.hit & (self.cid >= max_conn)
        self.images = np.stack([frame_image(k) for k in self.lookups])
        entries.setflags(write=False)


def _compose(home, lo, ipl, hi, band, b47=0):
    assert lo < 32 and ipl < (1 << 17) and hi < 512 and band < 64
    return home | lo << 10 | ipl << 15 | hi << 32 | band << 41 | b47 << 47


D_MASK = 1023  # the designed tables: home = key bits 0..9; bits 10..14 are the `lo` style's field


def _run_keys(home, R, style, band, rng):
    """R ascending keys of one home slot, and the unit that steps between neighbours without leaving the style's
    field.  ip: bits 15..31 differ; hi: only bits 32..40 (equal low words); lo: only bits 10..14 within groups of
    15 (the port's bits 0..14 less the home slot's ten: equal high words); b47: the upper half repeats the lower
    half's last key with bit 47 set, then goes on.  Bits 41..46 hold the run's number, so a run that follows
    another without an EmptyKey between has the larger keys."""
    lo0, ip0, hi0 = int(rng.integers(32)), 4 + 2 * int(rng.integers(1000)), int(rng.integers(100))
    step = 2 * int(rng.integers(1, 40))
    if style == "ip":
        return [_compose(home, lo0, ip0 + step * i, hi0, band) for i in range(R)], 1 << 15
    if style == "hi":
        return [_compose(home, lo0, ip0, 2 + 2 * i, band) for i in range(R)], 1 << 32
    if style == "lo":
        return [_compose(home, 1 + 2 * (i % 15), ip0 + 2 * (i // 15), hi0, band) for i in range(R)], 1 << 10
    m = (R + 1) // 2
    low = [_compose(home, lo0, ip0 + step * i, hi0, band) for i in range(m)]
    return low + [_compose(home, lo0, ip0 + step * (m - 1 + i), hi0, band, 1) for i in range(R - m)], 1 << 15


def _run_lookups(run, unit, extra=()):
    """Hits, misses between neighbours and the miss above the run, at the depth classes the run is long enough for
    (every entry of a short run)."""
    R = len(run)
    idx = set(range(R)) if R <= 8 else {d for d in DEPTHS if d < R} | {R - 1} | {d for d in extra if 0 <= d < R}
    if R > DEPTHS[-1]:  # the longest runs: enough depths for a 64-lane wave to stand at a different one on every lane
        idx |= set(range(0, R, 3))
    out = [run[-1] + unit]
    for i in sorted(idx):
        out.append(run[i])
        between = run[i - 1] + unit if i else run[0] - unit
        assert (run[i - 1] if i else 0) < between < run[i] and between & D_MASK == run[0] & D_MASK
        out.append(between)
    return out


def _cid(counter, i, rot):
    """Boundary conn_ids on the entries the lookups hit (rotated per run), a running number elsewhere."""
    if i in DEPTHS:
        return CID_EDGES[(DEPTHS.index(i) + rot) % len(CID_EDGES)]
    return 5 + counter


STYLES = ("ip", "hi", "lo", "b47")


@functools.lru_cache(maxsize=None)
def designed_table(t):
    """Table t of len(LENGTHS): one run of every length, each at its own home slot, ending on an EmptyKey ('a') or
    on the next home slot's larger key ('c'); then a run of LENGTHS[t] that ends on the array's last entry ('b').
    Styles and endings rotate with t, so over the tables every length meets every ending and style."""
    rng = np.random.default_rng(100 + t)
    L = len(LENGTHS)
    keys, cids, lookups, runs = [], [], [], []

    def add_run(R, style, band, rot):
        home = len(keys)
        assert home <= D_MASK
        run, unit = _run_keys(home, R, style, band, rng)
        assert run == sorted(set(run)) and all(k & D_MASK == home for k in run) and (not keys or keys[-1] == EMPTY or keys[-1] < run[0])
        pivot = (R + 1) // 2 if style == "b47" else -1
        lookups.extend(_run_lookups(run, unit, (pivot,)))
        for i, k in enumerate(run):
            keys.append(k)
            cids.append(_cid(len(keys), i, rot) if i != pivot else 77)
        runs.append((home, R, style))

    for p in range(L):
        R, s = LENGTHS[(p + t) % L], STYLES[(p + 2 * t) % 4]
        add_run(R, s, p + 1, p + t)
        if s in ("hi", "b47"):  # ending 'a'; the others end on the next run's first key
            keys.append(EMPTY)
            cids.append(0)
    R = LENGTHS[t]
    while len(keys) < D_MASK + 1 - R:  # the array must be longer than the mask
        keys.append(EMPTY)
        cids.append(0)
    add_run(R, STYLES[t % 3], L + 1, t)
    # absent keys above every entry whose home slots lie inside the longest run: one group per home slot, each
    # walking to the run's end (and on through the runs that follow without an EmptyKey between)
    start = max(runs, key=lambda r: r[1])[0]
    lookups += [_compose(start + 1 + j, j % 32, j, j, 63, 1) for j in range(K_WAVE + 2)]
    lookups += [int(k) for k in rng.integers(1, 1 << 48, 48)]  # and keys of no design: mostly empty or unmapped home slots
    ent = np.zeros(len(keys), orc.ENTRY_DTYPE)
    ent["key"], ent["conn_id"] = np.array(keys, np.uint64), np.array(cids, np.uint32)
    ent["_pad"] = rng.integers(1, 1 << 32, len(keys))
    return Table("designed%d" % t, ent, D_MASK, MAX_CONN, lookups)


@functools.lru_cache(maxsize=None)
def groups_table():
    """K_WAVE home slots 0 .. 63 of a 128-slot table, five entries each, packed: home slot h's run starts at 5h,
    4h past its home, behind the smaller keys of the slots before it.  One lane per home slot is K_WAVE groups."""
    rng = np.random.default_rng(7)
    keys, cids, lookups = [], [], []
    for h in range(K_WAVE):
        run = [h | (1000 * (h + 1) + 2 * i) << 15 for i in range(5)]
        lookups += _run_lookups(run, 1 << 15)
        keys += run
        cids += [CID_EDGES[(h + i) % len(CID_EDGES)] for i in range(5)]
    keys += [EMPTY] * 8
    cids += [0] * 8
    ent = np.zeros(len(keys), orc.ENTRY_DTYPE)
    ent["key"], ent["conn_id"] = np.array(keys, np.uint64), np.array(cids, np.uint32)
    ent["_pad"] = rng.integers(1, 1 << 32, len(keys))
    return Table("groups", ent, 127, MAX_CONN, lookups)


PRODUCT_CLUSTERS = (140, 70, 6, 3)


@functools.lru_cache(maxsize=None)
def product_table():
    """The product's own layout: pa.ConnTable.add (addConnEntry, expansions included) over four clusters of keys
    that share their low 12 bits, added in a shuffled order."""
    import pollnet_amd as pa

    rng = np.random.default_rng(11)
    runs = [[(0x100 * c + 7) | (5000 * (c + 1) + 2 * i) << 15 for i in range(R)] for c, R in enumerate(PRODUCT_CLUSTERS)]
    flat = [(k, CID_EDGES[(c + i) % 4] if i in DEPTHS else 10 + i) for c, run in enumerate(runs) for i, k in enumerate(run)]
    t = pa.ConnTable(1024, 1024)
    for j in rng.permutation(len(flat)):
        t.add(*flat[int(j)])
    ent, mask = t.snapshot()
    lookups = [int(k) for k in rng.integers(1, 1 << 48, 32)]
    for run in runs:
        lookups += _run_lookups(run, 1 << 15)
    tb = Table("product", ent, mask, t.max_conn_cnt, lookups)
    tb.conn_table = t
    return tb


N_DESIGNED = len(LENGTHS)


def tables():
    return [designed_table(t) for t in range(N_DESIGNED)] + [groups_table(), product_table()]


# ---- waves and batches ----
def _spread(items, w):
    """w of the items, evenly spread, in order (cycling when there are fewer)."""
    if len(items) >= w:
        return [items[(i * (len(items) - 1)) // max(w - 1, 1)] for i in range(w)]
    return sorted((items * (w // len(items) + 1))[:w])


RECIPES = ("ascending", "descending", "same_key", "w_groups", "adjacent_homes", "three_round_trips", "interleaved", "random")


@functools.lru_cache(maxsize=None)
def waves(tb, w):
    """The waves of width w for a table: the recipes, then every lookup of the table in shuffled order.  Lists of
    indices into tb.lookups; {recipe name: wave number}."""
    rng = np.random.default_rng(w)
    by_home = {}
    for i in np.argsort(tb.depth, kind="stable"):
        by_home.setdefault(int(tb.home[i]), []).append(int(i))
    depths = {h: {int(tb.depth[i]) for i in l} for h, l in by_home.items()}
    deep = max(by_home, key=lambda h: (len(depths[h] & set(DEPTHS)), len(depths[h])))  # the longest run's home slot
    own = by_home[deep]
    deep_hits = [i for i in own if tb.hit[i]] or own
    asc = _spread([own[j] for j in sorted({int(tb.depth[i]): n for n, i in enumerate(own)}.values())], w)
    t3 = [i for i in deep_hits if tier(int(tb.depth[i])) == 3] or deep_hits
    far = min(t3, key=lambda i: abs(int(tb.depth[i]) - DEPTHS[-2]))
    # one lookup of tier 3 per home slot, the home slots in order
    per_home = [next(i for i in reversed(by_home[h]) if tb.depth[i] > K_AHEAD) for h in sorted(by_home)
                if tb.depth[by_home[h][-1]] > K_AHEAD]
    homes3 = sorted(int(tb.home[i]) for i in per_home)
    adj = next(((a, b) for a, b in zip(per_home, per_home[1:]) if tb.home[b] == tb.home[a] + 1), (per_home[0], per_home[-1]))
    by_rt = [[i for i in own if round_trip(int(tb.depth[i])) == r] for r in (1, 2, 3)]
    by_rt = [l for l in by_rt if l] or [own]
    zero = [i for i in range(len(tb.lookups)) if tb.hit[i] and tb.depth[i] == 0]
    out = {
        "ascending": asc,
        "descending": asc[::-1],
        "same_key": [far] * w,
        "w_groups": [per_home[(j * max(len(per_home) // w, 1)) % len(per_home)] for j in range(w)],
        "adjacent_homes": [adj[j % 2] for j in range(w)],
        "three_round_trips": [by_rt[j % len(by_rt)][(j // len(by_rt)) % len(by_rt[j % len(by_rt)])] for j in range(w)],
        "interleaved": [zero[(j // 2) % len(zero)] if j % 2 == 0 else far for j in range(w)],
        "random": [int(i) for i in rng.integers(0, len(tb.lookups), w)],
    }
    assert homes3
    ws = [out[r] for r in RECIPES]
    order = [int(i) for i in rng.permutation(len(tb.lookups))]
    order += order[:(-len(order)) % w]
    ws += [order[i:i + w] for i in range(0, len(order), w)]
    return tuple(tuple(x) for x in ws)


@functools.lru_cache(maxsize=None)
def batch_index(tb, w, n):
    """n indices into tb.lookups: the waves of width w once in order (as many as n holds), then again and again
    in shuffled order; the last wave is cut where n ends."""
    ws = waves(tb, w)
    rng = np.random.default_rng(n)
    ids = list(range(len(ws)))
    while len(ids) * w < n:
        ids += [int(i) for i in rng.permutation(len(ws))]
    idx = np.array([i for j in ids for i in ws[j]], np.int64)[:n]
    idx.setflags(write=False)
    return idx


def batch(tb, w, n, stride=128, frame_off=2):
    """(slots, the oracle's records) of the batch."""
    slots = slots_of(tb.images, batch_index(tb, w, n), stride, frame_off)
    exp = orc.classify_batch(slots, stride, frame_off, n, tb.entries, tb.mask, tb.max_conn, threads=8)
    return slots, exp


def release(exp):
    """The verifying records as pn_set_verify(ctx, 0) reports them: no TCP verdicts, PN_F_TCP_UNCHECKED, fold 0xFFFF."""
    r = exp.copy()
    r["flags"] = (r["flags"] & ~np.uint16(0x0002 | 0x0800)) | np.uint16(0x8000)
    r["tcp_fold"] = 0xFFFF
    return r


# ---- the UDP subscription probe ----
def udp_sub_hash(ip, port):
    """udp_sub_hash of udp_classify.hpp on stored (little-endian loaded) values; numpy arrays or ints."""
    m = np.uint64(0xFFFFFFFF)
    x = (np.asarray(ip, np.uint64) ^ (np.asarray(port, np.uint64) * np.uint64(0x9E3779B1))) & m
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x


def udp_table(subs):
    """pn_udp_set_subs's host table: capacity 64 and up, a power of two >= 2 * n_subs; linear insertion that wraps.
    Entry: ip | port << 32 | (sub_id + 1) << 48, 0 empty."""
    cap = 64
    while cap < 2 * len(subs):
        cap <<= 1
    tbl = [0] * cap
    for i, s in enumerate(subs):
        ip, port = int(s["dst_ip"]), int(s["dst_port"])
        e = int(udp_sub_hash(ip, port)) & (cap - 1)
        while tbl[e]:
            e = (e + 1) & (cap - 1)
        tbl[e] = ip | port << 32 | (i + 1) << 48
    return tbl


def udp_walk(tbl, ip, port):
    """udp_probe: (sub_id or NO_SUB, entries read, whether the walk went from the last entry to entry 0)."""
    mask = len(tbl) - 1
    e = int(udp_sub_hash(ip, port)) & mask
    key, wrapped = ip | port << 32, False
    for step in range(len(tbl)):
        if tbl[e] == 0:
            return un.NO_SUB, step + 1, wrapped
        if tbl[e] & 0xFFFFFFFFFFFF == key:
            return (tbl[e] >> 48) - 1, step + 1, wrapped
        wrapped |= e == mask
        e = (e + 1) & mask
    return un.NO_SUB, len(tbl), wrapped


UDP_IP = un.ip4("239.1.2.3")
UDP_HOME_A, UDP_HOME_B = 20, 60  # of a 64-entry table: a chain of 12 inside it, a chain of 10 over its end


@functools.lru_cache(maxsize=None)
def udp_ports_by_home():
    """Host-order ports 1024 .. 65535 of UDP_IP by their home slot in a 64-entry table (brute force)."""
    ports = np.arange(1024, 65536)
    stored = ((ports & 0xFF) << 8) | (ports >> 8)
    h = udp_sub_hash(un.stored_u32(UDP_IP), stored) & np.uint64(63)
    return {s: [int(p) for p in ports[h == np.uint64(s)]] for s in range(64)}


@functools.lru_cache(maxsize=None)
def udp_case(n_subs):
    """(subs, lookups): n_subs = 32 fills a 64-entry table to exactly half, 33 doubles it.  The first 12 pairs share
    home slot 20 of the 64-entry table, the next 10 home slot 60 (entries 60 .. 63, 0 .. 5); the rest are scattered.
    Lookups, as (ip bytes, port): every subscribed pair, unsubscribed pairs of the two crowded home slots, and every
    subscribed pair with one byte of its ip or port changed."""
    by = udp_ports_by_home()
    pairs = [(UDP_IP, p) for p in by[UDP_HOME_A][:12] + by[UDP_HOME_B][:10]]
    pairs += [(UDP_IP, by[s][0]) for s in range(30, 30 + n_subs - 22)]
    assert len(pairs) == n_subs
    subs = un.make_subs(pairs)
    looks = list(pairs) + [(UDP_IP, p) for p in by[UDP_HOME_A][12:20] + by[UDP_HOME_B][10:18]]
    for ip, p in pairs:
        for b in range(4):
            for x in (0x01, 0x80):
                looks.append((bytes(v ^ (x if j == b else 0) for j, v in enumerate(ip)), p))
        looks += [(ip, p ^ 0x0001), (ip, p ^ 0x0080), (ip, p ^ 0x0100), (ip, p ^ 0x8000)]
    return subs, looks


@functools.lru_cache(maxsize=None)
def udp_images(n_subs):
    """One FRAME_W-byte frame image per lookup: a valid datagram to that (ip, port), every third sent without a
    checksum."""
    _, looks = udp_case(n_subs)
    rng = np.random.default_rng(n_subs)
    img = np.zeros((len(looks), FRAME_W), np.uint8)
    for i, (ip, port) in enumerate(looks):
        pay = rng.integers(1, 256, 1 + i % 13, dtype=np.uint8).tobytes()
        un.put_udp_frame(img[i], 0, pay, un.ip4("10.1.%d.%d" % (i >> 8, i & 255)), ip, 30000 + i, port,
                         udp_csum=0 if i % 3 == 2 else "valid")
    return img


def udp_batch(n_subs, n, stride=128, frame_off=2, verify=True):
    """(slots, expected records by the layout-free numpy model) for n frames cycling through the lookups in a
    shuffled order."""
    subs, looks = udp_case(n_subs)
    img = udp_images(n_subs)
    one = un.udp_classify_np(slots_of(img, np.arange(len(looks)), stride, frame_off), stride, frame_off, subs, verify)
    rng = np.random.default_rng(n)
    idx = np.concatenate([rng.permutation(len(looks)) for _ in range(n // len(looks) + 1)])[:n]
    return slots_of(img, idx, stride, frame_off), one[idx]
