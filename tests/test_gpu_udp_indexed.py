"""pn_udp_classify_indexed through the Python binding, every record bit-exact against tests/udp_indexed_np.py (the
gather into a strided twin ring + tests/udp_np.py): pollnet's ef_vi UDP ring driven by RX-event runs, packed
captures in every alignment class, the identity layout against pn_udp_classify on the same GPU, the window forms
(cooperative block / per-lane, avail ending inside the window), the forms of phase 2, out-of-class offsets, the
release path, 4,096 subscriptions, zero copy, and the argument errors."""
import numpy as np
import pytest

import pollnet_amd as pa

import udp_indexed_np as uin
import udp_np as un
from test_gpu_udp import mixed_ring

pytestmark = pytest.mark.gpu

GUARD = 0xAB
SRC = un.ip4("10.6.6.6")
PAIRS = [(un.ip4("239.4.%d.%d" % (i // 8, 20 + i % 8)), 21000 + 5 * p) for i in range(16) for p in range(4)]
STRANGER = (un.ip4("192.168.9.9"), 21000)
ALL_BUT_UNCHECKED = [b for b in un.ALL_FLAGS if b != un.UDP_UNCHECKED]


def _ip_add(ip, d):
    return ((int.from_bytes(ip, "big") + d) & 0xFFFFFFFF).to_bytes(4, "big")


def _expected(base, offsets, eth_mod16, avail, subs, verify=True):
    """The helper's records, computed once per distinct offset (event runs and tiled runs name a frame many times)."""
    uniq, inv = np.unique(np.asarray(offsets, np.uint64), return_inverse=True)
    return uin.udp_classify_indexed_np(base, uniq, eth_mod16, avail, subs, verify)[inv]


def _classify(ctx, base, offsets, eth_mod16, avail, pinned=False, dev=None):
    """Records of one launch; the canary after record n is checked.  dev: a device copy of base to reuse."""
    import torch

    n = len(offsets)
    offs = torch.from_numpy(np.ascontiguousarray(offsets, np.uint64).view(np.int64))
    if dev is None:
        dev = torch.from_numpy(np.ascontiguousarray(base).reshape(-1))
        dev = dev.pin_memory() if pinned else dev.cuda()
    if pinned:
        offs = offs.pin_memory()
        out = torch.full(((n + 9) * 16,), GUARD, dtype=torch.uint8).pin_memory()
    else:
        offs = offs.cuda()
        out = torch.full(((n + 9) * 16,), GUARD, dtype=torch.uint8, device="cuda")
    ctx.udp_classify_indexed(dev, offs, eth_mod16, n, avail, out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n * 16:] == GUARD).all(), "wrote past record n"
    return got[:n * 16].view(pa.UDP_RESULT_DTYPE).copy()


def _diff(got, exp):
    bad = np.flatnonzero(got != exp)
    return None if len(bad) == 0 else (len(bad), int(bad[0]), got[bad[0]], exp[bad[0]])


def _ctx(subs):
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(subs)
    return ctx


def _frame(rng, plen, dst=None, **kw):
    """One frame as bytes: 42 + plen, padded with zeros to the Ethernet minimum of 60."""
    ip, port = PAIRS[int(rng.integers(len(PAIRS)))] if dst is None else dst
    slot = np.zeros(max(42 + plen, 60), np.uint8)
    un.put_udp_frame(slot, 0, rng.integers(0, 256, plen, dtype=np.uint8).tobytes(), SRC, ip, int(rng.integers(1, 65536)),
                     port, **kw)
    return slot


def _mixed_frames(rng, count, avail, jumbo_every=0):
    """A rotation of deliverable datagrams and of every defect, 60 .. 1514 B (and a 9,000-B one now and then)."""
    out = []
    for i in range(count):
        k = i % 16
        plen = int(rng.integers(0, 1473))
        if k == 0:
            f = _frame(rng, plen)
        elif k == 1:
            f = _frame(rng, plen, udp_csum=0)
        elif k == 2:
            f = _frame(rng, plen | 1)
        elif k == 3:
            f = _frame(rng, max(plen, 1))
            f[42 + int(rng.integers(max(plen, 1)))] ^= 0x08  # a payload bit
        elif k == 4:
            ip, port = PAIRS[int(rng.integers(len(PAIRS)))]
            f = _frame(rng, plen, dst=[(ip, port + 1), (_ip_add(ip, 1), port), STRANGER][i // 16 % 3])
        elif k == 5:
            f = _frame(rng, plen, ulen=8 + plen + 2)
        elif k == 6:
            f = _frame(rng, plen, frag_off=0x2000 if i & 16 else 0x0007)
        elif k == 7:
            f = _frame(rng, plen, ver_ihl=0x46)
        elif k == 8:
            f = _frame(rng, plen, proto=6)
        elif k == 9:
            f = _frame(rng, plen, ether_type=0x86DD)
        elif k == 10:
            f = _frame(rng, plen, ip_csum=0x1234)
        elif k == 11:  # the declared datagram ends one byte past avail
            f = _frame(rng, plen, ulen=avail - 33, tot_len=20 + avail - 33)
        elif k == 12:
            f = _frame(rng, max(plen, 2), force_ffff=True)
        elif k == 13:
            f = _frame(rng, (0, 1, 2, 3, 17, 18)[i // 16 % 6])
        elif k == 14:
            f = _frame(rng, 8958 if jumbo_every and i // 16 % jumbo_every == 0 else 1472 - (i & 16) // 16)
        else:
            f = _frame(rng, plen, udp_csum=0xFFFF)  # a wrong checksum that happens to be 0xFFFF
        out.append(f)
    return out


def _pack(rng, frames, eth_mod16, avail, lead=0):
    """Frames back to back, each rounded up to 16 B plus the class, in random bytes; the buffer extends avail bytes
    past the last Ethernet header.  lead: 16-B chunks before the first frame (0: it starts at eth_mod16 exactly)."""
    offs, cur = [], 16 * lead
    for f in frames:
        offs.append(cur + eth_mod16)
        cur += (eth_mod16 + len(f) + 15) & ~15
    size = (offs[-1] + avail + 31) & ~15
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    for o, f in zip(offs, frames):
        buf[o:o + len(f)] = f
    return buf, np.array(offs, np.uint64)


def _coverage(flags, bits):
    for bit in bits:
        assert (flags & bit).any(), hex(bit)
    d = un.deliver(flags)
    assert d.any() and (~d).any()


def _event_ids(rng, n, bufs=511):
    """RX event ids in ring order over several laps: every 7th buffer discarded, some reposted and named again."""
    ids, i = [], int(rng.integers(bufs))
    while len(ids) < n:
        if i % 7 != 3:
            ids.append(i % bufs)
            if rng.integers(30) == 0:
                ids.append(i % bufs)
        i += 1
    return np.array(ids[:n], np.uint64)


@pytest.mark.parametrize("prefix", [0, 2, 14])
def test_event_ring(prefix):
    """pollnet's ef_vi UDP ring (511 x 2,048 B, the frame at 64 + prefix) and 1,300 events that wrap it; verifying and
    release launches, which together reach every flag."""
    subs = un.make_subs(PAIRS)
    frame_off, stride, bufs, n = 64 + prefix, 2048, 511, 1300
    avail = stride - frame_off
    ring = mixed_ring(500 + prefix, bufs, stride, frame_off, PAIRS)
    ids = _event_ids(np.random.default_rng(prefix), n)
    assert len(np.unique(ids)) < bufs and (np.diff(ids.astype(np.int64)) < 0).sum() >= 2 and (np.diff(ids) == 0).any()
    offsets = ids * np.uint64(stride) + np.uint64(frame_off)
    exp = _expected(ring, offsets, frame_off % 16, avail, subs)
    rel = _expected(ring, offsets, frame_off % 16, avail, subs, verify=False)
    assert np.array_equal(exp, un.udp_classify_np(ring, stride, frame_off, subs)[ids.astype(np.int64)])
    _coverage(exp["flags"], ALL_BUT_UNCHECKED)
    _coverage(rel["flags"], [un.UDP_UNCHECKED])
    ctx = _ctx(subs)
    got = _classify(ctx, ring, offsets, frame_off % 16, avail)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.set_verify(False)
    got = _classify(ctx, ring, offsets, frame_off % 16, avail)
    assert _diff(got, rel) is None, _diff(got, rel)
    ctx.close()


@pytest.mark.parametrize("eth_mod16,n", [(0, 700), (2, 700), (6, 700), (14, 700)] + [(c, 130) for c in range(0, 16, 2)])
def test_packed_capture(eth_mod16, n):
    subs = un.make_subs(PAIRS)
    rng = np.random.default_rng(900 + eth_mod16 + n)
    avail = 9216
    buf, offsets = _pack(rng, _mixed_frames(rng, n, avail, jumbo_every=2), eth_mod16, avail)
    gaps = np.diff(offsets.astype(np.int64))
    assert gaps.min() >= 64 and gaps.max() >= 9000 and (offsets % 16 == eth_mod16).all()
    exp = _expected(buf, offsets, eth_mod16, avail, subs)
    _coverage(exp["flags"], ALL_BUT_UNCHECKED)
    assert (exp["payload_len"][un.deliver(exp["flags"])] > 8000).any(), "no delivered jumbo datagram"
    ctx = _ctx(subs)
    got = _classify(ctx, buf, offsets, eth_mod16, avail)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


@pytest.mark.parametrize("frame_off,stride,n", [(2, 2048, 300), (0, 112, 130), (14, 128, 257), (6, 4096, 130)])
def test_identity_layout_equals_the_strided_entry_point(frame_off, stride, n):
    import torch

    subs = un.make_subs(PAIRS)
    slots = mixed_ring(40 + frame_off, n, stride, frame_off, PAIRS)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(frame_off)
    exp = un.udp_classify_np(slots, stride, frame_off, subs)
    assert np.array_equal(_expected(slots, offsets, frame_off % 16, stride - frame_off, subs), exp)
    _coverage(exp["flags"], ALL_BUT_UNCHECKED)
    ctx = _ctx(subs)
    dev = torch.from_numpy(slots.reshape(-1)).cuda()
    out = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    ctx.udp_classify(dev, stride, frame_off, n, out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    strided = out.cpu().numpy().view(pa.UDP_RESULT_DTYPE)
    got = _classify(ctx, slots, offsets, frame_off % 16, stride - frame_off, dev=dev)
    assert _diff(got, strided) is None, _diff(got, strided)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


@pytest.mark.parametrize("eth_mod16", [0, 2, 8, 14])
@pytest.mark.parametrize("avail", [96, 98, 100, 111, 112, 126, 128, 2048])
def test_window_forms(eth_mod16, avail):
    """The cooperative window block needs it inside [base, eth + avail): 14 - MIS + 112 <= avail and 16 B before the
    window at or above base.  40 frames in waves of 8: with avail below that bound every wave loads per lane, and
    avail ends inside the window -- datagrams that end exactly at avail, two bytes before it and one byte past it
    are there.  With avail above it the first wave holds the frame at offset eth_mod16 exactly (for class 0 its
    block would start below base: that wave loads per lane), the other waves take the cooperative form."""
    subs = un.make_subs(PAIRS)
    rng = np.random.default_rng(avail * 16 + eth_mod16)
    room = min(avail, 1514) - 42
    plens = [room, room - 1, room - 2, room - 3, room + 1, 0, 1, 54, 53, 30]
    frames = []
    for i in range(40):
        p = plens[i % len(plens)]
        if p > room:  # declared to end one byte past avail
            frames.append(_frame(rng, room, ulen=avail - 33, tot_len=20 + avail - 33))
        else:
            frames.append(_frame(rng, p, **({"udp_csum": 0} if i % 7 == 5 else {})))
    buf, offsets = _pack(rng, frames, eth_mod16, avail)
    assert offsets[0] == eth_mod16
    exp = _expected(buf, offsets, eth_mod16, avail, subs)
    fl = exp["flags"]
    ends = 34 + ((exp["payload_len"].astype(np.int64) + 8 + 1) & ~1)
    ok = (fl & un.UDP_OK) != 0
    assert (fl & un.TRUNC).any() and (ok & (exp["payload_len"] & 1 == 1)).any() and (fl & un.NOCSUM).any()
    if avail < 1514:  # verified datagrams whose last summed word is avail's last, and the one before it
        assert (ok & (ends >= avail - 1)).any() and (ok & (ends == (avail & ~1) - 2)).any()
    ctx = _ctx(subs)
    got = _classify(ctx, buf, offsets, eth_mod16, avail)
    assert _diff(got, exp) is None, _diff(got, exp)
    # the same frames behind one 16-B chunk: no block starts below base
    buf2, offsets2 = _pack(rng, frames, eth_mod16, avail, lead=1)
    exp2 = _expected(buf2, offsets2, eth_mod16, avail, subs)
    assert np.array_equal(exp2, exp)
    got = _classify(ctx, buf2, offsets2, eth_mod16, avail)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


def _summed_frames(rng, count, kind):
    out = []
    for i in range(count):
        if kind == "full":
            plen = 1472 - (i % 3 == 1)
        elif kind == "sizes":
            plen = int(rng.integers(1, 1473)) if i % 4 else (1, 2, 3, 70, 71, 1472)[i // 4 % 6]
        elif kind == "jumbo":
            plen = (8958, 3001, 2200, 1473)[i % 4]
        else:
            plen = int(rng.integers(0, 1473))
        if kind == "none":  # subscribed without a checksum, or for somebody else
            f = _frame(rng, plen, **({"udp_csum": 0} if i % 2 else {"dst": STRANGER}))
        else:
            f = _frame(rng, plen)
            if i % 5 == 2:  # one in five fails: a payload bit, or one of the source port
                f[(42 + int(rng.integers(plen))) if i % 10 == 2 else 34] ^= 0x01
        out.append(f)
    return out


@pytest.mark.parametrize("kind", ["full", "sizes", "jumbo", "none", "mixed"])
@pytest.mark.parametrize("n", [5, 100])
def test_phase2_forms(kind, n):
    """Waves whose every frame is summed and full size (every load issued), every frame summed with short ones (the
    skipping form), datagrams past the stream's two KiBs, waves with no summed frame (nothing streamed) and a mix
    with few summed frames per wave (compacted); a batch inside one wave and one of several waves."""
    subs = un.make_subs(PAIRS)
    rng = np.random.default_rng(n + len(kind))
    eth_mod16, avail = (2, 2048) if kind != "jumbo" else (10, 9216)
    frames = _mixed_frames(rng, n, avail) if kind == "mixed" else _summed_frames(rng, n, kind)
    buf, offsets = _pack(rng, frames, eth_mod16, avail, lead=1)
    exp = _expected(buf, offsets, eth_mod16, avail, subs)
    summed = ((exp["flags"] & (un.MATCH | un.LEN_BAD | un.TRUNC | un.NOCSUM)) == un.MATCH)
    if kind == "none":
        assert not summed.any() and un.deliver(exp["flags"]).any()
    elif kind == "mixed":
        assert 0 < summed.sum() < n
    else:
        assert summed.all() and (exp["flags"] & un.UDP_OK != 0).sum() == n - len(range(2, n, 5))
        assert n < 100 or (exp["payload_len"] & 1).any()
    ctx = _ctx(subs)
    got = _classify(ctx, buf, offsets, eth_mod16, avail)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


@pytest.mark.parametrize("n", [20000, 65573])
def test_many_small_frames(n):
    """512 distinct frames of 96 .. 200 B, packed, named n times: 16-frame waves at 20,000 and 64-frame waves at
    65,573.  The first 4,096 offsets name summed frames only, the next 4,096 frames that are not summed, the rest
    any: all three shapes of a wave at both sizes."""
    subs = un.make_subs(PAIRS)
    rng = np.random.default_rng(n)
    frames = []
    for i in range(512):
        plen = int(rng.integers(96 - 42, 200 - 42 + 1))
        kw = [{}, {}, {"udp_csum": 0}, {"dst": STRANGER}][i % 4]
        frames.append(_frame(rng, plen, **kw))
        if i % 8 == 1:
            frames[-1][42 + int(rng.integers(plen))] ^= 0x40
    eth_mod16, avail = 4, 256
    buf, base_offs = _pack(rng, frames, eth_mod16, avail, lead=1)
    base_exp = uin.udp_classify_indexed_np(buf, base_offs, eth_mod16, avail, subs)
    summed = np.flatnonzero((base_exp["flags"] & (un.MATCH | un.NOCSUM)) == un.MATCH)
    rest = np.flatnonzero((base_exp["flags"] & (un.MATCH | un.NOCSUM)) != un.MATCH)
    assert len(summed) == 256 and (base_exp["flags"][summed] & un.UDP_OK != 0).sum() == 192
    pick = np.concatenate([rng.choice(summed, 4096), rng.choice(rest, 4096), rng.integers(0, 512, n - 8192)])
    offsets, exp = base_offs[pick], base_exp[pick]
    ctx = _ctx(subs)
    got = _classify(ctx, buf, offsets, eth_mod16, avail)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


def test_out_of_class_offsets_get_the_badoff_record():
    """A tenth of the offsets scattered outside the class: another class, or far outside the buffer (none of their
    bytes is read).  Exactly the BADOFF record there, every neighbour as without them, the canary untouched."""
    subs = un.make_subs(PAIRS)
    frame_off, stride, bufs, n = 66, 2048, 511, 1000
    ring = mixed_ring(66, bufs, stride, frame_off, PAIRS)
    rng = np.random.default_rng(10)
    offsets = _event_ids(rng, n) * np.uint64(stride) + np.uint64(frame_off)
    clean = _expected(ring, offsets, 2, stride - frame_off, subs)
    bad = np.zeros(n, bool)
    bad[rng.choice(n, n // 10, replace=False)] = True
    bad[[0, 63, 64, n - 1]] = True
    stray = offsets.copy()
    for j, i in enumerate(np.flatnonzero(bad)):
        stray[i] = offsets[i] + np.uint64(2 * (1 + j % 7)) if j % 3 else np.uint64((1 << 44) + 16 * j + 2 * (2 + j % 7))
    assert ((stray[bad] % 16) != 2).all() and len(set((stray[bad] % 16).tolist())) == 7
    exp = _expected(ring, stray, 2, stride - frame_off, subs)
    assert (exp[bad] == uin.badoff_record()).all() and np.array_equal(exp[~bad], clean[~bad])
    assert not (clean["flags"] & uin.BADOFF).any()
    ctx = _ctx(subs)
    got = _classify(ctx, ring, stray, 2, stride - frame_off)
    assert _diff(got, exp) is None, _diff(got, exp)
    for verify in (False, True):  # and a batch of nothing but strays, on both kernels
        ctx.set_verify(verify)
        got = _classify(ctx, ring, stray[bad], 2, stride - frame_off)
        assert (got == uin.badoff_record()).all()
    ctx.close()


@pytest.mark.parametrize("eth_mod16,n", [(2, 700), (0, 130)])
def test_release_path(eth_mod16, n):
    """set_verify(False): where a sum was due the verdict is UDP_UNCHECKED, every other record as when verifying."""
    subs = un.make_subs(PAIRS)
    rng = np.random.default_rng(77 + eth_mod16)
    avail = 2048
    buf, offsets = _pack(rng, _mixed_frames(rng, n, avail), eth_mod16, avail)
    ver = _expected(buf, offsets, eth_mod16, avail, subs)
    rel = _expected(buf, offsets, eth_mod16, avail, subs, verify=False)
    ok = (ver["flags"] & un.UDP_OK) != 0
    unch = (rel["flags"] & un.UDP_UNCHECKED) != 0
    assert ok.any() and (unch & ~ok).any() and np.array_equal(rel["flags"][~unch], ver["flags"][~unch])
    assert np.array_equal(rel["flags"][ok], (ver["flags"][ok] ^ un.UDP_OK) | un.UDP_UNCHECKED)
    ctx = _ctx(subs)
    ctx.set_verify(False)
    got = _classify(ctx, buf, offsets, eth_mod16, avail)
    assert _diff(got, rel) is None, _diff(got, rel)
    ctx.set_verify(True)
    got = _classify(ctx, buf, offsets, eth_mod16, avail)
    assert _diff(got, ver) is None, _diff(got, ver)
    ctx.close()


def test_4096_subscriptions_and_their_neighbours():
    rng = np.random.default_rng(4096)
    pairs = set()
    while len(pairs) < 4096:
        pairs.add((bytes(rng.integers(0, 256, 4, dtype=np.uint8)), int(rng.integers(1, 65535))))
    pairs = sorted(pairs)
    rng.shuffle(pairs)
    pairs = [tuple(p) for p in pairs]
    subs = un.make_subs(pairs)
    dsts = list(pairs)
    for i in rng.choice(len(pairs), 256, replace=False):
        ip, port = pairs[i]
        dsts += [(ip, port + 1), (ip, port - 1), (_ip_add(ip, 1), port), (_ip_add(ip, -1), port)]
    frames = []
    for i, j in enumerate(rng.permutation(len(dsts))):
        ip, port = dsts[j]
        frames.append(_frame(rng, int(rng.integers(0, 60)), dst=(ip, port & 0xFFFF), **({} if i % 2 else {"udp_csum": 0})))
    eth_mod16, avail = 12, 128
    buf, offsets = _pack(rng, frames, eth_mod16, avail)
    order = rng.permutation(len(offsets))  # and not in memory order
    exp = uin.udp_classify_indexed_np(buf, offsets, eth_mod16, avail, subs)[order]
    hit = exp["sub_id"][exp["sub_id"] != un.NO_SUB]
    assert np.array_equal(np.unique(hit), np.arange(4096)) and (exp["sub_id"] == un.NO_SUB).sum() >= 1000
    ctx = _ctx(subs)
    got = _classify(ctx, buf, offsets[order], eth_mod16, avail)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


def test_zero_copy_pinned_base_offsets_and_results():
    subs = un.make_subs(PAIRS)
    frame_off, stride, bufs, n = 64, 2048, 511, 600
    ring = mixed_ring(64, bufs, stride, frame_off, PAIRS)
    offsets = _event_ids(np.random.default_rng(3), n) * np.uint64(stride) + np.uint64(frame_off)
    exp = _expected(ring, offsets, 0, stride - frame_off, subs)
    _coverage(exp["flags"], ALL_BUT_UNCHECKED)
    ctx = _ctx(subs)
    got = _classify(ctx, ring, offsets, 0, stride - frame_off, pinned=True)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


def test_errors_name_the_function_and_launch_nothing():
    import torch

    n, avail = 64, 2048
    dev = torch.zeros(n * 2048 + 4096, dtype=torch.uint8, device="cuda")
    offs = (torch.arange(n, dtype=torch.int64) * 2048 + 2).cuda()
    out = torch.full((n * 16 + 16,), GUARD, dtype=torch.uint8, device="cuda")
    ctx = pa.RxContext(0)

    def fails(rc, text, *args):
        with pytest.raises(pa.PollnetError) as e:
            ctx.udp_classify_indexed(*args)
        assert "(%d)" % rc in str(e.value) and "pn_udp_classify_indexed" in str(e.value) and text in str(e.value), str(e.value)
        assert text in pa.rx._pn_last_error(ctx._h).decode()

    fails(-4, "pn_udp_set_subs", dev, offs, 2, n, avail, out)  # PN_ENOTABLE: before set_subs
    ctx.udp_set_subs(un.make_subs(PAIRS[:1]))
    fails(-1, "NULL buffer", None, offs, 2, n, avail, out)
    fails(-1, "NULL buffer", dev, None, 2, n, avail, out)
    fails(-1, "NULL buffer", dev, offs, 2, n, avail, None)
    fails(-1, "16-byte", dev[8:], offs, 2, n, avail, out)
    fails(-1, "16-byte", dev, offs, 2, n, avail, out[8:])
    fails(-1, "eth_mod16 must be even < 16", dev, offs, 3, n, avail, out)
    fails(-1, "eth_mod16 must be even < 16", dev, offs, 16, n, avail, out)
    fails(-1, "avail in [96, 65536]", dev, offs, 2, n, 95, out)
    fails(-1, "avail in [96, 65536]", dev, offs, 2, n, 65537, out)
    ctx.udp_classify_indexed(dev, offs, 2, 0, avail, out)  # n == 0: PN_OK, nothing written
    ctx.udp_classify_indexed(None, None, 2, 0, avail, None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all(), "a refused call launched"
    ctx.close()
