"""pn_udp_classify / pn_udp_set_subs through the Python binding, every record bit-exact against
tests/udp_np.py (pinned by tests/test_udp_np.py): all eight alignment classes, the minimum and maximum strides,
batches ending inside a wave, a frame mix that reaches every flag, subscription sets of 1 .. 4096, the release
path, the round trip with the project's own UDP sender fill, zero copy, and the argument errors."""
import numpy as np
import pytest

import pollnet_amd as pa

import udp_np as un

pytestmark = pytest.mark.gpu

GUARD = 0xAB
GROUPS = [un.ip4("239.1.%d.%d" % (i // 8, 10 + i % 8)) for i in range(16)]


def _subs64():
    """64 subscriptions: 16 groups x 4 ports, in a scrambled order (sub_id is the index into this list)."""
    pairs = [(g, 20000 + 7 * p) for g in GROUPS for p in range(4)]
    order = np.random.default_rng(64).permutation(len(pairs))
    return [pairs[i] for i in order]


def _ip_add(ip, d):
    return ((int.from_bytes(ip, "big") + d) & 0xFFFFFFFF).to_bytes(4, "big")


PAYLOAD_LENS = (0, 1, 2, 3, 17, 18, 19, 1471, 1472)


def mixed_ring(seed, n, stride, frame_off, pairs):
    """n slots of random bytes (so garbage follows every datagram), each overwritten with one frame of a rotating
    mix: every even slot a deliverable datagram (valid checksum / checksum 0 / checksum sent as 0xFFFF / lengths
    at the slot's edge), every odd slot one of the defects and strangers below."""
    rng = np.random.default_rng(seed)
    slots = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    avail = stride - frame_off
    room = avail - 42  # payload bytes a slot holds
    lens = [v for v in PAYLOAD_LENS if v <= room]
    if stride >= 4096:  # ulen above 1480: past the stream's two KiBs in the jumbo slots
        lens += [1473, 2200, 3001, room - 7, min(room - 2, 9001)]
    src = un.ip4("10.1.2.3")

    def put(i, plen, dst=None, **kw):
        ip, port = pairs[int(rng.integers(len(pairs)))] if dst is None else dst
        payload = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
        un.put_udp_frame(slots[i], frame_off, payload, src, ip, int(rng.integers(1, 65536)), port, **kw)

    def plen(k, lo=0):
        v = lens[k % len(lens)] if k % 3 else int(rng.integers(lo, min(room, 1472) + 1))
        return max(v, lo)

    def flip(i, off, bit=0x10):
        slots[i, frame_off + off] ^= bit

    good = 0
    odd = 0
    for i in range(n):
        if i % 2 == 0:
            k, good = good, good + 1
            sel = k % 9
            if sel in (0, 1, 2):
                put(i, plen(k // 9 * 3 + sel))
            elif sel == 3:
                put(i, plen(k), udp_csum=0)
            elif sel == 4:
                put(i, plen(k, 2), force_ffff=True)
            elif sel == 5:  # ulen below tot_len - 20: the bytes between are not summed
                p = max(min(plen(k), room - 6), 0)
                put(i, p + 6, ulen=8 + p, tot_len=20 + 8 + p + 6)
            elif sel == 6:  # the datagram ends exactly at the slot's end
                put(i, room)
            elif sel == 7:  # odd length whose pad byte is the slot's last byte
                put(i, room - 1)
            else:  # DF alone is not a fragment
                put(i, plen(k), frag_off=0x4000)
            continue
        k, odd = odd, odd + 1
        sel = k % 27
        p = plen(k, 2)
        if sel == 0:
            put(i, p)
            flip(i, 42)  # first payload byte
        elif sel == 1:
            put(i, p)
            flip(i, 42 + p - 1)  # last payload byte
        elif sel == 2:
            put(i, p)
            flip(i, 35)  # UDP header: source port
        elif sel == 3:
            put(i, p, ulen=8 + p + 2)  # ulen above tot_len - 20
        elif sel == 4:
            put(i, p, ulen=0)
        elif sel == 5:
            put(i, p, ulen=7)
        elif sel == 6:  # ulen one byte past avail (tot_len agrees, so TRUNC alone)
            put(i, room, ulen=avail - 33, tot_len=20 + avail - 33)
        elif sel == 7:
            put(i, p, frag_off=0x2000)  # MF
        elif sel == 8:
            put(i, p, frag_off=0x0001 + int(rng.integers(0, 0x1FFF)))  # a fragment offset
        elif sel == 9:
            put(i, p, ver_ihl=0x46)
        elif sel == 10:
            put(i, p, proto=6)
        elif sel == 11:
            put(i, p, proto=1)
        elif sel == 12:
            put(i, p, ether_type=0x86DD)
        elif sel == 13:
            put(i, p, ether_type=0x8100)
        elif sel == 14:
            put(i, p, ip_csum=0x1234)
        elif sel == 15:
            pass  # random bytes
        elif sel in (16, 17, 18, 19):  # unsubscribed neighbours of a subscription
            ip, port = pairs[int(rng.integers(len(pairs)))]
            dst = [(ip, port + 1), (ip, port - 1), (_ip_add(ip, 1), port), (_ip_add(ip, -1), port)][sel - 16]
            put(i, p, dst=dst)
        elif sel == 20:  # a subscribed ip with another subscription's port + 3 / a subscribed port with a stranger's ip
            put(i, p, dst=(pairs[0][0], pairs[-1][1] + 3))
        elif sel == 21:
            put(i, p, dst=(un.ip4("192.168.7.7"), pairs[0][1]))
        elif sel == 22:
            put(i, p, tot_len=27)
        elif sel == 23:
            put(i, p, ver_ihl=0x65)  # version 6 in an IPv4 ethertype
        elif sel == 24:  # a bad IP checksum on an otherwise unverifiable frame, and a truncated one to nobody
            put(i, room, ulen=avail - 33, tot_len=20 + avail - 33, dst=(un.ip4("192.168.7.7"), 9), ip_csum=1)
        elif sel == 25:
            put(i, p, udp_csum=0, ip_csum=0x4321)  # checksum 0 but a bad header: NOCSUM without IP_OK
        else:
            put(i, p, udp_csum=0xFFFF)  # a wrong checksum that happens to be 0xFFFF
    return slots


LAYOUTS = [(2, 112, 1), (4, 112, 63), (6, 1536, 1000), (8, 2048, 65), (10, 2048, 64), (12, 4096, 130), (14, 128, 257),
           (16, 65536, 200), (0, 2048, 4097)]


def _classify(ctx, slots, stride, frame_off, n, pinned=False):
    import torch

    flat = torch.from_numpy(np.ascontiguousarray(slots).reshape(-1))
    if pinned:
        dev = flat.pin_memory()
        out = torch.full(((n + 9) * 16,), GUARD, dtype=torch.uint8).pin_memory()
    else:
        dev = flat.cuda()
        out = torch.full(((n + 9) * 16,), GUARD, dtype=torch.uint8, device="cuda")
    ctx.udp_classify(dev, stride, frame_off, n, out, torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n * 16:] == GUARD).all(), "wrote past n"
    return got[:n * 16].view(pa.UDP_RESULT_DTYPE).copy()


def _diff(got, exp):
    bad = np.flatnonzero(got != exp)
    return None if len(bad) == 0 else (len(bad), int(bad[0]), got[bad[0]], exp[bad[0]])


@pytest.mark.parametrize("frame_off,stride,n", LAYOUTS)
def test_layouts_bit_exact(frame_off, stride, n):
    pairs = _subs64()
    subs = un.make_subs(pairs)
    slots = mixed_ring(1000 + frame_off, n, stride, frame_off, pairs)
    exp = un.udp_classify_np(slots, stride, frame_off, subs)
    if n >= 63:  # a batch that holds the whole rotation reaches everything (a 1-frame batch cannot)
        fl = exp["flags"]
        for bit in un.ALL_FLAGS:
            if bit != un.UDP_UNCHECKED:  # the release path's flag: test_release_path
                assert (fl & bit).any(), hex(bit)
        chk = fl & (un.UDP_OK | un.NOCSUM)
        assert (chk == un.UDP_OK).any() and (chk == un.NOCSUM).any() and (chk == 0).any()
        d = un.deliver(fl)
        assert 4 * d.sum() >= n and 4 * (~d).sum() >= n, (int(d.sum()), n)
        if stride >= 4096:
            assert (exp["payload_len"][d] > 1480 - 8).any(), "no delivered datagram with ulen above 1480"
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(subs)
    got = _classify(ctx, slots, stride, frame_off, n)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


@pytest.mark.parametrize("kind,frame_off,stride", [("full", 2, 2048), ("full", 0, 2048), ("full", 6, 4096),
                                                   ("sizes", 2, 2048), ("sizes", 8, 4096)])
def test_waves_whose_every_frame_is_summed(kind, frame_off, stride):
    """The mixed rings above put a frame that is not summed into every wave, which always takes the compacting
    form of phase 2.  Here every frame is subscribed and carries a checksum: full-size datagrams (1471 / 1472
    payload bytes: the pipelined form in 2-KiB slots, every load issued in 4-KiB ones) and all sizes (the strided
    skipping form), one frame in five with a flipped payload or header bit so that both verdicts occur."""
    pairs = _subs64()
    subs = un.make_subs(pairs)
    n = 330
    rng = np.random.default_rng(frame_off + stride)
    slots = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    room = stride - frame_off - 42
    for i in range(n):
        if kind == "full":
            plen = 1472 - (i % 3 == 1)
        else:
            plen = int(rng.integers(1, min(room, 3000) + 1)) if i % 4 else (1, 2, 3, 70, 71, room)[i // 4 % 6]
        ip, port = pairs[i % len(pairs)]
        un.put_udp_frame(slots[i], frame_off, rng.integers(0, 256, plen, dtype=np.uint8).tobytes(), un.ip4("10.8.8.8"), ip,
                         2000 + i, port)
        if i % 5 == 2:
            slots[i, frame_off + (42 + int(rng.integers(plen)) if i % 10 == 2 else 34)] ^= 0x01
    exp = un.udp_classify_np(slots, stride, frame_off, subs)
    assert (exp["flags"] & un.MATCH).all() and not (exp["flags"] & (un.NOCSUM | un.LEN_BAD | un.TRUNC)).any()
    ok = (exp["flags"] & un.UDP_OK) != 0
    assert ok.sum() == n - n // 5 and (exp["payload_len"] & 1).any()
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(subs)
    got = _classify(ctx, slots, stride, frame_off, n)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


@pytest.mark.parametrize("kind", ["full", "mixed"])
def test_sixty_four_frame_waves(kind):
    """Batches below 65,536 frames run on waves of 8 .. 32 frames (frames_per_wave); the production shape is 64.
    512 distinct slots repeated to 65,573: every frame full-size and summed (the pipelined form over eight
    batches), and the mixed ring (the compacting form with up to 32 summed frames of 64)."""
    pairs = _subs64()
    subs = un.make_subs(pairs)
    stride, frame_off, base_n, n = 2048, 2, 512, 65536 + 37
    if kind == "mixed":
        base = mixed_ring(64, base_n, stride, frame_off, pairs)
    else:
        rng = np.random.default_rng(6464)
        base = rng.integers(0, 256, (base_n, stride), dtype=np.uint8)
        for i in range(base_n):
            ip, port = pairs[i % len(pairs)]
            un.put_udp_frame(base[i], frame_off, rng.integers(0, 256, 1472 - (i % 3 == 1), dtype=np.uint8).tobytes(),
                             un.ip4("10.8.8.8"), ip, 2000 + i, port)
            if i % 7 == 3:
                base[i, frame_off + 42 + int(rng.integers(1471))] ^= 0x20
    reps = -(-n // base_n)
    slots = np.tile(base, (reps, 1))[:n]
    exp = np.tile(un.udp_classify_np(base, stride, frame_off, subs), reps)[:n]
    assert (exp["flags"] & un.UDP_OK).any() and (un.deliver(exp["flags"]) == 0).any()
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(subs)
    got = _classify(ctx, slots, stride, frame_off, n)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


def _sub_sets():
    rng = np.random.default_rng(4096)
    rnd = set()
    while len(rnd) < 4096:
        rnd.add((bytes(rng.integers(0, 256, 4, dtype=np.uint8)), int(rng.integers(1, 65535))))
    rnd = sorted(rnd)
    rng.shuffle(rnd)
    return {
        "one": [(un.ip4("239.9.9.9"), 31000)],
        "sixty_four": _subs64(),
        "random_4096": [tuple(x) for x in rnd],
        "ports_4096": [(un.ip4("239.1.1.1"), 10000 + k) for k in range(4096)],
        "groups_4096": [(_ip_add(un.ip4("239.2.0.0"), k), 30001) for k in range(4096)],
    }


@pytest.mark.parametrize("name", ["one", "sixty_four", "random_4096", "ports_4096", "groups_4096"])
def test_subscription_sets(name):
    """A frame for every subscription, the unsubscribed neighbours (port +-1, ip +-1) of a sample, same-ip
    wrong-port and same-port wrong-ip frames; small slots, so the table walk is what is tested."""
    pairs = _sub_sets()[name]
    subs = un.make_subs(pairs)
    rng = np.random.default_rng(len(pairs))
    dsts = list(pairs)
    sample = [pairs[i] for i in rng.choice(len(pairs), min(len(pairs), 256), replace=False)] + [pairs[0], pairs[-1]]
    for ip, port in sample:
        dsts += [(ip, port + 1), (ip, port - 1), (_ip_add(ip, 1), port), (_ip_add(ip, -1), port),
                 (ip, (port + 4096 + 77) & 0xFFFF), (un.ip4("172.16.0.9"), port)]
    order = rng.permutation(len(dsts))
    n, stride, frame_off = len(dsts), 128, 2
    slots = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    for i, j in enumerate(order):
        ip, port = dsts[j]
        payload = rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8).tobytes()
        un.put_udp_frame(slots[i], frame_off, payload, un.ip4("10.4.4.4"), ip, 4000 + i % 50000, port & 0xFFFF,
                         udp_csum="valid" if i % 2 else 0)
    exp = un.udp_classify_np(slots, stride, frame_off, subs)
    hit = exp["sub_id"][exp["sub_id"] != un.NO_SUB]
    assert np.array_equal(np.unique(hit), np.arange(len(pairs))), "a subscription without a frame"
    assert (exp["sub_id"] == un.NO_SUB).sum() >= 4
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(subs)
    got = _classify(ctx, slots, stride, frame_off, n)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


def test_set_subs_twice_the_second_applies():
    pairs = _subs64()
    a, b = un.make_subs(pairs), un.make_subs(pairs[::-1][:40] + [(un.ip4("239.7.7.7"), 1)])
    n, stride, frame_off = 300, 2048, 2
    slots = mixed_ring(5, n, stride, frame_off, pairs)
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(a)
    ctx.udp_set_subs(b)  # twice before any launch
    exp_b = un.udp_classify_np(slots, stride, frame_off, b)
    assert _diff(_classify(ctx, slots, stride, frame_off, n), exp_b) is None
    ctx.udp_set_subs(a)  # and between launches
    exp_a = un.udp_classify_np(slots, stride, frame_off, a)
    assert (exp_a["sub_id"] != exp_b["sub_id"]).any()
    assert _diff(_classify(ctx, slots, stride, frame_off, n), exp_a) is None
    ctx.udp_set_subs(b)
    assert _diff(_classify(ctx, slots, stride, frame_off, n), exp_b) is None
    ctx.close()


@pytest.mark.parametrize("frame_off,stride,n", [(2, 2048, 700), (0, 4096, 130)])
def test_release_path(frame_off, stride, n):
    """set_verify(False): the same records, except that where a checksum was due (checkable, field non-zero) the
    verdict is UDP_UNCHECKED: UDP_OK is replaced by it, and a failing checksum gets it too."""
    pairs = _subs64()
    subs = un.make_subs(pairs)
    slots = mixed_ring(77, n, stride, frame_off, pairs)
    ver = un.udp_classify_np(slots, stride, frame_off, subs)
    rel = un.udp_classify_np(slots, stride, frame_off, subs, verify=False)
    ok = (ver["flags"] & un.UDP_OK) != 0
    assert ok.any() and np.array_equal(rel["flags"][ok], (ver["flags"][ok] ^ un.UDP_OK) | un.UDP_UNCHECKED)
    unch = (rel["flags"] & un.UDP_UNCHECKED) != 0
    assert (unch & ~ok).any()  # bad checksums are not told apart on the release path
    assert np.array_equal(rel["flags"][~unch], ver["flags"][~unch])
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(subs)
    ctx.set_verify(False)
    got = _classify(ctx, slots, stride, frame_off, n)
    assert _diff(got, rel) is None, _diff(got, rel)
    ctx.set_verify(True)
    got = _classify(ctx, slots, stride, frame_off, n)
    assert _diff(got, ver) is None, _diff(got, ver)
    ctx.close()


def test_round_trip_with_the_udp_sender_fill():
    """Efvi's sender frames built on the CPU (checksum 0, Efvi.h:611-621), their IPv4 checksum filled on the GPU
    (pn_tx_fill, PN_TX_UDP), then received: every one is delivered, with the length it was sent with."""
    import torch
    from oracle import pyoracle as orc

    n, stride, frame_off = 500, 2048, 14
    slots, lens, _ = orc.tx_build_batch(23, n, stride, frame_off, mode=orc.TX_UDP_EFVI)
    keys = {}
    for i in range(n):
        eth = slots[i, frame_off:]
        keys.setdefault((bytes(eth[30:34]), int.from_bytes(bytes(eth[36:38]), "big")), len(keys))
    subs = un.make_subs(list(keys))
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(subs)
    dev = torch.from_numpy(slots.reshape(-1)).cuda()
    dlens = torch.from_numpy(lens.view(np.int16)).cuda()
    out = torch.full(((n + 4) * 16,), GUARD, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    ctx.tx_fill(dev, stride, frame_off, n, lens=dlens, mode=pa.PN_TX_UDP, stream=s)
    ctx.udp_classify(dev, stride, frame_off, n, out, s)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n * 16:] == GUARD).all()
    rec = got[:n * 16].view(pa.UDP_RESULT_DTYPE)
    assert pa.UF.deliver(rec["flags"]).all(), np.unique(rec["flags"])
    assert (rec["flags"] == (pa.UF.MATCH | pa.UF.IP_OK | pa.UF.NOCSUM)).all()
    assert np.array_equal(rec["payload_len"], lens)
    filled = dev.cpu().numpy().reshape(n, stride)
    assert _diff(rec, un.udp_classify_np(filled, stride, frame_off, subs)) is None
    ctx.close()


def test_zero_copy_pinned_frames_and_results():
    pairs = _subs64()
    subs = un.make_subs(pairs)
    n, stride, frame_off = 257, 2048, 2
    slots = mixed_ring(257, n, stride, frame_off, pairs)
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(subs)
    got = _classify(ctx, slots, stride, frame_off, n, pinned=True)
    exp = un.udp_classify_np(slots, stride, frame_off, subs)
    assert _diff(got, exp) is None, _diff(got, exp)
    ctx.close()


def test_errors_name_themselves_and_launch_nothing():
    import torch

    n, stride = 64, 2048
    dev = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    out = torch.full((n * 16,), GUARD, dtype=torch.uint8, device="cuda")
    ctx = pa.RxContext(0)
    one = un.make_subs([(un.ip4("239.1.1.1"), 5000)])

    def fails(rc, text, fn, *args):
        with pytest.raises(pa.PollnetError) as e:
            fn(*args)
        assert "(%d)" % rc in str(e.value) and text in str(e.value), str(e.value)
        assert text in pa.rx._pn_last_error(ctx._h).decode()

    fails(-4, "pn_udp_set_subs", ctx.udp_classify, dev, stride, 2, n, out)  # PN_ENOTABLE: before set_subs
    dup = un.make_subs([(un.ip4("239.1.1.1"), 5000), (un.ip4("239.1.1.2"), 5000), (un.ip4("239.1.1.1"), 5000)])
    fails(-1, "duplicate subscription", ctx.udp_set_subs, dup)
    padded = one.copy()
    padded["_pad"] = 1
    fails(-1, "_pad", ctx.udp_set_subs, padded)
    fails(-1, "n_subs must be in [1, PN_UDP_MAX_SUBS]", ctx.udp_set_subs, np.zeros(0, pa.UDP_SUB_DTYPE))
    many = un.make_subs([(un.ip4("239.1.1.1"), 1 + k) for k in range(4097)])
    fails(-1, "n_subs must be in [1, PN_UDP_MAX_SUBS]", ctx.udp_set_subs, many)
    fails(-4, "pn_udp_set_subs", ctx.udp_classify, dev, stride, 2, n, out)  # a refused set leaves no table
    ctx.udp_set_subs(one)
    fails(-1, "layout contract", ctx.udp_classify, dev, stride, 3, n, out)  # odd frame_off
    fails(-1, "layout contract", ctx.udp_classify, dev, 96, 2, n, out)  # stride below frame_off + 96
    fails(-1, "layout contract", ctx.udp_classify, dev, 2056, 2, n, out)  # not a multiple of 16
    fails(-1, "16-byte aligned", ctx.udp_classify, dev[8:], stride, 2, n - 1, out)
    ctx.udp_classify(dev, stride, 2, 0, out)  # n == 0: PN_OK, nothing written
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all(), "a refused call launched"
    ctx.close()
