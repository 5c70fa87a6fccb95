"""pn_udp_gather through the Python binding: the payload buffer, the four index arrays and the total -- each a
non-constant canary with guard entries around it -- compared whole against tests/udp_gather_np.py (pinned by
tests/test_udp_gather_np.py).  Records come from pn_udp_classify on the same ring where the test is about real
frames, and are written by hand (any 16 bytes are a legal input) where it is about batch shapes and taken patterns."""
import numpy as np
import pytest

import pollnet_amd as pa

import udp_build_np as ub
import udp_gather_np as ug
import udp_np as un
from test_gpu_udp import mixed_ring
from test_udp_build_np import _dest_templates
from udp_gather_dev import G, Gather, canary

pytestmark = pytest.mark.gpu

LENS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1151, 1152, 1153, 1472)
PAIRS = [(un.ip4("239.7.%d.%d" % (i // 8, 30 + i % 8)), 22000 + 3 * p) for i in range(16) for p in range(4)]
SRC = un.ip4("10.7.7.7")
OK = un.MATCH | un.IP_OK | un.UDP_OK


def _ctx():
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(un.make_subs(PAIRS))
    return ctx


def _ring_of(lens, stride, frame_off, seed, over=()):
    """One deliverable datagram of each length per slot, in slots of non-zero random bytes (a non-zero byte after
    every datagram); slots listed in `over` declare one byte more than the slot holds (TRUNC)."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    slots = rng.integers(1, 256, (n, stride), dtype=np.uint8)
    avail = stride - frame_off
    for i, ln in enumerate(lens):
        ip, port = PAIRS[i % len(PAIRS)]
        kw = {"udp_csum": 0} if i % 5 == 3 else {}
        if i in over:
            kw.update(ulen=avail - 33, tot_len=20 + avail - 33)
        un.put_udp_frame(slots[i], frame_off, rng.integers(1, 256, ln, dtype=np.uint8).tobytes(), SRC, ip,
                         1 + i % 60000, port, **kw)
    return slots


def _need(rec, avail):
    return sum(ug.pad16(r["payload_len"]) for r in rec if ug.taken(r, avail))


@pytest.mark.parametrize("frame_off", range(0, 16, 2))
def test_every_length_in_every_alignment_class(frame_off):
    """2-KiB slots: every length of LENS, the largest the slot holds, and one more (TRUNC: not taken), twice over so
    that both the 8-lane and the wave-wide part see each length at two places of a wave.  The eight frame_off classes
    give both source shifts and every 16-byte residue of the source."""
    stride = 2048
    room = stride - frame_off - 42
    lens = list(LENS) + [room, room] + list(LENS[::-1]) + [room]
    over = {len(LENS) + 1}
    slots = _ring_of(lens, stride, frame_off, frame_off, over)
    n = len(lens)
    ctx = _ctx()
    cap = sum(ug.pad16(v) for v in lens)
    g = Gather(slots, n, cap).classify(ctx, stride, frame_off).gather(ctx, stride, frame_off)
    rec = g.host_records()
    assert np.array_equal(rec, un.udp_classify_np(slots, stride, frame_off, un.make_subs(PAIRS)))
    assert un.deliver(rec["flags"]).sum() == n - 1 and rec["flags"][len(LENS) + 1] & un.TRUNC
    total = g.check()
    assert total["n_msgs"] == n - 1 == total["n_fit"] and total["n_bytes"] == cap - ug.pad16(room)
    ctx.close()


@pytest.mark.parametrize("stride,frame_off,lens,over", [
    (16384, 8, (9000, 8999, 9001, 16384 - 8 - 42, 16384 - 8 - 42, 2200, 0, 9000), {4}),
    (65536, 0, (65494, 1, 65493, 65494), {3}),   # 42 + 65,494 = the slot
    (65536, 14, (65480, 65479, 3), ()),
    (112, 0, (70, 69, 0, 70, 54), {3}),          # the smallest slot there is
    (128, 14, (72, 71, 1, 72), {3}),
])
def test_jumbo_and_minimum_slots(stride, frame_off, lens, over):
    slots = _ring_of(lens, stride, frame_off, stride + frame_off, set(over))
    n = len(lens)
    ctx = _ctx()
    g = Gather(slots, n, sum(ug.pad16(v) for v in lens)).classify(ctx, stride, frame_off).gather(ctx, stride, frame_off)
    total = g.check()
    assert total["n_msgs"] == n - len(over)
    ctx.close()


def _hand_records(n, room, take, seed, sub_mod=4096):
    """n records written by hand: frame i delivered iff take[i], lengths 0 .. room at random (every 7th at an edge)."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    lens = rng.integers(0, room + 1, n)
    lens[::7] = np.resize(np.array([0, 1, 15, 16, 17, room - 1, room]), len(lens[::7]))
    rec["sub_id"] = rng.integers(0, sub_mod, n)
    rec["src_ip"] = rng.integers(0, 1 << 32, n)
    rec["src_port"] = rng.integers(0, 1 << 16, n)
    rec["payload_off"] = 42
    rec["payload_len"] = lens
    not_taken = np.array([un.MATCH | un.IP_OK, un.IP_OK | un.NOT_UDP, un.MATCH | un.UDP_OK, 0, un.IP_OK | un.UDP_OK,
                          un.MATCH | un.IP_OK | un.TRUNC | un.LEN_BAD], np.uint16)
    taken = np.array([OK, un.MATCH | un.IP_OK | un.NOCSUM, un.MATCH | un.IP_OK | un.UDP_UNCHECKED], np.uint16)
    rec["flags"] = np.where(take, taken[np.arange(n) % 3], not_taken[np.arange(n) % 6])
    return rec


# 8 frames a wave up to 16,368 frames, 16 up to 32,736, 32 up to 65,472, 64 above.  8,184 / 8,185: 1,023 and 1,024
# waves, the scan's one full pass; 8,193: 1,025 waves, its second pass; 65,573: 64-frame waves, 1,025 of them
@pytest.mark.parametrize("n", [1, 5, 8, 9, 63, 64, 65, 8184, 8185, 8193, 16368, 16369, 32737, 65573])
def test_batch_sizes(n):
    stride, frame_off = 112, 0
    room = stride - 42
    ring = canary(n * stride, n)
    take = np.random.default_rng(n).integers(0, 4, n) != 0
    rec = _hand_records(n, room, take, n)
    need = _need(rec, stride)
    ctx = pa.RxContext(0)  # no table of any kind is needed
    g = Gather(ring, n, need).records(rec).gather(ctx, stride, frame_off)
    total = g.check()
    assert total["n_msgs"] == take.sum() == total["n_fit"]
    ctx.close()


PATTERNS = {
    "every": lambda i, fpw: np.ones_like(i, bool),
    "none": lambda i, fpw: np.zeros_like(i, bool),
    "every_other": lambda i, fpw: i % 2 == 1,
    "one_in_16": lambda i, fpw: i % 16 == 5,
    "only_the_last": lambda i, fpw: i == i[-1],
    "lane_0_of_each_wave": lambda i, fpw: i % fpw == 0,
    "empty_waves_then_a_full_one": lambda i, fpw: (i // fpw) % 5 == 4,
}


@pytest.mark.parametrize("n", [300, 66000])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_taken_patterns(pattern, n):
    """8-frame waves (300 frames) and 64-frame waves (66,000)."""
    stride, frame_off = 128, 6
    fpw = 8 if n < 16369 else 64
    ring = canary(n * stride, 7)
    take = PATTERNS[pattern](np.arange(n), fpw)
    rec = _hand_records(n, stride - frame_off - 42, take, n + len(pattern))
    ctx = pa.RxContext(0)
    g = Gather(ring, n, _need(rec, stride - frame_off) + 64).records(rec).gather(ctx, stride, frame_off)
    total = g.check()
    assert total["n_msgs"] == take.sum()
    if pattern == "none":
        assert tuple(total) == (0, 0, 0)
    ctx.close()


def test_a_mixed_ring_that_reaches_every_flag_and_the_release_path():
    stride, frame_off, n = 2048, 2, 540
    subs = un.make_subs(PAIRS)
    slots = mixed_ring(17, n, stride, frame_off, PAIRS)
    exp = un.udp_classify_np(slots, stride, frame_off, subs)
    rel = un.udp_classify_np(slots, stride, frame_off, subs, verify=False)
    for bit in un.ALL_FLAGS:
        assert ((exp["flags"] | rel["flags"]) & bit).any(), hex(bit)
    ctx = _ctx()
    g = Gather(slots, n, n * 1488).classify(ctx, stride, frame_off).gather(ctx, stride, frame_off)
    assert np.array_equal(g.host_records(), exp)
    total = g.check()
    assert 0 < total["n_msgs"] == un.deliver(exp["flags"]).sum() < n
    # pn_set_verify(ctx, 0): UDP_UNCHECKED frames are taken, those with a wrong checksum among them
    ctx.set_verify(False)
    g = Gather(slots, n, n * 1488).classify(ctx, stride, frame_off).gather(ctx, stride, frame_off)
    assert np.array_equal(g.host_records(), rel)
    total_rel = g.check()
    assert total_rel["n_msgs"] == un.deliver(rel["flags"]).sum() > total["n_msgs"]
    ctx.close()


def test_forged_records_read_and_write_nothing_outside():
    """payload_len past avail, payload_off other than 42, and 16 random bytes as a record: the flags alone take
    nothing, and whatever is taken stays inside its frame and the outputs."""
    stride, frame_off, n = 256, 8, 1200
    avail = stride - frame_off
    ring = canary(n * stride, 4)
    rng = np.random.default_rng(6)
    rec = rng.integers(0, 256, n * 16, dtype=np.uint8).view(un.UDP_RESULT_DTYPE).copy()
    rec["flags"][::2] = OK
    rec["payload_off"][::3] = 42
    rec["payload_len"][::4] = rng.integers(0, avail - 42 + 3, len(rec[::4]))
    rec[0] = (1, 0, 0, 42, avail - 42, OK)       # ends exactly at avail: taken
    rec[1] = (2, 0, 0, 42, avail - 41, OK)       # one byte past it
    rec[2] = (3, 0, 0, 42, 65535, OK)
    rec[3] = (4, 0, 0, 40, 10, OK)
    rec[4] = (5, 0, 0, 44, 10, OK)
    rec[5] = (6, 0, 0, 0, 10, OK)
    tk = np.array([ug.taken(r, avail) for r in rec])
    assert list(tk[:6]) == [True, False, False, False, False, False] and 30 < tk.sum() < n // 2
    ctx = pa.RxContext(0)
    g = Gather(ring, n, _need(rec, avail)).records(rec).gather(ctx, stride, frame_off)
    assert g.check()["n_msgs"] == tk.sum()
    ctx.close()


@pytest.mark.parametrize("short", ["zero", "one_block", "exact", "half", "empty_tail"])
def test_payload_capacity(short):
    """payload_cap 0, one 16-byte block short of the need, exact, and half; the messages past it are indexed, not
    copied, and n_fit counts the prefix that was.  empty_tail: the capacity ends where a message ends and empty
    messages follow (they fit)."""
    stride, frame_off, n = 2048, 8, 300
    room = stride - frame_off - 42
    ring = canary(n * stride, 8)
    rec = _hand_records(n, room, np.arange(n) % 3 != 1, 5)
    if short == "empty_tail":
        rec["payload_len"][150:160] = 0
    need = _need(rec, stride - frame_off)
    cap = {"zero": 0, "one_block": need - 16, "exact": need, "half": (need // 2) & ~15}.get(short)
    if cap is None:
        cap = _need(rec[:150], stride - frame_off)
    ctx = pa.RxContext(0)
    g = Gather(ring, n, cap).records(rec).gather(ctx, stride, frame_off)
    total = g.check()
    assert total["n_bytes"] == need and total["n_msgs"] == 200
    assert (total["n_fit"] == 200) == (short == "exact")
    if short == "one_block":
        assert total["n_fit"] == 199
    if short == "zero":
        assert total["n_fit"] >= 1  # the first message is empty: it fits anywhere
    ctx.close()


def test_everything_in_pinned_memory():
    stride, frame_off, n = 2048, 10, 140
    slots = mixed_ring(31, n, stride, frame_off, PAIRS)
    ctx = _ctx()
    g = Gather(slots, n, n * 1488, pinned=True).classify(ctx, stride, frame_off).gather(ctx, stride, frame_off)
    assert g.check()["n_msgs"] > 40
    ctx.close()


def test_src_index_may_be_null():
    stride, frame_off, n = 512, 4, 500
    ring = canary(n * stride, 9)
    rec = _hand_records(n, stride - frame_off - 42, np.arange(n) % 2 == 0, 9)
    ctx = pa.RxContext(0)
    g = Gather(ring, n, n * 480, src_index=False).records(rec).gather(ctx, stride, frame_off)
    assert g.check()["n_msgs"] == 250
    ctx.close()


def test_two_gathers_back_to_back_on_two_streams():
    """One ctx, one scratch: a call on another stream waits for the one before it on the device; all are right."""
    import torch

    stride, frame_off = 128, 8
    ctx = pa.RxContext(0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    gs = []
    for k, n in enumerate((20000, 900, 20001)):
        rec = _hand_records(n, stride - frame_off - 42, np.arange(n) % 4 != k, 30 + k)
        gs.append(Gather(canary(n * stride, 20 + k), n, _need(rec, stride - frame_off), seed=k).records(rec))
    torch.cuda.synchronize()
    for g, s in zip(gs, (s1, s2, s1)):
        g.gather(ctx, stride, frame_off, s)
    for g in gs:
        g.check()
    ctx.sync()
    ctx.close()


def test_build_classify_gather_build_closes_the_loop():
    """udp_build(CSUM) -> udp_classify -> udp_gather gives the messages back; udp_build again from the gathered arrays
    (chan_ids = sub_ids) gives the same ring."""
    import torch

    stride, frame_off, n, n_ch = 2048, 8, 700, 256
    tmpl, pairs = _dest_templates(n_ch)
    chans = ub.make_channels(tmpl)
    rng = np.random.default_rng(3)
    lens = rng.integers(0, stride - frame_off - 42 + 1, n).astype(np.uint16)
    lens[:len(LENS)] = LENS
    offs = np.cumsum(np.concatenate([[0], lens[:-1].astype(np.int64) + rng.integers(0, 5, n - 1)])).astype(np.uint64)
    src = rng.integers(1, 256, int(offs[-1]) + int(lens[-1]) + 32, dtype=np.uint8)
    ch = rng.integers(0, n_ch, n).astype(np.uint32)
    ctx = pa.RxContext(0)
    ctx.udp_set_channels(chans)
    ctx.udp_set_subs(un.make_subs(pairs))
    cur = torch.cuda.current_stream()
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()  # noqa: E731
    d_src = dev(np.concatenate([src, np.zeros(-len(src) % 16 + 16, np.uint8)]), np.uint8)
    d_offs, d_lens, d_ch = dev(offs, np.int64), dev(lens, np.int16), dev(ch, np.int32)
    ring0 = canary(n * stride, 12)
    g = Gather(ring0, n, sum(ug.pad16(v) for v in lens))
    flens = torch.zeros(n, dtype=torch.int16, device="cuda")
    ctx.udp_build(d_src, len(src), d_offs, d_lens, d_ch, g.frames_ptr(), stride, frame_off, n, pa.PN_UB_CSUM, flens, cur)
    torch.cuda.synchronize()
    built = g.d_buf.cpu().numpy()[G:G + n * stride].copy()
    g.buf = built  # the frames the gather reads
    g.classify(ctx, stride, frame_off).gather(ctx, stride, frame_off)
    total = g.check()
    assert total["n_msgs"] == n == total["n_fit"]
    pay, g_offs, g_lens, g_subs, g_src, _ = g.outputs()
    assert np.array_equal(g_lens[16:16 + n], lens) and np.array_equal(g_subs[16:16 + n], ch)
    for i in (0, 1, 5, 17, n - 1):
        o, at, ln = G + int(g_offs[16 + i]), int(offs[i]), int(lens[i])
        assert np.array_equal(pay[o:o + ln], src[at:at + ln])
    # and back: a second ring built from what the gather wrote
    ring2 = torch.from_numpy(ring0.copy()).cuda()
    flens2 = torch.zeros(n, dtype=torch.int16, device="cuda")
    ctx.udp_build(g.d_pay.data_ptr() + G, int(total["n_bytes"]), g.d_offs.data_ptr() + 128, g.d_lens.data_ptr() + 32,
                  g.d_subs.data_ptr() + 64, ring2, stride, frame_off, n, pa.PN_UB_CSUM, flens2, cur)
    torch.cuda.synchronize()
    assert np.array_equal(ring2.cpu().numpy(), built) and torch.equal(flens, flens2)
    ctx.close()


def test_errors_name_themselves_and_launch_nothing():
    import torch

    stride, frame_off, n = 2048, 8, 64
    ring = canary(n * stride, 1)
    rec = _hand_records(n, 1000, np.ones(n, bool), 1)
    g = Gather(ring, n, n * 1008).records(rec)
    ctx = pa.RxContext(0)
    outs = g._outs()

    def fails(text, **k):
        a = dict(f=g.frames_ptr(), s=stride, o=frame_off, n=n, r=g.d_rec, p=outs[0], c=outs[1], po=outs[2], pl=outs[3],
                 su=outs[4], si=outs[5], t=outs[6])
        a.update(k)
        with pytest.raises(pa.PollnetError) as e:
            ctx.udp_gather(*a.values())
        assert "(-1)" in str(e.value) and "pn_udp_gather" in str(e.value) and text in str(e.value), str(e.value)

    for key in ("f", "r", "p", "po", "pl", "su"):
        fails("NULL", **{key: None})
    fails("NULL total", t=None)
    fails("NULL total", t=None, n=0)
    fails("8-byte", t=outs[6] + 4)
    fails("aligned", f=g.frames_ptr() + 8)
    fails("aligned", r=g.d_rec.data_ptr() + 8)
    fails("aligned", p=outs[0] + 8)
    fails("aligned", c=outs[1] + 8)
    fails("aligned", po=outs[2] + 4)
    fails("aligned", pl=outs[3] + 1)
    fails("aligned", su=outs[4] + 2)
    fails("aligned", si=outs[5] + 2)
    fails("layout contract", o=3)
    fails("layout contract", s=96)
    fails("layout contract", s=2056)
    fails("layout contract", s=65552)
    torch.cuda.synchronize()
    got = g.outputs()
    assert np.array_equal(got[0], g.pay0) and np.array_equal(got[1], g.offs0) and (got[5] == got[5][0]).all(), \
        "a refused call launched"
    # n == 0: PN_OK, the total zeroed on the stream, nothing else written (the other pointers are not looked at)
    ctx.udp_gather(None, 0, 0, 0, None, None, 0, None, None, None, None, outs[6], torch.cuda.current_stream())
    got = g.outputs()
    assert tuple(got[5][1]) == (0, 0, 0) and got[5][0] == got[5][2] and got[5][0]["n_msgs"] == 0x22222222
    assert np.array_equal(got[0], g.pay0) and np.array_equal(got[2], g.lens0)
    g.gather(ctx, stride, frame_off)  # and the ctx still works
    assert g.check()["n_msgs"] == n
    ctx.close()
