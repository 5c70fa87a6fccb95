"""pn_udp_demux through the Python binding: the payload buffer, the four per-message arrays, the two
per-subscription arrays and the total -- each a non-constant canary with guard entries around it -- compared whole
against tests/udp_demux_np.py (pinned by tests/test_udp_demux_np.py).  Records come from pn_udp_classify on the same
ring where the test is about real frames, and are written by hand (any 16 bytes are a legal input) where it is about
batch shapes and key patterns."""
import numpy as np
import pytest

import pollnet_amd as pa

import udp_build_np as ub
import udp_demux_np as ud
import udp_gather_np as ug
import udp_np as un
from test_gpu_udp import mixed_ring
from test_gpu_udp_gather import LENS, PAIRS, _ring_of
from test_udp_build_np import _dest_templates
from test_udp_demux_np import CAP_CASES, argsort_identity, capacity_case, random_records
from udp_demux_dev import G, GE, Demux, canary
from udp_gather_dev import Gather

pytestmark = pytest.mark.gpu

OK = un.MATCH | un.IP_OK | un.UDP_OK
# The launch plan's constants (pollnet_amd/csrc/udp_demux.hpp: kUdMinTile, kUdMaxTiles, kUdChunk, kUdScanThreads)
TILE_MIN, MAX_TILES, CHUNK, SCAN_PASS, WAVE = 256, 1024, 256, 1024, 64
COLS_UNROLL = 8  # tiles the cols kernel loads together


def _ctx():
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(un.make_subs(PAIRS))
    return ctx


def _need(rec, avail, n_subs):
    tk = (un.deliver(rec["flags"]).astype(bool) & (rec["payload_off"] == 42) &
          (42 + rec["payload_len"].astype(np.int64) <= avail) & (rec["sub_id"] < n_subs))
    return int(((rec["payload_len"][tk].astype(np.int64) + 15) // 16 * 16).sum()), int(tk.sum())


def _run(n, n_subs, rec, stride=112, frame_off=0, cap=None, seed=0, fast=False, **kw):
    ring = canary(n * stride, seed + 1)
    need, msgs = _need(rec, stride - frame_off, n_subs)
    ctx = pa.RxContext(0)  # no table of any kind is needed
    d = Demux(ring, n, need if cap is None else cap, n_subs, fast=fast, **kw).records(rec)
    d.demux(ctx, stride, frame_off)
    total = d.check()
    assert total["n_msgs"] == msgs and total["n_bytes"] == need
    ctx.close()
    return total


# one tile / two; 7, 8 and 9 tiles around the cols kernel's unrolled step; a chunk of the offset scan and one more
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE_MIN - 1, TILE_MIN, TILE_MIN + 1, CHUNK * 2 + 1,
                               TILE_MIN * (COLS_UNROLL - 1), TILE_MIN * (COLS_UNROLL - 1) + 1,
                               TILE_MIN * COLS_UNROLL, TILE_MIN * COLS_UNROLL + 1, 5000])
def test_batch_sizes(n):
    rec = random_records(n, 70, 40, n)
    total = _run(n, 37, rec, seed=n)  # ids 37, 38, 39 are skipped
    assert total["n_fit"] == total["n_msgs"]


@pytest.mark.parametrize("n", [TILE_MIN * MAX_TILES - 1, TILE_MIN * MAX_TILES, TILE_MIN * MAX_TILES + 1])
def test_the_edge_where_the_tile_grows_and_the_scan_takes_a_second_pass(n):
    """262,144 frames: the last batch with 256-frame tiles (1,024 of them) and with one pass of the offset scan
    (1,024 chunks); one more frame: 320-frame tiles and a second pass.  112-byte slots, the vectorised model."""
    assert (n - 1) // CHUNK + 1 in (SCAN_PASS, SCAN_PASS + 1)
    rec = random_records(n, 70, 700, 3, take=0.9)
    total = _run(n, 512, rec, seed=2, fast=True)
    assert total["n_fit"] == total["n_msgs"] > n // 2


@pytest.mark.parametrize("n_subs", [1, 2, 63, 64, 65, 1024, 4095, 4096])
def test_subscription_counts(n_subs):
    n = 3000
    rec = random_records(n, 70, n_subs + 2, n_subs)
    rec["sub_id"][5] = n_subs - 1
    rec["sub_id"][6] = 0
    _run(n, n_subs, rec, seed=n_subs)


def _pattern(name, n, n_subs):
    i = np.arange(n)
    sub, take = np.zeros(n, np.int64), np.ones(n, bool)
    if name == "one_subscription":
        sub[:] = 5
    elif name == "distinct_64_in_64":
        sub = (i * 7) % 64 + 64 * ((i // 64) % 3)
    elif name == "two_alternating":
        sub = np.where(i % 2 == 0, 900, 3)
    elif name == "only_in_the_last_frame":
        sub = i % 50
        sub[-1] = 777
    elif name == "only_in_lane_0_of_each_wave":
        sub = np.where(i % WAVE == 0, 321, 1 + i % 9)
    elif name == "only_the_last_id_and_0":
        sub = np.where((i // 3) % 2 == 0, n_subs - 1, 0)
    elif name == "long_runs_of_empty_subscriptions":
        sub = (i % 4) * 1000 + 17
    elif name == "nothing_taken":
        take[:] = False
    elif name == "one_in_16":
        sub, take = i % 300, i % 16 == 5
    elif name == "an_empty_tile_between_two_full_ones":
        sub, take = (i * 13) % 100, (i // TILE_MIN) % 3 != 1
    return sub, take


PATTERNS = ["one_subscription", "distinct_64_in_64", "two_alternating", "only_in_the_last_frame",
            "only_in_lane_0_of_each_wave", "only_the_last_id_and_0", "long_runs_of_empty_subscriptions", "nothing_taken",
            "one_in_16", "an_empty_tile_between_two_full_ones"]


@pytest.mark.parametrize("n", [300, 2100])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_key_patterns(pattern, n):
    """Two tiles with a ragged last wave (300 frames) and nine tiles (2,100): the place kernel walks 64 frames a step
    whatever the batch, so both sizes see every pattern at whole waves and at a partial one."""
    n_subs = 4096
    sub, take = _pattern(pattern, n, n_subs)
    rec = random_records(n, 70, 1, n)
    rec["sub_id"] = sub
    rec["flags"] = np.where(take, OK, un.MATCH | un.IP_OK)
    total = _run(n, n_subs, rec, stride=128, frame_off=6, seed=len(pattern))
    assert total["n_msgs"] == take.sum()
    if pattern == "nothing_taken":
        assert tuple(total) == (0, 0, 0)


def test_a_thousand_messages_of_one_subscription_stay_in_arrival_order():
    """Subscription 40 gets 1,000 messages whose payloads encode their arrival index, between traffic for others."""
    n, n_subs, stride, frame_off = 4000, 64, 128, 2
    rng = np.random.default_rng(1)
    rec = random_records(n, 70, n_subs, 1, take=1.0)
    rec["sub_id"] = np.where(rec["sub_id"] == 40, 41, rec["sub_id"])
    mine = np.sort(rng.choice(n, 1000, replace=False))
    rec["sub_id"][mine] = 40
    rec["payload_len"][mine] = 4
    ring = canary(n * stride, 3).reshape(n, stride)
    for k, i in enumerate(mine):
        ring[i, frame_off + 42:frame_off + 46] = np.frombuffer(np.uint32(k).tobytes(), np.uint8)
    ctx = pa.RxContext(0)
    d = Demux(ring, n, _need(rec, stride - frame_off, n_subs)[0], n_subs).records(rec).demux(ctx, stride, frame_off)
    d.check()
    pay, offs, lens, subs, src, first, sbytes, _ = d.outputs()
    lo, hi = int(first[GE + 40]), int(first[GE + 41])
    assert hi - lo == 1000 and np.array_equal(src[GE + lo:GE + hi], mine)
    b0 = int(sbytes[GE + 40])
    assert int(sbytes[GE + 41]) - b0 == 16000
    got = pay[G + b0:G + b0 + 16000].reshape(1000, 16)[:, :4].copy().view(np.uint32).reshape(-1)
    assert np.array_equal(got, np.arange(1000))
    ctx.close()


@pytest.mark.parametrize("frame_off", range(0, 16, 2))
def test_every_length_in_every_alignment_class(frame_off):
    """2-KiB slots of non-zero bytes: every length of LENS, the largest the slot holds, and one more (TRUNC: not
    taken), twice over, across the eight frame_off classes (both source shifts, every 16-byte residue)."""
    stride = 2048
    room = stride - frame_off - 42
    lens = list(LENS) + [room, room] + list(LENS[::-1]) + [room]
    over = {len(LENS) + 1}
    slots = _ring_of(lens, stride, frame_off, frame_off, over)
    n = len(lens)
    ctx = _ctx()
    cap = sum(ug.pad16(v) for v in lens)
    d = Demux(slots, n, cap, len(PAIRS)).classify(ctx, stride, frame_off).demux(ctx, stride, frame_off)
    rec = d.host_records()
    assert un.deliver(rec["flags"]).sum() == n - 1 and rec["flags"][len(LENS) + 1] & un.TRUNC
    total = d.check()
    assert total["n_msgs"] == n - 1 == total["n_fit"] and total["n_bytes"] == cap - ug.pad16(room)
    ctx.close()


@pytest.mark.parametrize("stride,frame_off,lens,over", [
    (16384, 8, (9000, 8999, 9001, 16384 - 8 - 42, 16384 - 8 - 42, 2200, 0, 9000), {4}),
    (16384, 2, (9000, 1, 9001, 0, 9000), ()),
    (112, 0, (70, 69, 0, 70, 54), {3}),          # the smallest slot there is
    (128, 14, (72, 71, 1, 72), {3}),
])
def test_jumbo_and_minimum_slots(stride, frame_off, lens, over):
    slots = _ring_of(lens, stride, frame_off, stride + frame_off, set(over))
    n = len(lens)
    ctx = _ctx()
    d = Demux(slots, n, sum(ug.pad16(v) for v in lens), len(PAIRS)).classify(ctx, stride, frame_off)
    total = d.demux(ctx, stride, frame_off).check()
    assert total["n_msgs"] == n - len(over)
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
    d = Demux(slots, n, n * 1488, len(PAIRS)).classify(ctx, stride, frame_off).demux(ctx, stride, frame_off)
    assert np.array_equal(d.host_records(), exp)
    total = d.check()
    assert 0 < total["n_msgs"] == un.deliver(exp["flags"]).sum() < n
    ctx.set_verify(False)
    d = Demux(slots, n, n * 1488, len(PAIRS)).classify(ctx, stride, frame_off).demux(ctx, stride, frame_off)
    assert np.array_equal(d.host_records(), rel)
    assert d.check()["n_msgs"] == un.deliver(rel["flags"]).sum() > total["n_msgs"]
    # fewer subscriptions than the table holds: the others' frames are skipped
    d = Demux(slots, n, n * 1488, 10).classify(ctx, stride, frame_off).demux(ctx, stride, frame_off)
    assert 0 < d.check()["n_msgs"] < total["n_msgs"]
    ctx.close()


def test_forged_records_read_and_write_nothing_outside():
    """sub_id == n_subs, sub_id 0xFFFFFFFF with DELIVER bits, payload_len past avail, payload_off 40, and 16 random
    bytes as a record: whatever is taken stays inside its frame and the outputs."""
    stride, frame_off, n, n_subs = 256, 8, 1200, 100
    avail = stride - frame_off
    rng = np.random.default_rng(6)
    rec = rng.integers(0, 256, n * 16, dtype=np.uint8).view(un.UDP_RESULT_DTYPE).copy()
    rec["flags"][::2] = OK
    rec["payload_off"][::3] = 42
    rec["payload_len"][::4] = rng.integers(0, avail - 42 + 3, len(rec[::4]))
    rec["sub_id"][::2] = rng.integers(0, n_subs + 20, len(rec[::2]))
    rec[0] = (1, 0, 0, 42, avail - 42, OK)       # ends exactly at avail: taken
    rec[1] = (2, 0, 0, 42, avail - 41, OK)       # one byte past it
    rec[2] = (n_subs, 0, 0, 42, 10, OK)
    rec[3] = (0xFFFFFFFF, 0, 0, 42, 10, OK)
    rec[4] = (5, 0, 0, 40, 10, OK)
    rec[5] = (n_subs - 1, 0, 0, 42, 10, OK)
    rec[6] = (1 << 12, 0, 0, 42, 10, OK)
    tk = np.array([ud.taken(r, avail, n_subs) for r in rec])
    assert list(tk[:7]) == [True, False, False, False, False, True, False] and 30 < tk.sum() < n // 2
    total = _run(n, n_subs, rec, stride=stride, frame_off=frame_off, seed=4)
    assert total["n_msgs"] == tk.sum()


@pytest.mark.parametrize("cap,fit,why", CAP_CASES)
def test_payload_capacity_by_hand(cap, fit, why):
    """The model test's seven frames: payload_cap 0, exact, one block short, the crossing inside a subscription (with
    empty messages after it) and exactly on a subscription's boundary."""
    ring, rec, stride = capacity_case()
    n = len(rec)
    ctx = pa.RxContext(0)
    d = Demux(ring, n, cap, 4).records(rec).demux(ctx, stride, 0)
    total = d.check()
    assert tuple(total) == (96, 7, fit), why
    ctx.close()


@pytest.mark.parametrize("short", ["zero", "one_block", "exact", "half", "boundary"])
def test_payload_capacity(short):
    """The same over 300 frames of 2-KiB slots: the messages past the capacity are indexed, not copied."""
    stride, frame_off, n, n_subs = 2048, 8, 300, 9
    avail = stride - frame_off
    rec = random_records(n, avail - 42, n_subs, 5)
    need, msgs = _need(rec, avail, n_subs)
    before_5 = _need(rec[rec["sub_id"] < 5], avail, n_subs)[0]  # where subscription 5's bytes start
    cap = {"zero": 0, "one_block": need - 16, "exact": need, "half": (need // 2) & ~15, "boundary": before_5}[short]
    total = _run(n, n_subs, rec, stride=stride, frame_off=frame_off, cap=cap, seed=8)
    assert (total["n_fit"] == msgs) == (short == "exact")


def test_everything_in_pinned_memory():
    stride, frame_off, n = 2048, 10, 140
    slots = mixed_ring(31, n, stride, frame_off, PAIRS)
    ctx = _ctx()
    d = Demux(slots, n, n * 1488, len(PAIRS), pinned=True).classify(ctx, stride, frame_off).demux(ctx, stride, frame_off)
    assert d.check()["n_msgs"] > 40
    ctx.close()


def test_src_index_may_be_null():
    n = 500
    rec = random_records(n, 400, 30, 9)
    _run(n, 30, rec, stride=512, frame_off=4, src_index=False)


def test_the_same_call_twice_gives_the_same_bytes():
    n, n_subs, stride, frame_off = 9000, 200, 128, 8
    rec = random_records(n, stride - frame_off - 42, n_subs, 12)
    ring = canary(n * stride, 5)
    need = _need(rec, stride - frame_off, n_subs)[0]
    ctx = pa.RxContext(0)
    a = Demux(ring, n, need, n_subs).records(rec).demux(ctx, stride, frame_off)
    b = Demux(ring, n, need, n_subs).records(rec).demux(ctx, stride, frame_off)
    a.check()
    for x, y in zip(a.outputs(), b.outputs()):
        assert np.array_equal(x, y)
    ctx.close()


def test_a_demux_and_a_gather_interleaved_on_two_streams():
    """One ctx: demux, gather, demux, gather on two streams, each scratch ordered by its own fence; all are right."""
    import torch

    stride, frame_off = 128, 8
    avail = stride - frame_off
    ctx = pa.RxContext(0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = []
    for k, n in enumerate((20000, 900, 20001, 3000)):
        rec = random_records(n, avail - 42, 50, 30 + k)
        ring = canary(n * stride, 20 + k)
        if k % 2 == 0:
            jobs.append(Demux(ring, n, _need(rec, avail, 50)[0], 50, seed=k).records(rec))
        else:
            jobs.append(Gather(ring, n, _need(rec, avail, 1 << 32)[0], seed=k).records(rec))
    torch.cuda.synchronize()
    for k, (j, s) in enumerate(zip(jobs, (s1, s2, s2, s1))):
        (j.demux if k % 2 == 0 else j.gather)(ctx, stride, frame_off, s)
    for j in jobs:
        j.check()
    ctx.sync()
    ctx.close()


def test_argsort_identity_against_the_gather_on_the_gpu():
    """pn_udp_gather's own output for the same ring and records, permuted by the stable argsort of its sub_ids."""
    stride, frame_off, n, n_subs = 256, 6, 6000, 48
    avail = stride - frame_off
    rec = random_records(n, avail - 42, 64, 21)  # ids 48..63 are dropped by the demux, kept by the gather
    ring = canary(n * stride, 6)
    ctx = pa.RxContext(0)
    g = Gather(ring, n, _need(rec, avail, 1 << 32)[0]).records(rec).gather(ctx, stride, frame_off)
    d = Demux(ring, n, _need(rec, avail, n_subs)[0], n_subs).records(rec).demux(ctx, stride, frame_off)
    go, do = g.outputs(), d.outputs()
    cut = lambda a, guard: a[guard:len(a) - guard]  # noqa: E731
    argsort_identity((cut(go[0], G), cut(go[1], GE), cut(go[2], GE), cut(go[3], GE), cut(go[4], GE), go[5][1:2]),
                     (cut(do[0], G), cut(do[1], GE), cut(do[2], GE), cut(do[3], GE), cut(do[4], GE), do[5][GE:],
                      do[6][GE:], do[7][1:2]), n_subs)
    ctx.close()


def test_build_classify_demux_build_gives_each_channel_back_in_order():
    """udp_build(CSUM) -> udp_classify -> udp_demux; udp_build again from the demuxed arrays (chan_ids = sub_ids)
    gives each channel's frames, contiguous and in the order they were sent."""
    import torch

    stride, frame_off, n, n_ch = 2048, 8, 700, 256
    tmpl, pairs = _dest_templates(n_ch)
    rng = np.random.default_rng(3)
    lens = rng.integers(0, stride - frame_off - 42 + 1, n).astype(np.uint16)
    lens[:len(LENS)] = LENS
    offs = np.cumsum(np.concatenate([[0], lens[:-1].astype(np.int64) + rng.integers(0, 5, n - 1)])).astype(np.uint64)
    src = rng.integers(1, 256, int(offs[-1]) + int(lens[-1]) + 32, dtype=np.uint8)
    ch = rng.integers(0, n_ch, n).astype(np.uint32)
    ctx = pa.RxContext(0)
    ctx.udp_set_channels(ub.make_channels(tmpl))
    ctx.udp_set_subs(un.make_subs(pairs))
    cur = torch.cuda.current_stream()
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()  # noqa: E731
    d_src = dev(np.concatenate([src, np.zeros(-len(src) % 16 + 16, np.uint8)]), np.uint8)
    d_offs, d_lens, d_ch = dev(offs, np.int64), dev(lens, np.int16), dev(ch, np.int32)
    ring0 = canary(n * stride, 12)
    d = Demux(ring0, n, sum(ug.pad16(v) for v in lens), n_ch)
    flens = torch.zeros(n, dtype=torch.int16, device="cuda")
    ctx.udp_build(d_src, len(src), d_offs, d_lens, d_ch, d.frames_ptr(), stride, frame_off, n, pa.PN_UB_CSUM, flens, cur)
    torch.cuda.synchronize()
    built = d.d_buf.cpu().numpy()[G:G + n * stride].copy()
    d.buf = built  # the frames the demux reads
    d.classify(ctx, stride, frame_off).demux(ctx, stride, frame_off)
    total = d.check()
    assert total["n_msgs"] == n == total["n_fit"]
    order = np.argsort(ch, kind="stable")
    out = d.outputs()
    assert np.array_equal(out[4][GE:GE + n], order) and np.array_equal(out[3][GE:GE + n], ch[order])
    ring2 = torch.from_numpy(ring0.copy()).cuda()
    flens2 = torch.zeros(n, dtype=torch.int16, device="cuda")
    ctx.udp_build(d.d_pay.data_ptr() + G, int(total["n_bytes"]), d.d_offs.data_ptr() + 8 * GE,
                  d.d_lens.data_ptr() + 2 * GE, d.d_subs.data_ptr() + 4 * GE, ring2, stride, frame_off, n,
                  pa.PN_UB_CSUM, flens2, cur)
    torch.cuda.synchronize()
    again, fl, fl2 = ring2.cpu().numpy().reshape(n, stride), flens.cpu().numpy(), flens2.cpu().numpy()
    assert np.array_equal(fl2, fl[order])
    for j in range(n):
        e = frame_off + int(fl2[j])
        assert np.array_equal(again[j, frame_off:e], built.reshape(n, stride)[order[j], frame_off:e]), j
    ctx.close()


def test_errors_name_themselves_and_launch_nothing():
    import torch

    stride, frame_off, n, n_subs = 2048, 8, 64, 8
    ring = canary(n * stride, 1)
    rec = random_records(n, 1000, n_subs, 1, take=1.0)
    d = Demux(ring, n, n * 1008, n_subs).records(rec)
    ctx = pa.RxContext(0)
    outs = d._douts()

    def fails(text, **k):
        a = dict(f=d.frames_ptr(), s=stride, o=frame_off, n=n, r=d.d_rec, ns=n_subs, p=outs[0], c=outs[1], po=outs[2],
                 pl=outs[3], su=outs[4], si=outs[5], sf=outs[6], sb=outs[7], t=outs[8])
        a.update(k)
        with pytest.raises(pa.PollnetError) as e:
            ctx.udp_demux(*a.values())
        assert "(-1)" in str(e.value) and "pn_udp_demux" in str(e.value) and text in str(e.value), str(e.value)

    for key in ("f", "r", "p", "po", "pl", "su"):
        fails("NULL", **{key: None})
    for key in ("t", "sf", "sb"):
        fails("NULL total, sub_first or sub_bytes", **{key: None})
        fails("NULL total, sub_first or sub_bytes", n=0, **{key: None})
    fails("8-byte", t=outs[8] + 4)
    fails("4-byte", sf=outs[6] + 2)
    fails("8-byte", sb=outs[7] + 4)
    fails("n_subs", ns=0)
    fails("n_subs", ns=4097)
    fails("n_subs", ns=0, n=0)
    fails("PN_UDP_DEMUX_MAX_N", n=(1 << 24) + 1)
    fails("aligned", f=d.frames_ptr() + 8)
    fails("aligned", r=d.d_rec.data_ptr() + 8)
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
    got = d.outputs()
    assert np.array_equal(got[0], d.pay0) and np.array_equal(got[1], d.offs0) and np.array_equal(got[5], d.first0) \
        and (got[7] == got[7][0]).all(), "a refused call launched"
    # n == 0: PN_OK, the total and both per-subscription arrays zeroed on the stream, nothing else written
    ctx.udp_demux(None, 0, 0, 0, None, n_subs, None, 0, None, None, None, None, outs[6], outs[7], outs[8],
                  torch.cuda.current_stream())
    got = d.outputs()
    assert tuple(got[7][1]) == (0, 0, 0) and got[7][0] == got[7][2] and got[7][0]["n_msgs"] == 0x22222222
    want_first, want_bytes = d.first0.copy(), d.bytes0.copy()
    want_first[GE:GE + n_subs + 1] = 0
    want_bytes[GE:GE + n_subs + 1] = 0
    assert np.array_equal(got[5], want_first) and np.array_equal(got[6], want_bytes)
    assert np.array_equal(got[0], d.pay0) and np.array_equal(got[2], d.lens0)
    d.demux(ctx, stride, frame_off)  # and the ctx still works
    assert d.check()["n_msgs"] == n
    ctx.close()
