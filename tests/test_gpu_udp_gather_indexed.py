"""pn_udp_gather_indexed through the Python binding, every output whole against tests/udp_gather_np.py: pollnet's
ef_vi UDP ring driven by RX-event runs that wrap, repeat and skip, packed captures in all eight alignment classes,
the smallest avail with a datagram that ends exactly at it, offsets outside the class, and the identity layout
against pn_udp_gather on the same GPU.  The records are the ones pn_udp_classify_indexed wrote for the same
offsets (tests/test_gpu_udp_indexed.py holds those to their own model)."""
import numpy as np
import pytest

import pollnet_amd as pa

import udp_gather_np as ug
import udp_np as un
from test_gpu_udp import mixed_ring
from test_gpu_udp_indexed import PAIRS, _event_ids, _frame, _mixed_frames, _pack
from udp_gather_dev import Gather, canary

pytestmark = pytest.mark.gpu

OK = un.MATCH | un.IP_OK | un.UDP_OK


def _ctx():
    ctx = pa.RxContext(0)
    ctx.udp_set_subs(un.make_subs(PAIRS))
    return ctx


@pytest.mark.parametrize("prefix", [0, 2, 14])
def test_event_ring_runs_that_wrap_repeat_and_skip(prefix):
    """EfviUdpRingLayout: 511 buffers of 2,048 B, the frame at 64 + prefix; 1,300 events over it, then the release
    path on the same run."""
    frame_off, stride, bufs, n = 64 + prefix, 2048, 511, 1300
    avail = stride - frame_off
    ring = mixed_ring(600 + prefix, bufs, stride, frame_off, PAIRS)
    ids = _event_ids(np.random.default_rng(prefix), n)
    assert len(np.unique(ids)) < bufs and (np.diff(ids.astype(np.int64)) < 0).sum() >= 2 and (np.diff(ids) == 0).any()
    offsets = ids * np.uint64(stride) + np.uint64(frame_off)
    ctx = _ctx()
    g = Gather(ring, n, n * 1488).classify_indexed(ctx, offsets, frame_off % 16, avail)
    g.gather_indexed(ctx, offsets, frame_off % 16, avail)
    total = g.check()
    assert 300 < total["n_msgs"] < n and total["n_fit"] == total["n_msgs"]
    ctx.set_verify(False)
    g = Gather(ring, n, n * 1488).classify_indexed(ctx, offsets, frame_off % 16, avail)
    g.gather_indexed(ctx, offsets, frame_off % 16, avail)
    assert g.check()["n_msgs"] > total["n_msgs"]
    ctx.close()


@pytest.mark.parametrize("eth_mod16", range(0, 16, 2))
def test_packed_capture(eth_mod16):
    """Frames back to back at 16-byte steps (the next frame's bytes follow every datagram), 9,000-byte datagrams
    among them; and the same capture with a capacity that ends mid-way."""
    n, avail = 200, 9216
    rng = np.random.default_rng(950 + eth_mod16)
    buf, offsets = _pack(rng, _mixed_frames(rng, n, avail, jumbo_every=2), eth_mod16, avail)
    ctx = _ctx()
    g = Gather(buf, n, 1 << 19).classify_indexed(ctx, offsets, eth_mod16, avail)
    g.gather_indexed(ctx, offsets, eth_mod16, avail)
    rec = g.host_records()
    assert (rec["payload_len"][un.deliver(rec["flags"])] > 8000).any(), "no delivered jumbo datagram"
    total = g.check()
    assert 40 < total["n_msgs"] < n
    half = (int(total["n_bytes"]) // 2) & ~15
    g = Gather(buf, n, half).classify_indexed(ctx, offsets, eth_mod16, avail)
    g.gather_indexed(ctx, offsets, eth_mod16, avail)
    assert 0 < g.check()["n_fit"] < total["n_msgs"]
    ctx.close()


@pytest.mark.parametrize("eth_mod16", [0, 2, 8, 14])
def test_avail_of_96_with_a_datagram_ending_exactly_at_it(eth_mod16):
    """avail 96: payloads of 54 bytes end at avail's last byte; 53 and 52 end below it; one declares a byte more
    (TRUNC).  The capture's next frame (non-zero bytes) starts right behind."""
    avail, room = 96, 54
    rng = np.random.default_rng(eth_mod16)
    frames = []
    for i in range(40):
        p = (room, room - 1, room - 2, room + 1, 0, 1, 17, 33, room - 3, room)[i % 10]
        if p > room:
            frames.append(_frame(rng, room, ulen=avail - 33, tot_len=20 + avail - 33))
        else:
            frames.append(_frame(rng, p, **({"udp_csum": 0} if i % 7 == 5 else {})))
    buf, offsets = _pack(rng, frames, eth_mod16, avail)
    ctx = _ctx()
    g = Gather(buf, len(frames), 40 * 64).classify_indexed(ctx, offsets, eth_mod16, avail)
    g.gather_indexed(ctx, offsets, eth_mod16, avail)
    rec = g.host_records()
    d = un.deliver(rec["flags"])
    assert (rec["payload_len"][d] == room).sum() >= 8 and ((rec["flags"] & un.TRUNC) != 0).sum() == 4 and d.sum() == 36
    assert g.check()["n_msgs"] == 36
    ctx.close()


def test_a_tenth_of_the_offsets_outside_the_class():
    """Another class, or far outside the buffer: BADOFF records, never taken, none of their bytes read.  And records
    that claim delivery for them (forged) take nothing either."""
    frame_off, stride, bufs, n = 66, 2048, 511, 1000
    ring = mixed_ring(66, bufs, stride, frame_off, PAIRS)
    rng = np.random.default_rng(10)
    offsets = _event_ids(rng, n) * np.uint64(stride) + np.uint64(frame_off)
    bad = np.zeros(n, bool)
    bad[rng.choice(n, n // 10, replace=False)] = True
    bad[[0, 63, 64, n - 1]] = True
    stray = offsets.copy()
    for j, i in enumerate(np.flatnonzero(bad)):
        stray[i] = offsets[i] + np.uint64(2 * (1 + j % 7)) if j % 3 else np.uint64((1 << 44) + 16 * j + 2 * (2 + j % 7))
    ctx = _ctx()
    g = Gather(ring, n, n * 1488).classify_indexed(ctx, stray, 2, stride - frame_off)
    g.gather_indexed(ctx, stray, 2, stride - frame_off)
    rec = g.host_records()
    assert (rec["flags"][bad] == 0x4000).all() and not (rec["flags"][~bad] & 0x4000).any()
    total = g.check()
    src = g.outputs()[4][16:16 + int(total["n_msgs"])]
    assert not bad[src].any() and total["n_msgs"] == un.deliver(rec["flags"]).sum() > 200
    forged = rec.copy()
    forged["flags"][bad] = OK
    forged["payload_off"][bad] = 42
    forged["payload_len"][bad] = 100
    g2 = Gather(ring, n, n * 1488).records(forged)
    g2.gather_indexed(ctx, stray, 2, stride - frame_off)
    assert g2.check()["n_msgs"] == total["n_msgs"]
    ctx.close()


@pytest.mark.parametrize("frame_off,stride,n", [(2, 2048, 300), (0, 112, 130), (14, 128, 257), (6, 4096, 130),
                                                (8, 128, 20000)])
def test_identity_layout_equals_the_strided_call(frame_off, stride, n):
    """offsets[i] = i * stride + frame_off: byte for byte what pn_udp_gather writes for the same ring and records."""
    if n < 1000:
        slots = mixed_ring(40 + frame_off, n, stride, frame_off, PAIRS)
    else:
        slots = canary(n * stride, 5)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(frame_off)
    ctx = _ctx()
    cap = n * ug.pad16(stride - frame_off - 42)
    a = Gather(slots, n, cap)
    b = Gather(slots, n, cap)
    if n < 1000:
        a.classify(ctx, stride, frame_off)
        b.records(a.host_records())
    else:
        rng = np.random.default_rng(n)
        rec = np.zeros(n, un.UDP_RESULT_DTYPE)
        rec["payload_off"], rec["payload_len"] = 42, rng.integers(0, stride - frame_off - 42 + 1, n)
        rec["flags"] = np.where(rng.integers(0, 3, n) != 0, OK, un.MATCH)
        rec["sub_id"] = rng.integers(0, 64, n)
        a.records(rec)
        b.records(rec)
    a.gather(ctx, stride, frame_off)
    b.gather_indexed(ctx, offsets, frame_off % 16, stride - frame_off)
    total = a.check()
    assert b.check() == total and total["n_msgs"] > n // 4
    for x, y in zip(a.outputs(), b.outputs()):
        assert np.array_equal(x, y)
    ctx.close()


def test_everything_in_pinned_memory():
    frame_off, stride, bufs, n = 64, 2048, 511, 600
    ring = mixed_ring(64, bufs, stride, frame_off, PAIRS)
    offsets = _event_ids(np.random.default_rng(3), n) * np.uint64(stride) + np.uint64(frame_off)
    ctx = _ctx()
    g = Gather(ring, n, n * 1488, pinned=True).classify_indexed(ctx, offsets, 0, stride - frame_off)
    g.gather_indexed(ctx, offsets, 0, stride - frame_off)
    assert g.check()["n_msgs"] > 150
    ctx.close()


def test_errors_name_the_function_and_launch_nothing():
    import torch

    n, avail = 64, 2048
    ring = canary(n * 2048 + 4096, 1)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(2048) + np.uint64(2)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    rec["payload_off"], rec["payload_len"], rec["flags"] = 42, 200, OK
    g = Gather(ring, n, n * 208).records(rec)
    g.d_idx = g.put(offsets.view(np.int64).copy())
    ctx = pa.RxContext(0)
    outs = g._outs()

    def fails(text, **k):
        a = dict(b=g.frames_ptr(), o=g.d_idx, m=2, n=n, a=avail, r=g.d_rec, p=outs[0], c=outs[1], po=outs[2], pl=outs[3],
                 su=outs[4], si=outs[5], t=outs[6])
        a.update(k)
        with pytest.raises(pa.PollnetError) as e:
            ctx.udp_gather_indexed(*a.values())
        assert "(-1)" in str(e.value) and "pn_udp_gather_indexed" in str(e.value) and text in str(e.value), str(e.value)
        assert text in pa.rx._pn_last_error(ctx._h).decode()

    for key in ("b", "o", "r", "p", "po", "pl", "su"):
        fails("NULL", **{key: None})
    fails("NULL total", t=None)
    fails("8-byte", t=outs[6] + 4)
    fails("16-byte", b=g.frames_ptr() + 8)
    fails("8-byte aligned", o=g.d_idx.data_ptr() + 4)
    fails("aligned", r=g.d_rec.data_ptr() + 8)
    fails("aligned", p=outs[0] + 8)
    fails("aligned", c=outs[1] + 8)
    fails("aligned", si=outs[5] + 2)
    fails("eth_mod16 must be even < 16", m=3)
    fails("eth_mod16 must be even < 16", m=16)
    fails("avail in [96, 65536]", a=95)
    fails("avail in [96, 65536]", a=65537)
    torch.cuda.synchronize()
    got = g.outputs()
    assert np.array_equal(got[0], g.pay0) and np.array_equal(got[3], g.subs0) and (got[5] == got[5][0]).all(), \
        "a refused call launched"
    ctx.udp_gather_indexed(None, None, 2, 0, avail, None, None, 0, None, None, None, None, outs[6],
                           torch.cuda.current_stream())  # n == 0: the total zeroed, nothing else
    got = g.outputs()
    assert tuple(got[5][1]) == (0, 0, 0) and got[5][0] == got[5][2] and np.array_equal(got[0], g.pay0)
    g.gather_indexed(ctx, offsets, 2, avail)
    assert g.check()["n_msgs"] == n
    ctx.close()
