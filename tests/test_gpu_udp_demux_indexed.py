"""pn_udp_demux_indexed through the Python binding, every output whole against tests/udp_demux_np.py: pollnet's
ef_vi UDP ring driven by RX-event runs that wrap, repeat and skip, packed captures in all eight alignment classes,
offsets outside the class (with forged DELIVER records for them), and the identity layout byte for byte against
pn_udp_demux.  The records are the ones pn_udp_classify_indexed wrote for the same offsets."""
import numpy as np
import pytest

import pollnet_amd as pa

import udp_gather_np as ug
import udp_np as un
from test_gpu_udp import mixed_ring
from test_gpu_udp_indexed import PAIRS, _event_ids, _mixed_frames, _pack
from test_udp_demux_np import random_records
from udp_demux_dev import GE, Demux, canary

pytestmark = pytest.mark.gpu

OK = un.MATCH | un.IP_OK | un.UDP_OK
N_SUBS = len(PAIRS)


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
    d = Demux(ring, n, n * 1488, N_SUBS).classify_indexed(ctx, offsets, frame_off % 16, avail)
    total = d.demux_indexed(ctx, offsets, frame_off % 16, avail).check()
    assert 300 < total["n_msgs"] < n and total["n_fit"] == total["n_msgs"]
    first = d.outputs()[5][GE:GE + N_SUBS + 1]
    assert (np.diff(first.astype(np.int64)) > 0).sum() > 8, "several subscriptions received"
    ctx.set_verify(False)
    d = Demux(ring, n, n * 1488, N_SUBS).classify_indexed(ctx, offsets, frame_off % 16, avail)
    assert d.demux_indexed(ctx, offsets, frame_off % 16, avail).check()["n_msgs"] > total["n_msgs"]
    ctx.close()


@pytest.mark.parametrize("eth_mod16", range(0, 16, 2))
def test_packed_capture(eth_mod16):
    """Frames back to back at 16-byte steps (the next frame's bytes follow every datagram), 9,000-byte datagrams
    among them; and the same capture with a capacity that ends mid-way."""
    n, avail = 200, 9216
    rng = np.random.default_rng(950 + eth_mod16)
    buf, offsets = _pack(rng, _mixed_frames(rng, n, avail, jumbo_every=2), eth_mod16, avail)
    ctx = _ctx()
    d = Demux(buf, n, 1 << 19, N_SUBS).classify_indexed(ctx, offsets, eth_mod16, avail)
    d.demux_indexed(ctx, offsets, eth_mod16, avail)
    rec = d.host_records()
    assert (rec["payload_len"][un.deliver(rec["flags"])] > 8000).any(), "no delivered jumbo datagram"
    total = d.check()
    assert 40 < total["n_msgs"] < n
    half = (int(total["n_bytes"]) // 2) & ~15
    d = Demux(buf, n, half, N_SUBS).classify_indexed(ctx, offsets, eth_mod16, avail)
    assert 0 < d.demux_indexed(ctx, offsets, eth_mod16, avail).check()["n_fit"] < total["n_msgs"]
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
    d = Demux(ring, n, n * 1488, N_SUBS).classify_indexed(ctx, stray, 2, stride - frame_off)
    d.demux_indexed(ctx, stray, 2, stride - frame_off)
    rec = d.host_records()
    assert (rec["flags"][bad] == 0x4000).all() and not (rec["flags"][~bad] & 0x4000).any()
    total = d.check()
    src = d.outputs()[4][GE:GE + int(total["n_msgs"])]
    assert not bad[src].any() and total["n_msgs"] == un.deliver(rec["flags"]).sum() > 200
    forged = rec.copy()
    forged["flags"][bad] = OK
    forged["payload_off"][bad] = 42
    forged["payload_len"][bad] = 100
    forged["sub_id"][bad] = 3
    d2 = Demux(ring, n, n * 1488, N_SUBS).records(forged)
    assert d2.demux_indexed(ctx, stray, 2, stride - frame_off).check()["n_msgs"] == total["n_msgs"]
    ctx.close()


@pytest.mark.parametrize("frame_off,stride,n", [(2, 2048, 300), (0, 112, 130), (14, 128, 257), (6, 4096, 130),
                                                (8, 128, 20000)])
def test_identity_layout_equals_the_strided_call(frame_off, stride, n):
    """offsets[i] = i * stride + frame_off: byte for byte what pn_udp_demux writes for the same ring and records."""
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(frame_off)
    ctx = _ctx()
    cap = n * ug.pad16(stride - frame_off - 42)
    if n < 1000:
        slots = mixed_ring(40 + frame_off, n, stride, frame_off, PAIRS)
        a = Demux(slots, n, cap, N_SUBS).classify(ctx, stride, frame_off)
        rec = a.host_records()
    else:
        slots = canary(n * stride, 5)
        rec = random_records(n, stride - frame_off - 42, N_SUBS + 3, n)
        a = Demux(slots, n, cap, N_SUBS)
    a.records(rec)
    b = Demux(slots, n, cap, N_SUBS).records(rec)
    a.demux(ctx, stride, frame_off)
    b.demux_indexed(ctx, offsets, frame_off % 16, stride - frame_off)
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
    d = Demux(ring, n, n * 1488, N_SUBS, pinned=True).classify_indexed(ctx, offsets, 0, stride - frame_off)
    assert d.demux_indexed(ctx, offsets, 0, stride - frame_off).check()["n_msgs"] > 150
    ctx.close()


def test_errors_name_the_function_and_launch_nothing():
    import torch

    n, avail, n_subs = 64, 2048, 4
    ring = canary(n * 2048 + 4096, 1)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(2048) + np.uint64(2)
    rec = np.zeros(n, un.UDP_RESULT_DTYPE)
    rec["payload_off"], rec["payload_len"], rec["flags"], rec["sub_id"] = 42, 200, OK, np.arange(n) % n_subs
    d = Demux(ring, n, n * 208, n_subs).records(rec)
    d.d_idx = d.put(offsets.view(np.int64).copy())
    ctx = pa.RxContext(0)
    outs = d._douts()

    def fails(text, **k):
        a = dict(b=d.frames_ptr(), o=d.d_idx, m=2, n=n, a=avail, r=d.d_rec, ns=n_subs, p=outs[0], c=outs[1], po=outs[2],
                 pl=outs[3], su=outs[4], si=outs[5], sf=outs[6], sb=outs[7], t=outs[8])
        a.update(k)
        with pytest.raises(pa.PollnetError) as e:
            ctx.udp_demux_indexed(*a.values())
        assert "(-1)" in str(e.value) and "pn_udp_demux_indexed" in str(e.value) and text in str(e.value), str(e.value)
        assert text in pa.rx._pn_last_error(ctx._h).decode()

    for key in ("b", "o", "r", "p", "po", "pl", "su"):
        fails("NULL", **{key: None})
    for key in ("t", "sf", "sb"):
        fails("NULL total, sub_first or sub_bytes", **{key: None})
    fails("8-byte", t=outs[8] + 4)
    fails("4-byte", sf=outs[6] + 2)
    fails("n_subs", ns=0)
    fails("n_subs", ns=4097)
    fails("PN_UDP_DEMUX_MAX_N", n=(1 << 24) + 1)
    fails("16-byte", b=d.frames_ptr() + 8)
    fails("8-byte aligned", o=d.d_idx.data_ptr() + 4)
    fails("aligned", r=d.d_rec.data_ptr() + 8)
    fails("aligned", p=outs[0] + 8)
    fails("aligned", c=outs[1] + 8)
    fails("aligned", si=outs[5] + 2)
    fails("eth_mod16 must be even < 16", m=3)
    fails("eth_mod16 must be even < 16", m=16)
    fails("avail in [96, 65536]", a=95)
    fails("avail in [96, 65536]", a=65537)
    torch.cuda.synchronize()
    got = d.outputs()
    assert np.array_equal(got[0], d.pay0) and np.array_equal(got[3], d.subs0) and np.array_equal(got[6], d.bytes0) \
        and (got[7] == got[7][0]).all(), "a refused call launched"
    ctx.udp_demux_indexed(None, None, 2, 0, avail, None, n_subs, None, 0, None, None, None, None, outs[6], outs[7],
                          outs[8], torch.cuda.current_stream())  # n == 0: the total and the two arrays zeroed
    got = d.outputs()
    assert tuple(got[7][1]) == (0, 0, 0) and got[7][0] == got[7][2] and np.array_equal(got[0], d.pay0)
    assert not got[5][GE:GE + n_subs + 1].any() and not got[6][GE:GE + n_subs + 1].any()
    assert got[5][GE + n_subs + 1] == d.first0[GE + n_subs + 1] and got[6][GE - 1] == d.bytes0[GE - 1]
    d.demux_indexed(ctx, offsets, 2, avail)
    assert d.check()["n_msgs"] == n
    ctx.close()
