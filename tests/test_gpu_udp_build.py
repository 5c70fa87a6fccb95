"""pn_udp_build / pn_udp_set_channels through the Python binding: the whole ring -- guard bytes before slot 0 and
after slot n-1 included -- and frame_lens byte for byte against tests/udp_build_np.py (pinned by
tests/test_udp_build_np.py).  The ring starts as a non-constant canary, so any stray write fails."""
import numpy as np
import pytest

import pollnet_amd as pa

import udp_build_np as ub
import udp_np as un
from test_udp_build_np import _dest_templates, _templates

pytestmark = pytest.mark.gpu

G = 256  # guard bytes before slot 0 and after slot n-1
LENS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 1023, 1024, 1025, 1472)
MODES = (ub.UB_EFVI, ub.UB_PLAIN, ub.UB_CSUM)


def _canary(nbytes, seed=0xCA):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def _pack(lens, residues=None, seed=3, tail=0):
    """Payloads packed one after another (message i's offset moved up to residue residues[i] mod 16 when given).
    Returns (buffer, payload_bytes, offs)."""
    offs, at = [], 0
    for i, ln in enumerate(lens):
        if residues is not None:
            at += (int(residues[i]) - at) % 16
        offs.append(at)
        at += int(ln)
    payload_bytes = at + tail
    buf = np.random.default_rng(seed).integers(0, 256, max(payload_bytes, 1), dtype=np.uint8)
    return buf, payload_bytes, np.array(offs, np.uint64)


class Dev:
    """The device (or pinned) buffers of one build and their comparison with the model."""

    def __init__(self, n, stride, pay, payload_bytes, offs, lens, chan_ids, pinned=False, ring=None):
        import torch

        self.torch, self.n, self.stride = torch, n, stride
        self.ring0 = _canary(2 * G + n * stride) if ring is None else ring
        self.pay, self.payload_bytes = pay, payload_bytes
        self.offs, self.lens, self.chan_ids = offs, np.asarray(lens, np.uint16), chan_ids
        put = (lambda a: torch.from_numpy(a).pin_memory()) if pinned else (lambda a: torch.from_numpy(a).cuda())
        padded = np.zeros((len(pay) + 15) // 16 * 16 + 16, np.uint8)
        padded[:len(pay)] = pay
        self.d_pay = put(padded)
        self.d_ring = put(self.ring0.copy())
        self.d_offs = put(np.asarray(offs, np.uint64).view(np.int64))
        self.d_lens = put(self.lens.view(np.int16))
        self.d_chans = None if chan_ids is None else put(np.asarray(chan_ids, np.uint32).view(np.int32))
        self.flens0 = ((np.arange(7, 7 + n + 16) * 257) % 65521 | 1).astype(np.uint16)  # canary around and under frame_lens
        self.d_flens = put(self.flens0.copy().view(np.int16))

    def build(self, ctx, frame_off, mode, stream=None, n=None):
        ctx.udp_build(self.d_pay, self.payload_bytes, self.d_offs, self.d_lens, self.d_chans,
                      self.d_ring.data_ptr() + G, self.stride, frame_off, self.n if n is None else n, mode,
                      self.d_flens.data_ptr() + 16, stream if stream is not None else self.torch.cuda.current_stream())

    def ring(self):
        self.torch.cuda.synchronize()
        return self.d_ring.cpu().numpy()

    def check(self, chans, frame_off, mode, ring0=None):
        """The ring and frame_lens now vs the model applied to ring0 (default: the canary).  Returns frame_lens."""
        exp, flens = ub.udp_build_np(self.ring0 if ring0 is None else ring0, self.stride, frame_off, chans, self.pay,
                                     self.payload_bytes, self.offs, self.lens, self.chan_ids, mode, first_slot_at=G)
        got = self.ring()
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, "ring differs at byte %d (slot %d + %d): got %02x want %02x; %d bytes differ" % (
            bad[0], (bad[0] - G) // self.stride, (bad[0] - G) % self.stride, got[bad[0]], exp[bad[0]], bad.size)
        gl = self.d_flens.cpu().numpy().view(np.uint16)
        el = self.flens0.copy()
        el[8:8 + self.n] = flens
        badl = np.flatnonzero(gl != el)
        assert badl.size == 0, "frame_lens differs at %d: got %d want %d" % (badl[0] - 8, gl[badl[0]], el[badl[0]])
        return flens


def _ctx(chans):
    ctx = pa.RxContext(0)
    ctx.udp_set_channels(chans)
    return ctx


def _chans64():
    tmpl, _ = _templates(64, 64)
    return ub.make_channels(tmpl)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("frame_off", range(0, 16, 2))
def test_every_length_source_residue_and_destination_class(frame_off, mode):
    """Stride 2048: every length of LENS, the largest that fits and that + 1 (refused), each at every source
    residue pay_offs % 16, in each of the 8 destination classes and the 3 modes."""
    stride = 2048
    room = stride - frame_off - 42
    lens, res = [], []
    for r in range(16):
        for ln in LENS + (room, room + 1):
            lens.append(ln)
            res.append((r + len(lens)) % 16 if ln in (room, room + 1) else r)
    for ln in LENS:  # and once more at residues rotated against the lengths
        lens.append(ln)
        res.append((ln * 7 + 5) % 16)
    n = len(lens)
    assert {(ln, r) for ln, r in zip(lens, res)} >= {(ln, r) for ln in LENS for r in range(16)}
    pay, pb, offs = _pack(lens, res, seed=frame_off)
    chans = _chans64()
    chan_ids = (np.arange(n, dtype=np.uint32) * 5) % 64
    ctx = _ctx(chans)
    d = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    d.build(ctx, frame_off, mode)
    fl = d.check(chans, frame_off, mode)
    assert (fl == 0).sum() == 16
    ctx.close()


@pytest.mark.parametrize("stride,frame_off,lens", [
    (2048, 8, None),                                   # Efvi's TX ring exactly: 128 pkt_bufs
    (112, 0, None), (128, 8, None), (128, 14, None),   # 112 + frame_off rounded up to 16
    (96, 0, None), (112, 2, None),                     # the contract's minimum, frame_off + 96
    (16384, 8, (9000, 8999, 9001, 16384 - 8 - 42, 16384 - 8 - 41, 2007, 0)),
    (65536, 0, (65493, 65494, 65507, 65508, 1)),       # 42 + 65,494 does not fit frame_lens; 65,507 not the slot
    (65536, 8, (65486, 65487)),
])
def test_layouts(stride, frame_off, lens):
    room = stride - frame_off - 42
    if lens is None:
        n = 128
        rng = np.random.default_rng(stride + frame_off)
        lens = rng.integers(0, room + 2, n)
        lens[:4] = (room, room + 1, 0, room - 1)
    n = len(lens)
    pay, pb, offs = _pack(lens, seed=stride)
    chans = _chans64()
    chan_ids = np.random.default_rng(5).integers(0, 64, n).astype(np.uint32)
    ctx = _ctx(chans)
    d = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    d.build(ctx, frame_off, ub.UB_CSUM)
    fl = d.check(chans, frame_off, ub.UB_CSUM)
    assert (fl != 0).any() and (fl == 0).any()
    ctx.close()


@pytest.mark.parametrize("n,mode", [(1, 2), (5, 2), (63, 2), (64, 2), (65, 2), (1000, 2), (8195, 2), (16389, 1),
                                    (32771, 2), (65573, 0)])
def test_batch_sizes_and_frames_per_wave_tiers(n, mode):
    """Batches that end inside a wave, in each frames-per-wave tier (8 messages a wave up to 16,368 messages, 16
    up to 32,736, 32 up to 65,472, 64 above), short payloads in 256-B slots."""
    stride, frame_off = 256, 8
    room = stride - frame_off - 42
    rng = np.random.default_rng(n)
    lens = rng.integers(0, room + 1, n)
    if n >= 64:
        lens[rng.integers(0, n, n // 50 + 1)] = room + 1 + rng.integers(0, 9)  # a few refused
    pay, pb, offs = _pack(lens, seed=n)
    chans = _chans64()
    chan_ids = rng.integers(0, 64, n).astype(np.uint32)
    ctx = _ctx(chans)
    d = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    d.build(ctx, frame_off, mode)
    d.check(chans, frame_off, mode)
    ctx.close()


@pytest.mark.parametrize("n_ch", [1, 64, 4096])
def test_channel_sets(n_ch):
    """Sets of 1, 64 and 4,096 channels; one id equal to the count (refused); and chan_ids = NULL."""
    stride, frame_off, n = 256, 8, 700
    tmpl, _ = _templates(n_ch, n_ch)
    chans = ub.make_channels(tmpl)
    rng = np.random.default_rng(n_ch)
    lens = rng.integers(0, 180, n)
    pay, pb, offs = _pack(lens, seed=n_ch)
    chan_ids = rng.integers(0, n_ch, n).astype(np.uint32)
    chan_ids[:3] = (n_ch - 1, n_ch, 0)
    chan_ids[77] = 0xFFFFFFFF
    ctx = _ctx(chans)
    d = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    d.build(ctx, frame_off, ub.UB_CSUM)
    fl = d.check(chans, frame_off, ub.UB_CSUM)
    assert fl[1] == 0 and fl[77] == 0 and fl[0] != 0
    d0 = Dev(n, stride, pay, pb, offs, lens, None)
    d0.build(ctx, frame_off, ub.UB_EFVI)
    assert (d0.check(chans, frame_off, ub.UB_EFVI) != 0).all()
    ctx.close()


def test_one_payload_fanned_out_to_64_channels_and_overlapping_ranges():
    stride, frame_off = 2048, 8
    chans = _chans64()
    pay = _canary(4096, 9)
    lens = [1400] * 64 + [300] * 64
    offs = np.array([13] * 64 + [5 + 3 * i for i in range(64)], np.uint64)  # equal, then overlapping
    chan_ids = np.concatenate([np.arange(64), np.arange(64)[::-1]]).astype(np.uint32)
    ctx = _ctx(chans)
    d = Dev(128, stride, pay, len(pay), offs, lens, chan_ids)
    d.build(ctx, frame_off, ub.UB_CSUM)
    assert (d.check(chans, frame_off, ub.UB_CSUM) != 0).all()
    ctx.close()


@pytest.mark.parametrize("payload_bytes", [4096, 4099, 4081])
def test_payload_bounds(payload_bytes):
    """A message ending exactly at payload_bytes, one byte past it (refused), pay_offs == payload_bytes with len 0
    (accepted) and len 1 (refused): refused offsets stay within a few bytes of the buffer."""
    stride, frame_off = 2048, 8
    pb = payload_bytes
    pay = _canary(pb, pb)
    cases = [(pb - 100, 100), (pb - 100, 101), (pb, 0), (pb, 1), (pb + 1, 0), (pb - 1, 1), (pb - 1, 2), (0, 1472),
             (pb - 1472, 1472), (pb - 1471, 1472), (pb - 3, 3), (pb - 3, 4), (pb + 3, 0), (pb - 17, 17), (pb - 17, 18)]
    want_refused = [False, True, False, True, True, False, True, False, False, True, False, True, True, False, True]
    offs = np.array([c[0] for c in cases], np.uint64)
    lens = [c[1] for c in cases]
    chans = _chans64()
    ctx = _ctx(chans)
    d = Dev(len(cases), stride, pay, pb, offs, lens, np.arange(len(cases), dtype=np.uint32))
    d.build(ctx, frame_off, ub.UB_CSUM)
    fl = d.check(chans, frame_off, ub.UB_CSUM)
    assert list(fl == 0) == want_refused
    ctx.close()


def _mixed_refusals(n, room, n_ch, pb_extra=0, seed=11):
    """n messages, a tenth refused for mixed reasons scattered through the batch."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, room + 1, n)
    pay, pb, offs = _pack(lens, seed=seed)
    chan_ids = rng.integers(0, n_ch, n).astype(np.uint32)
    bad = rng.permutation(n)[:n // 10]
    for k, i in enumerate(bad):
        why = k % 4
        if why == 0:
            lens[i] = room + 1 + k % 5  # too long for the slot
        elif why == 1:
            chan_ids[i] = n_ch + k % 3  # no such channel
        elif why == 2:
            offs[i] = pb + 1 + k % 3  # starts past the buffer
        else:
            offs[i], lens[i] = pb - 5, 6 + k % 3  # ends past the buffer
    return pay, pb, offs, lens, chan_ids, bad


@pytest.mark.parametrize("mode", MODES)
def test_a_tenth_refused_for_mixed_reasons(mode):
    stride, frame_off, n = 2048, 8, 640
    chans = _chans64()
    pay, pb, offs, lens, chan_ids, bad = _mixed_refusals(n, stride - frame_off - 42, 64)
    ctx = _ctx(chans)
    d = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    d.build(ctx, frame_off, mode)
    fl = d.check(chans, frame_off, mode)
    assert set(np.flatnonzero(fl == 0)) == set(bad)
    ctx.close()


@pytest.mark.parametrize("mode", [ub.UB_PLAIN, ub.UB_CSUM])
def test_built_ring_through_pn_udp_classify(mode):
    """Sender -> receiver on the GPU: the channels' destinations as subscriptions; every accepted frame comes back
    MATCH | IP_OK with sub_id = its channel, its length, and NOCSUM (PLAIN) or UDP_OK (CSUM)."""
    import torch

    stride, frame_off, n, n_ch = 2048, 8, 640, 256
    tmpl, pairs = _dest_templates(n_ch)
    chans = ub.make_channels(tmpl)
    pay, pb, offs, lens, chan_ids, bad = _mixed_refusals(n, stride - frame_off - 42, n_ch, seed=12 + mode)
    ctx = _ctx(chans)
    ctx.udp_set_subs(un.make_subs(pairs))
    d = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    d.build(ctx, frame_off, mode)
    out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    ctx.udp_classify(d.d_ring.data_ptr() + G, stride, frame_off, n, out, torch.cuda.current_stream())
    fl = d.check(chans, frame_off, mode)
    rec = out.cpu().numpy().view(pa.UDP_RESULT_DTYPE)
    acc = fl != 0
    want = pa.UF.MATCH | pa.UF.IP_OK | (pa.UF.NOCSUM if mode == ub.UB_PLAIN else pa.UF.UDP_OK)
    assert acc.sum() == n - len(bad)
    assert (rec["flags"][acc] == want).all(), np.unique(rec["flags"][acc])
    assert (rec["sub_id"][acc] == chan_ids[acc]).all()
    assert (rec["payload_len"][acc] == np.asarray(lens, np.uint16)[acc]).all()
    ctx.close()


def test_consistent_with_pn_tx_fill():
    """Build in PLAIN mode, scramble the four fields every build writes, run pn_tx_fill(PN_TX_UDP, lens): the
    ring is the built ring again."""
    import torch

    stride, frame_off, n = 2048, 8, 300
    chans = _chans64()
    rng = np.random.default_rng(21)
    lens = rng.integers(0, stride - frame_off - 42 + 1, n)
    pay, pb, offs = _pack(lens, seed=21)
    ctx = _ctx(chans)
    d = Dev(n, stride, pay, pb, offs, lens, rng.integers(0, 64, n).astype(np.uint32))
    d.build(ctx, frame_off, ub.UB_PLAIN)
    d.check(chans, frame_off, ub.UB_PLAIN)
    built = d.ring()
    scr = built.copy()
    for i in range(n):
        e = G + i * stride + frame_off
        for o in (16, 24, 38):
            scr[e + o:e + o + 2] = rng.integers(0, 256, 2)
    d.d_ring.copy_(torch.from_numpy(scr))
    ctx.tx_fill(d.d_ring.data_ptr() + G, stride, frame_off, n, lens=d.d_lens, mode=pa.PN_TX_UDP,
                stream=torch.cuda.current_stream())
    assert np.array_equal(d.ring(), built)
    ctx.close()


@pytest.mark.parametrize("mode", MODES)
def test_zero_copy_pinned_payloads_frames_and_index_arrays(mode):
    stride, frame_off, n = 2048, 8, 130
    chans = _chans64()
    pay, pb, offs, lens, chan_ids, _ = _mixed_refusals(n, stride - frame_off - 42, 64, seed=31)
    ctx = _ctx(chans)
    d = Dev(n, stride, pay, pb, offs, lens, chan_ids, pinned=True)
    d.build(ctx, frame_off, mode)
    d.check(chans, frame_off, mode)
    ctx.close()


def test_two_streams_and_a_set_channels_between_builds():
    import torch

    stride, frame_off, n = 2048, 8, 200
    a, b = _chans64(), ub.make_channels(_templates(99, 64)[0])
    pay, pb, offs, lens, chan_ids, _ = _mixed_refusals(n, stride - frame_off - 42, 64, seed=41)
    ctx = _ctx(a)
    d1 = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    d2 = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    d1.build(ctx, frame_off, ub.UB_CSUM, s1)
    d2.build(ctx, frame_off, ub.UB_EFVI, s2)  # back to back on another stream
    ctx.udp_set_channels(b)  # waits for both
    d1.check(a, frame_off, ub.UB_CSUM)
    d2.check(a, frame_off, ub.UB_EFVI)
    d3 = Dev(n, stride, pay, pb, offs, lens, chan_ids)
    d3.build(ctx, frame_off, ub.UB_CSUM, s1)
    d3.check(b, frame_off, ub.UB_CSUM)
    ctx.sync()
    ctx.close()


def test_errors_name_themselves_and_launch_nothing():
    import torch

    stride, frame_off, n = 2048, 8, 64
    chans = _chans64()
    lens = [100] * n
    pay, pb, offs = _pack(lens)
    d = Dev(n, stride, pay, pb, offs, lens, np.zeros(n, np.uint32))
    ctx = pa.RxContext(0)

    def fails(rc, text, fn, *args):
        with pytest.raises(pa.PollnetError) as e:
            fn(*args)
        assert "(%d)" % rc in str(e.value) and text in str(e.value), str(e.value)

    ring, fl = d.d_ring.data_ptr() + G, d.d_flens.data_ptr() + 16
    args = lambda **k: tuple({**dict(p=d.d_pay, pb=pb, o=d.d_offs, l=d.d_lens, c=d.d_chans, r=ring, s=stride,  # noqa: E731
                                     f=frame_off, n=n, m=0, fl=fl), **k}.values())
    fails(-4, "pn_udp_set_channels", ctx.udp_build, *args())  # PN_ENOTABLE: before set_channels
    padded = chans.copy()
    padded["_pad"][3, 5] = 1
    fails(-1, "_pad", ctx.udp_set_channels, padded)
    for at, v in ((12, 0x86), (14, 0x46), (23, 6)):
        wrong = chans.copy()
        wrong["hdr"][63, at] = v
        fails(-1, "not IPv4/UDP", ctx.udp_set_channels, wrong)
    fails(-1, "n_chans must be in [1, PN_UDP_MAX_CHANNELS]", ctx.udp_set_channels, np.zeros(0, pa.UDP_CHANNEL_DTYPE))
    fails(-1, "n_chans must be in [1, PN_UDP_MAX_CHANNELS]", ctx.udp_set_channels, np.tile(chans, 65)[:4097])
    fails(-4, "pn_udp_set_channels", ctx.udp_build, *args())  # a refused set leaves no table
    ctx.udp_set_channels(chans)
    fails(-1, "unknown mode", ctx.udp_build, *args(m=3))
    fails(-1, "layout contract", ctx.udp_build, *args(f=3))
    fails(-1, "layout contract", ctx.udp_build, *args(s=96))  # below frame_off + 96
    fails(-1, "layout contract", ctx.udp_build, *args(s=2056))
    fails(-1, "layout contract", ctx.udp_build, *args(s=65552))
    fails(-1, "aligned", ctx.udp_build, *args(r=ring + 8))
    fails(-1, "aligned", ctx.udp_build, *args(p=d.d_pay.data_ptr() + 4))
    fails(-1, "aligned", ctx.udp_build, *args(o=d.d_offs.data_ptr() + 4))
    fails(-1, "aligned", ctx.udp_build, *args(l=d.d_lens.data_ptr() + 1))
    fails(-1, "aligned", ctx.udp_build, *args(c=d.d_chans.data_ptr() + 2))
    fails(-1, "aligned", ctx.udp_build, *args(fl=fl + 1))
    fails(-1, "NULL", ctx.udp_build, *args(p=None))
    fails(-1, "NULL", ctx.udp_build, *args(o=None))
    fails(-1, "NULL", ctx.udp_build, *args(l=None))
    fails(-1, "NULL", ctx.udp_build, *args(r=None))
    fails(-1, "NULL", ctx.udp_build, *args(fl=None))
    ctx.udp_build(*args(n=0))  # n == 0: PN_OK, nothing written
    torch.cuda.synchronize()
    assert np.array_equal(d.ring(), d.ring0), "a refused call launched"
    assert np.array_equal(d.d_flens.cpu().numpy().view(np.uint16), d.flens0)
    d.build(ctx, frame_off, ub.UB_EFVI)  # and the ctx still works
    d.check(chans, frame_off, ub.UB_EFVI)
    ctx.close()
