"""GPU: the strided verifying paths over every segment length a slot can hold, in slots whose every other byte is
poison (tests/strided_np.py; tests/test_strided_extent_np.py shows on the CPU that those rings put a summed extent
at, one word before and one word behind every point where the stream changes its behaviour, and that a record
depends on the bytes behind its frame only for an odd length).  pn_classify, pn_classify_indexed, the notify form,
the resident service, the release path, pn_tx_fill in TCP mode and pn_udp_classify (strided and indexed): every
record bit-exact against the C oracle or the numpy UDP model on the same bytes, every ring byte after a TX fill
equal to the built ring.  A sum that takes in a word, a dword or a 16-B chunk too many -- or too few -- changes
tcp_fold here, where trailing zeros would hide it."""
import time
import warnings

import numpy as np
import pytest

import pollnet_amd as pa
from oracle import pyoracle as orc

import indexed_np as ixn
import strided_np as sn
from test_strided_extent_np import scrambled

pytestmark = pytest.mark.gpu

CANARY = 0xAB
FOUR = [(2, 2048), (18, 2048), (2, 2064), (2, 4096)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    c = pa.RxContext(0)
    e, m = ixn.conn_entries()
    c.set_conn_entries(e, m, ixn.MAX_CONN)
    c.udp_set_subs(sn.udp_subs())
    yield c
    c.set_verify(True)
    c.close()


def frames_per_wave(n):
    """frames_per_wave of pollnet_amd/csrc/frame_pass.hpp."""
    fpw = 64
    while fpw > 8 and (n + fpw - 1) // fpw < 1024:
        fpw >>= 1
    return fpw


def _tensor(torch, a):
    """A CPU tensor over a (read-only, shared) ring array: it is only read from."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(a.reshape(-1))


def _upload(torch, ring):
    dev = _tensor(torch, ring.slots).cuda()
    assert dev.data_ptr() % 128 == 0  # strided_np.geometry assumes it
    return dev


def _records(torch, out, n, dtype, what):
    got = out.cpu().numpy()
    assert (got[n * 16:] == CANARY).all(), f"{what} wrote past {n} records"
    return got[:n * 16].view(dtype).copy()


def _results(torch, n, pinned=False):
    r = torch.full(((n + 11) * 16,), CANARY, dtype=torch.uint8)
    return r.pin_memory() if pinned else r.cuda()


def _classify(torch, ctx, dev, ring, n=None):
    n = ring.n if n is None else n
    res = _results(torch, n)
    ctx.classify(dev, ring.stride, ring.frame_off, n, res, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return _records(torch, res, n, pa.RESULT_DTYPE, "pn_classify")


def _offsets(torch, ring):
    o = np.arange(ring.n, dtype=np.uint64) * np.uint64(ring.stride) + np.uint64(ring.frame_off)
    return torch.from_numpy(o.view(np.int64)).cuda()


def _same(got, exp, ring, what):
    exp = exp[:len(got)]
    if np.array_equal(got, exp):
        return
    bad = np.flatnonzero(got != exp)
    i = int(bad[0])
    more = "; ".join(ring.describe(int(j)) for j in bad[1:4])
    raise AssertionError(f"{what}: {len(bad)} of {len(exp)} records differ; first {ring.describe(i)}: gpu={got[i]} "
                         f"expected={exp[i]}; then {more}")


def _same_bytes(got, exp, ring, what):
    got, exp = got.reshape(ring.n, ring.stride), exp.reshape(ring.n, ring.stride)
    if np.array_equal(got, exp):
        return
    bad = np.flatnonzero((got != exp).any(1))
    i = int(bad[0])
    cols = np.flatnonzero(got[i] != exp[i])
    raise AssertionError(f"{what}: {len(bad)} of {ring.n} slots differ; first {ring.describe(i)}: slot bytes {cols[:8].tolist()} "
                         f"gpu={got[i, cols[:8]].tolist()} expected={exp[i, cols[:8]].tolist()}")


def wait_token(word_np, token, torch, timeout_s=10.0):
    t0 = time.time()
    while int(word_np[0]) != token:  # the acquire side: records are read only after this
        if time.time() - t0 > timeout_s:
            torch.cuda.synchronize()
            raise AssertionError(f"notify word {int(word_np[0])} never became {token}")


# ---------------------------------------------------------------- pn_classify ----
@pytest.mark.parametrize("order", sn.ORDERS)
@pytest.mark.parametrize("frame_off,stride", sn.LAYOUTS)
def test_classify_sweep(torch_cuda, ctx, frame_off, stride, order):
    """Every length once: ascending (waves of near-equal extents; above s0 + 1024 the full-size and pipelined
    forms), shuffled, and alternating (every batch of 8 mixes short and long frames: the skipping form)."""
    r = sn.sweep_ring(frame_off, stride, order)
    _same(_classify(torch_cuda, ctx, _upload(torch_cuda, r), r), r.exp, r, f"pn_classify {order}")


@pytest.mark.parametrize("target,fpw", [(10000, 8), (18000, 16), (34000, 32), (65600, 64)])
@pytest.mark.parametrize("order", ["shuffled", "ascending"])
@pytest.mark.parametrize("frame_off,stride", sn.TILED)
def test_classify_sweep_in_wider_waves(torch_cuda, ctx, frame_off, stride, order, target, fpw):
    """A ring repeated until a wave takes 8, 16, 32 and 64 frames (16 from 16,369 frames on, 32 from 32,737, 64
    from 65,473), every repeat on other lanes; then the same buffer with n cut to end inside a wave and inside a
    batch of 8.  Shuffled: a wide wave always holds a short frame (the skipping form).  Ascending: whole waves of
    long frames at every width (the full-size and pipelined forms, whose look-ahead runs past a ragged last wave)."""
    r = sn.sweep_ring(frame_off, stride, order)
    t = sn.tile(r, -(-target // (r.n - 1)))
    dev = _upload(torch_cuda, t)
    ns = [t.n] + [t.n - 64 + (k - t.n) % 64 for k in (1, 7, 9, 63)]
    assert t.n >= target and [n % 64 for n in ns[1:]] == [1, 7, 9, 63]
    for n in ns:
        assert 0 < n <= t.n and frames_per_wave(n) == fpw
        _same(_classify(torch_cuda, ctx, dev, t, n), t.exp, t, f"pn_classify n={n} ({fpw} frames per wave)")


@pytest.mark.parametrize("frame_off,stride", sn.OFF_GRID)
def test_classify_off_the_line_grid(torch_cuda, ctx, frame_off, stride):
    """A stride that is no multiple of 128: s0 differs from slot to slot, and over 8 repeats of an odd-length
    ring every frame has had every s0."""
    t = sn.tile(sn.sweep_ring(frame_off, stride, "shuffled"), 8)
    _same(_classify(torch_cuda, ctx, _upload(torch_cuda, t), t), t.exp, t, "pn_classify x8")


@pytest.mark.parametrize("order", ["shuffled", "ascending"])
@pytest.mark.parametrize("frame_off,stride", FOUR)
def test_indexed_equals_strided(torch_cuda, ctx, frame_off, stride, order):
    torch = torch_cuda
    r = sn.sweep_ring(frame_off, stride, order)
    dev = _upload(torch, r)
    strided = _classify(torch, ctx, dev, r)
    res = _results(torch, r.n)
    ctx.classify_indexed(dev, _offsets(torch, r), frame_off % 16, r.n, r.avail, res, torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = _records(torch, res, r.n, pa.RESULT_DTYPE, "pn_classify_indexed")
    _same(got, r.exp, r, "pn_classify_indexed")
    _same(got, strided, r, "indexed against strided")


@pytest.mark.parametrize("frame_off,stride", [(2, 2048), (18, 2048)])
def test_classify_notify(torch_cuda, ctx, frame_off, stride):
    """The frames around every stream boundary through pn_classify_notify, slots and records in pinned memory."""
    torch = torch_cuda
    r = sn.sweep_ring(frame_off, stride, "shuffled")
    sub = r.take(sn.band_subset(r, pa.rx.PN_NOTIFY_MAX_FRAMES))
    slots = _tensor(torch, sub.slots).pin_memory()
    assert slots.data_ptr() % 128 == 0
    word = torch.zeros(16, dtype=torch.int32).pin_memory()
    st = torch.cuda.Stream()
    for tok in (21, 22):
        res = _results(torch, sub.n, pinned=True)
        ctx.classify_notify(slots, stride, frame_off, sub.n, res, word, tok, st)
        wait_token(word.numpy(), tok, torch)
        got = res.numpy().copy()
        assert (got[sub.n * 16:] == CANARY).all()
        _same(got[:sub.n * 16].view(pa.RESULT_DTYPE), sub.exp, sub, f"pn_classify_notify token {tok}")
    st.synchronize()


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("frame_off,stride", [(2, 2048), (18, 2048)])
def test_service(torch_cuda, ctx, frame_off, stride, pinned):
    """The resident service: the whole sweep in one post on the latency tier (up to 4,096 frames), and three
    repeats of it in one post, which helper waves share.  Frames and records in device or pinned host memory."""
    torch = torch_cuda
    r = sn.sweep_ring(frame_off, stride, "shuffled")
    t = sn.tile(r, 3)
    assert r.n <= 4096 < t.n
    svc = pa.RxService(ctx, stride, frame_off)
    try:
        for ring in (r, t):
            flat = _tensor(torch, ring.slots)
            frames = flat.pin_memory() if pinned else flat.cuda()
            assert frames.data_ptr() % 128 == 0
            res = _results(torch, ring.n, pinned)
            svc.classify(frames, ring.n, res)
            _same(_records(torch, res, ring.n, pa.RESULT_DTYPE, "the service"), ring.exp, ring, f"service post of {ring.n}")
    finally:
        svc.close()


@pytest.mark.parametrize("frame_off,stride", [(2, 2048), (2, 2064)])
def test_release_path(torch_cuda, ctx, frame_off, stride):
    """pn_set_verify(ctx, 0): header lines only.  Off the 128-B grid the line a header lies in moves from slot to
    slot."""
    r = sn.sweep_ring(frame_off, stride, "shuffled")
    t = sn.tile(r, 8)
    ctx.set_verify(False)
    try:
        for ring in (r, t):
            _same(_classify(torch_cuda, ctx, _upload(torch_cuda, ring), ring), ixn.release(ring.exp), ring, "release path")
    finally:
        ctx.set_verify(True)


# ---------------------------------------------------------------- pn_tx_fill ----
def _tx_fill(torch, ctx, slots, ring, lens=None):
    d = torch.from_numpy(slots.reshape(-1)).cuda()
    assert d.data_ptr() % 128 == 0
    l = None if lens is None else torch.from_numpy(lens.astype(np.uint16).view(np.int16)).cuda()
    ctx.tx_fill(d, ring.stride, ring.frame_off, ring.n, l, pa.PN_TX_TCP, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("frame_off,stride", sn.LAYOUTS + [(14, 2048)])
def test_tx_fill_sweep(torch_cuda, ctx, frame_off, stride):
    """A sender's ring with both checksum fields scrambled: the fill restores the built ring, every poison byte
    and every frame that must stay untouched included.  Then with tot_len scrambled too and lens = tot_len - 40:
    the oracle's ring."""
    r = sn.sweep_ring(frame_off, stride, "shuffled", True)
    _same_bytes(_tx_fill(torch_cuda, ctx, scrambled(r), r), r.slots, r, "pn_tx_fill")
    s = scrambled(r, tot_too=True)
    lens = ((r.tot - 40) & 0xFFFF).astype(np.uint16)
    exp = s.copy()
    orc.tx_fill_batch(exp, stride, frame_off, r.n, lens, orc.TX_TCP)
    assert np.array_equal(exp[r.swept], r.slots[r.swept])  # which restores the swept frames as well
    _same_bytes(_tx_fill(torch_cuda, ctx, s, r, lens), exp, r, "pn_tx_fill with lens")


def test_tx_fill_two_launch_form(torch_cuda, ctx):
    """Above 65,536 frames: patch records, then a patch launch."""
    t = sn.tile(sn.sweep_ring(2, 2048, "shuffled", True), 33)
    assert t.n > 65536
    _same_bytes(_tx_fill(torch_cuda, ctx, scrambled(t), t), t.slots, t, "pn_tx_fill, two launches")


@pytest.mark.parametrize("frame_off,stride", [(2, 2048), (18, 2048)])
def test_tx_fill_notify(torch_cuda, ctx, frame_off, stride):
    torch = torch_cuda
    r = sn.sweep_ring(frame_off, stride, "shuffled", True)
    sub = r.take(sn.band_subset(r, pa.rx.PN_NOTIFY_MAX_FRAMES))
    b = torch.from_numpy(scrambled(sub).reshape(-1)).pin_memory()
    word = torch.zeros(16, dtype=torch.int32).pin_memory()
    st = torch.cuda.Stream()
    ctx.tx_fill_notify(b, stride, frame_off, sub.n, word, 31, stream=st)
    wait_token(word.numpy(), 31, torch)
    _same_bytes(b.numpy().copy(), sub.slots, sub, "pn_tx_fill_notify")
    st.synchronize()


# ---------------------------------------------------------------- pn_udp_classify ----
def _udp_classify(torch, ctx, dev, ring):
    res = _results(torch, ring.n)
    ctx.udp_classify(dev, ring.stride, ring.frame_off, ring.n, res, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return _records(torch, res, ring.n, pa.UDP_RESULT_DTYPE, "pn_udp_classify")


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("kind", ["all_summed", "compact"])
@pytest.mark.parametrize("frame_off,stride", sn.UDP_LAYOUTS)
def test_udp_classify_sweep(torch_cuda, ctx, frame_off, stride, kind, order):
    """Every payload length once.  all_summed: the pipelined form (2-KiB slots) and every load issued (4-KiB);
    compact: every wave streams another subset of its frames on permuted lanes."""
    u = sn.udp_ring(frame_off, stride, kind, 5, order)
    _same(_udp_classify(torch_cuda, ctx, _upload(torch_cuda, u), u), u.exp, u, f"pn_udp_classify {kind} {order}")


@pytest.mark.parametrize("kind,order", [("compact", "shuffled"), ("all_summed", "ascending")])
def test_udp_classify_in_64_frame_waves(torch_cuda, ctx, kind, order):
    """Above 65,472 frames: 64-frame waves that compact, and whole 64-frame waves of long datagrams (pipelined)."""
    t = sn.tile(sn.udp_ring(2, 2048, kind, 5, order), 33)
    assert t.n > 65536 and frames_per_wave(t.n) == 64
    _same(_udp_classify(torch_cuda, ctx, _upload(torch_cuda, t), t), t.exp, t, f"pn_udp_classify {kind} x33")


@pytest.mark.parametrize("kind,order", [("all_summed", "ascending"), ("compact", "shuffled")])
@pytest.mark.parametrize("frame_off,stride", FOUR)
def test_udp_indexed_equals_strided(torch_cuda, ctx, frame_off, stride, kind, order):
    torch = torch_cuda
    u = sn.udp_ring(frame_off, stride, kind, 5, order)
    dev = _upload(torch, u)
    strided = _udp_classify(torch, ctx, dev, u)
    res = _results(torch, u.n)
    ctx.udp_classify_indexed(dev, _offsets(torch, u), frame_off % 16, u.n, u.avail, res, torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = _records(torch, res, u.n, pa.UDP_RESULT_DTYPE, "pn_udp_classify_indexed")
    _same(got, u.exp, u, "pn_udp_classify_indexed")
    _same(got, strided, u, "indexed against strided")
