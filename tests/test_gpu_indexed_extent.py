"""GPU: pn_classify_indexed where the readable extent ends inside the header window -- small-slot rings, avail
96 .. 128 -- and right behind it, every record bit-exact against the C oracle on the same bytes (inputs and
expected records: tests/indexed_np.py; tests/test_indexed_extent_np.py shows on the CPU that those inputs hold the
cases).  At such sizes every wave loads its windows per lane and a segment may end in the one 16-B chunk that
avail ends in.  Also: waves with no in-class offset, offsets named twice and backwards, the header-only
(pn_set_verify(ctx, 0)) kernels in the per-lane form, and the strided entry point on the same small slots."""
import numpy as np
import pytest

import pollnet_amd as pa
from oracle import pyoracle as orc

import indexed_np as ixn
from test_indexed_extent_np import AVAILS, CLASSES, FILL_SEEDS, SEED_AVAILS, SMALL_SLOTS, window_form_cases

pytestmark = pytest.mark.gpu


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
    yield c
    c.close()


@pytest.fixture
def verifying(ctx, request):
    """ctx with pn_set_verify as the test's `verify` parameter says, back on afterwards."""
    ctx.set_verify(request.node.callspec.params["verify"])
    yield ctx
    ctx.set_verify(True)


def _indexed(torch, ctx, buf, offsets, eth_mod16, avail, canary=13):
    """Records of one launch into a canary-padded buffer; buf: numpy bytes or a device tensor of them."""
    n = len(offsets)
    dev = buf if torch.is_tensor(buf) else torch.from_numpy(np.array(buf)).cuda()
    assert dev.data_ptr() % 128 == 0  # Case.win_phase assumes it
    offs = torch.from_numpy(np.array(offsets, dtype=np.uint64).view(np.int64)).cuda()
    res = torch.full(((n + canary) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.classify_indexed(dev, offs, eth_mod16, n, avail, res, torch.cuda.current_stream())
    torch.cuda.synchronize()
    out = res.cpu().numpy()
    assert (out[n * 16:] == 0xAB).all(), "kernel wrote past n records"
    return out[: n * 16].view(pa.RESULT_DTYPE).copy()


def _same(got, exp, what="", names=None):
    if np.array_equal(got, exp):
        return
    bad = np.nonzero(got != exp)[0]
    i = int(bad[0])
    nm = f" ({names[i]})" if names is not None else ""
    raise AssertionError(f"{what}: {len(bad)} of {len(exp)} records differ; first #{i}{nm}: gpu={got[i]} expected={exp[i]}")


def _want(exp, verify):
    return exp if verify else ixn.release(exp)


@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("avail", AVAILS)
@pytest.mark.parametrize("eth_mod16", CLASSES)
def test_window_forms(torch_cuda, verifying, eth_mod16, avail, verify):
    """The edge list of (eth_mod16, avail) in 8-frame waves: spaced (every edge at each 16-B phase of a line),
    packed from base + eth_mod16 (for class 0 the first wave's block would start below base) and behind one chunk,
    and packed 16 times over with a ragged last wave.  avail < 14 - MIS + 112: every wave loads per lane and avail
    ends inside the window; above it the waves load cooperatively, but for the one at the buffer start."""
    for name, c in window_form_cases(eth_mod16, avail).items():
        got = _indexed(torch_cuda, verifying, c.buf, c.offsets, eth_mod16, avail)
        _same(got, _want(c.exp, verify), name, c.names)


@pytest.mark.parametrize("n", [20000, 65573])
@pytest.mark.parametrize("eth_mod16,avail", [(2, 100), (0, 98), (14, 126), (8, 2046)])
def test_window_forms_in_wider_waves(torch_cuda, ctx, eth_mod16, avail, n):
    """The spaced frames named n times in a random order: 16-frame waves at 20,000 and 64-frame waves at 65,573
    (frames_per_wave), each wave a mix of every edge and phase."""
    c = ixn.spaced(eth_mod16, avail, FILL_SEEDS[0])
    pick = np.random.default_rng(n + avail).integers(0, c.n, n)
    got = _indexed(torch_cuda, ctx, c.buf, c.offsets[pick], eth_mod16, avail)
    _same(got, c.exp[pick], "tiled", [c.names[i] for i in pick])


@pytest.mark.parametrize("avail", SEED_AVAILS)
@pytest.mark.parametrize("eth_mod16", CLASSES)
def test_bytes_outside_avail_do_not_matter(torch_cuda, ctx, eth_mod16, avail):
    """The same frames with every byte outside each [eth, eth + avail) drawn from another seed."""
    a, b = (ixn.spaced(eth_mod16, avail, s) for s in FILL_SEEDS)
    assert not np.array_equal(a.buf, b.buf)
    ga = _indexed(torch_cuda, ctx, a.buf, a.offsets, eth_mod16, avail)
    gb = _indexed(torch_cuda, ctx, b.buf, b.offsets, eth_mod16, avail)
    _same(ga, a.exp, "seed %d" % FILL_SEEDS[0], a.names)
    _same(gb, b.exp, "seed %d" % FILL_SEEDS[1], b.names)
    _same(ga, gb, "between the seeds", a.names)


@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("stride,frame_off", SMALL_SLOTS)
def test_equals_strided_at_small_slots(torch_cuda, verifying, stride, frame_off, verify):
    """The same slot bytes through pn_classify and through pn_classify_indexed with offsets i*stride + frame_off
    and avail = stride - frame_off: equal records, and the oracle's."""
    torch = torch_cuda
    slots = ixn.small_slots(stride, frame_off)
    n = len(slots)
    e, m = ixn.conn_entries()
    exp = _want(orc.classify_batch(np.ascontiguousarray(slots), stride, frame_off, n, e, m, ixn.MAX_CONN), verify)
    dev = torch.from_numpy(np.array(slots).reshape(-1)).cuda()
    res = torch.full(((n + 5) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    verifying.classify(dev, stride, frame_off, n, res, torch.cuda.current_stream())
    torch.cuda.synchronize()
    out = res.cpu().numpy()
    assert (out[n * 16:] == 0xAB).all(), "pn_classify wrote past n records"
    strided = out[: n * 16].view(pa.RESULT_DTYPE).copy()
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(frame_off)
    got = _indexed(torch, verifying, dev, offsets, frame_off % 16, stride - frame_off)
    _same(strided, exp, "pn_classify")
    _same(got, exp, "pn_classify_indexed")
    _same(got, strided, "indexed against strided")


@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("n", [200, 203])
@pytest.mark.parametrize("avail", [100, 2048])
def test_out_of_class_waves(torch_cuda, verifying, avail, n, verify):
    """64 consecutive offsets out of class (eight whole 8-frame waves: nothing to load), a wave whose first 5
    lanes are, and everything from offset 192 on (the last wave, of 3 frames at n = 203).  Out of class: another
    class inside the buffer, or far outside it -- no byte of either is read.  Exactly the BADOFF record there,
    the oracle's everywhere else."""
    eth_mod16 = 2
    c = ixn.spaced(eth_mod16, avail, FILL_SEEDS[0])
    idx = np.arange(n) % c.n
    offsets, exp = c.offsets[idx].copy(), _want(c.exp[idx], verify)
    bad = np.zeros(n, bool)
    bad[64:128] = bad[128:133] = bad[192:] = True
    for j, i in enumerate(np.flatnonzero(bad)):
        offsets[i] = offsets[i] + np.uint64(2 * (1 + j % 7)) if j % 3 else np.uint64((1 << 44) + 16 * j + 2 * (2 + j % 7))
    assert ((offsets[bad] % 16) != eth_mod16).all() and len(set((offsets[bad] % 16).tolist())) == 7
    exp[bad] = ixn.badoff_record()
    assert not (exp["flags"][~bad] & ixn.BADOFF).any() and (exp["flags"][~bad] & ixn.HIT).any()
    got = _indexed(torch_cuda, verifying, c.buf, offsets, eth_mod16, avail)
    _same(got, exp, "out of class")
    assert (got[bad] == ixn.badoff_record()).all()


@pytest.mark.parametrize("eth_mod16,avail", [(2, 100), (0, 111), (12, 128), (6, 2048)])
def test_duplicate_and_reversed_offsets(torch_cuda, ctx, eth_mod16, avail):
    """The spaced buffer's offsets backwards, every third named twice: records follow the offsets' order."""
    c = ixn.spaced(eth_mod16, avail, FILL_SEEDS[1])
    idx = np.repeat(np.arange(c.n)[::-1], np.where(np.arange(c.n) % 3 == 0, 2, 1))
    assert len(idx) > c.n and (np.diff(idx) <= 0).all() and (np.diff(idx) == 0).any()
    got = _indexed(torch_cuda, ctx, c.buf, c.offsets[idx], eth_mod16, avail)
    _same(got, c.exp[idx], "reversed", [c.names[i] for i in idx])
