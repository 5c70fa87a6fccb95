"""GPU: the conn-table probe of every TCP classify entry point (probe_finish, rx_classify.hpp) on the tables and
batches of tests/probe_np.py -- every tier of the walk, every round trip up to the fourth, as many groups as a wave
has lanes, runs that end on an EmptyKey, on the array's last entry and on the next home slot's key, keys that
differ in one word only, conn_ids on both sides of max_conn -- at 8, 16, 32 and 64 live lanes per wave
(tests/test_probe_np.py shows on the CPU that the batches hold all of that).  pn_classify, the release path,
pn_classify_indexed in order and reversed, pn_classify_notify, and the resident service with its helper grid: the
whole record array bit-exact against the C oracle, guard records behind it.  Then the UDP subscription probe
(udp_probe, udp_classify.hpp) on subscription sets with a chain of 12, a chain that wraps over the table's end, and
a table at exactly half load, against the numpy model, which knows nothing of the table's layout.

pn_classify_notify takes at most 1,024 frames, where frames_per_wave gives 8: its kernels cannot be run at another
width.  The service's release path is the cheapest way to 64 live lanes: svc_fpw gives it 64 at any post size."""
import time

import numpy as np
import pytest

import pollnet_amd as pa

import probe_np as pn

pytestmark = pytest.mark.gpu

CANARY = 0xAB
STRIDE, OFF = 128, 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    c = pa.RxContext(0)
    yield c
    c.set_verify(True)
    c.close()


def _results(torch, n, pinned=False):
    r = torch.full(((n + 11) * 16,), CANARY, dtype=torch.uint8)
    return r.pin_memory() if pinned else r.cuda()


def _records(res, n, dtype, what):
    got = res.cpu().numpy()
    assert (got[n * 16:] == CANARY).all(), f"{what} wrote past {n} records"
    return got[:n * 16].view(dtype).copy()


def _same(got, exp, tb, idx, w, what):
    if np.array_equal(got, exp):
        return
    bad = np.flatnonzero(got != exp)
    i = int(bad[0])
    j = int(idx[i])
    raise AssertionError(
        f"{what}, table {tb.name}: {len(bad)} of {len(exp)} records differ; first frame {i} (lane {i % w} of {w}): key "
        f"{tb.lookups[j]:#014x}, home slot {int(tb.home[j])}, stops {int(tb.depth[j])} entries on (tier "
        f"{pn.tier(int(tb.depth[j]))}, round trip {pn.round_trip(int(tb.depth[j]))}), {tb.outcome[j]}: gpu={got[i]} "
        f"oracle={exp[i]}")


def _offsets(torch, n, stride, off, reverse=False):
    o = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(off)
    return torch.from_numpy((o[::-1].copy() if reverse else o).view(np.int64)).cuda()


def _classify(torch, ctx, tb, w, n, verify=True, stride=STRIDE, off=OFF, how="strided"):
    """One batch of width w through one entry point, against the oracle."""
    slots, exp = pn.batch(tb, w, n, stride, off)
    idx = pn.batch_index(tb, w, n)
    if not verify:
        exp = pn.release(exp)
    dev = torch.from_numpy(slots.reshape(-1)).cuda()
    res = _results(torch, n)
    if how == "strided":
        ctx.classify(dev, stride, off, n, res, torch.cuda.current_stream())
    else:
        rev = how == "reversed"
        ctx.classify_indexed(dev, _offsets(torch, n, stride, off, rev), off % 16, n, stride - off, res,
                             torch.cuda.current_stream())
        if rev:
            exp, idx = exp[::-1], idx[::-1]
    torch.cuda.synchronize()
    _same(_records(res, n, pa.RESULT_DTYPE, how), exp, tb, idx, w, f"{how} n={n} verify={verify}")


def _each_table(ctx):
    for tb in pn.tables():
        ctx.set_conn_entries(tb.entries, tb.mask, tb.max_conn)
        yield tb


@pytest.mark.parametrize("last", [0, 1], ids=["last_wave_1", "last_wave_w-1"])
@pytest.mark.parametrize("w", pn.WIDTHS)
def test_classify(torch_cuda, ctx, w, last):
    """pn_classify, verifying, every table: n just inside the width's range, the last wave 1 or w - 1 lanes wide."""
    n = pn.batch_sizes(w)[last]
    assert pn.frames_per_wave(n) == w
    ctx.set_verify(True)
    for tb in _each_table(ctx):
        _classify(torch_cuda, ctx, tb, w, n)


@pytest.mark.parametrize("w", pn.WIDTHS)
def test_release_path(torch_cuda, ctx, w):
    """pn_set_verify(ctx, 0): the header-only kernels carry their own copy of the probe."""
    n = pn.batch_sizes(w)[1]
    ctx.set_verify(False)
    try:
        for tb in _each_table(ctx):
            _classify(torch_cuda, ctx, tb, w, n, verify=False)
    finally:
        ctx.set_verify(True)


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "release"])
def test_second_window_loader(torch_cuda, ctx, verify):
    """2,048-byte slots at frame_off 18: the window block off the line grid, the other strided loader."""
    ctx.set_verify(verify)
    try:
        for tb in _each_table(ctx):
            _classify(torch_cuda, ctx, tb, 8, 1023, verify, stride=2048, off=18)
    finally:
        ctx.set_verify(True)


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "release"])
@pytest.mark.parametrize("how", ["in_order", "reversed"])
@pytest.mark.parametrize("w", [8, 64])
def test_indexed(torch_cuda, ctx, w, how, verify):
    """pn_classify_indexed over the strided batch's own slots, offsets[i] = i * stride + frame_off, and the same
    frames from the last to the first."""
    n = pn.batch_sizes(w)[1] if w == 64 else 4095
    assert pn.frames_per_wave(n) == w
    ctx.set_verify(verify)
    try:
        for tb in _each_table(ctx):
            _classify(torch_cuda, ctx, tb, w, n, verify, how=how)
    finally:
        ctx.set_verify(True)


def _wait_token(word_np, token, torch, timeout_s=10.0):
    t0 = time.time()
    while int(word_np[0]) != token:  # the acquire side: records are read only after this
        if time.time() - t0 > timeout_s:
            torch.cuda.synchronize()
            raise AssertionError(f"notify word {int(word_np[0])} never became {token}")


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "release"])
def test_classify_notify(torch_cuda, ctx, verify):
    """The completion-word kernels, at their limit of 1,024 frames and with a last wave of one frame (8 lanes: the
    only width the limit allows)."""
    torch = torch_cuda
    word = torch.zeros(16, dtype=torch.int32).pin_memory()
    st = torch.cuda.Stream()
    ctx.set_verify(verify)
    try:
        tok = 40
        for tb in _each_table(ctx):
            for n in (pa.rx.PN_NOTIFY_MAX_FRAMES, pa.rx.PN_NOTIFY_MAX_FRAMES - 7):
                assert pn.frames_per_wave(n) == 8
                slots, exp = pn.batch(tb, 8, n)
                frames = torch.from_numpy(slots.reshape(-1)).pin_memory()
                res = _results(torch, n, pinned=True)
                tok += 1
                ctx.classify_notify(frames, STRIDE, OFF, n, res, word, tok, st)
                _wait_token(word.numpy(), tok, torch)
                got = res.numpy().copy()
                assert (got[n * 16:] == CANARY).all()
                _same(got[:n * 16].view(pa.RESULT_DTYPE), exp if verify else pn.release(exp), tb, pn.batch_index(tb, 8, n),
                      8, f"pn_classify_notify n={n} verify={verify}")
        st.synchronize()
    finally:
        ctx.set_verify(True)


SERVICE_POSTS = (64, 513, 1025, 2049, 4099)


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "release"])
def test_service(torch_cuda, ctx, verify):
    """The resident service: verifying posts of 64, 513, 1,025 and 2,049 frames run 8, 16, 32 and 64 lanes a group,
    the release path 64 at every size; 4,099 frames also run on the helper grid."""
    torch = torch_cuda
    assert [pn.svc_fpw(n, True) for n in SERVICE_POSTS] == [8, 16, 32, 64, 64] and SERVICE_POSTS[-1] > 64 * pn.SVC_WAVES
    ctx.set_verify(verify)
    try:
        for tb in _each_table(ctx):
            svc = pa.RxService(ctx, STRIDE, OFF)
            try:
                for n in SERVICE_POSTS:
                    w = pn.svc_fpw(n, verify)
                    slots, exp = pn.batch(tb, w, n)
                    frames = torch.from_numpy(slots.reshape(-1)).cuda()
                    res = _results(torch, n)
                    svc.classify(frames, n, res)
                    _same(_records(res, n, pa.RESULT_DTYPE, "the service"), exp if verify else pn.release(exp), tb,
                          pn.batch_index(tb, w, n), w, f"service post of {n} verify={verify}")
            finally:
                svc.close()
    finally:
        ctx.set_verify(True)


# ---------------------------------------------------------------- the UDP subscription probe ----
UDP_SIZES = {8: 3001, 64: pn.batch_sizes(64)[1]}


@pytest.mark.parametrize("verify", [True, False], ids=["verify", "release"])
@pytest.mark.parametrize("w", [8, 64])
@pytest.mark.parametrize("n_subs", [32, 33])
def test_udp_probe(torch_cuda, ctx, n_subs, w, verify):
    """pn_udp_classify and pn_udp_classify_indexed: every subscribed pair down its chain, absent pairs that walk a
    whole chain -- over the table's end -- to the empty entry, and pairs one byte away from a subscribed one."""
    torch = torch_cuda
    n = UDP_SIZES[w]
    assert pn.frames_per_wave(n) == w
    subs, looks = pn.udp_case(n_subs)
    slots, exp = pn.udp_batch(n_subs, n, STRIDE, OFF, verify)
    ctx.udp_set_subs(subs)
    ctx.set_verify(verify)
    try:
        dev = torch.from_numpy(slots.reshape(-1)).cuda()
        for how in ("strided", "indexed"):
            res = _results(torch, n)
            if how == "strided":
                ctx.udp_classify(dev, STRIDE, OFF, n, res, torch.cuda.current_stream())
            else:
                ctx.udp_classify_indexed(dev, _offsets(torch, n, STRIDE, OFF), OFF % 16, n, STRIDE - OFF, res,
                                         torch.cuda.current_stream())
            torch.cuda.synchronize()
            got = _records(res, n, pa.UDP_RESULT_DTYPE, how)
            if not np.array_equal(got, exp):
                bad = np.flatnonzero(got != exp)
                i = int(bad[0])
                raise AssertionError(f"pn_udp_classify {how}, {n_subs} subscriptions, n={n}: {len(bad)} records differ; "
                                     f"first frame {i} (lane {i % w}): gpu={got[i]} expected={exp[i]}")
    finally:
        ctx.set_verify(True)
