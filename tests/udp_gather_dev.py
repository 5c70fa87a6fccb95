"""The device side of the gather tests (test-only helper, shared by tests/test_gpu_udp_gather.py and
tests/test_gpu_udp_gather_indexed.py): one call's buffers, each output a non-constant canary with guard entries on
both sides, and the comparison of every output, whole, against tests/udp_gather_np.py."""
import numpy as np

import pollnet_amd as pa

import udp_gather_np as ug

G = 256     # guard bytes before the frames and on both sides of the payload buffer
GE = 16     # guard entries on both sides of each index array
TOTAL0 = np.array([(0x1111111111111111, 0x22222222, 0x33333333)] * 3, ug.UDP_GATHER_TOTAL_DTYPE)


def canary(nbytes, seed=0xCA):
    return np.random.default_rng(seed).integers(1, 256, nbytes, dtype=np.uint8)


class Gather:
    """buf: the bytes the frames lie in (slot 0 / base at its first byte); records: UDP_RESULT_DTYPE, host array or a
    device tensor of n records; cap: payload_cap."""

    def __init__(self, buf, n, cap, pinned=False, src_index=True, seed=1):
        import torch

        self.torch, self.n, self.cap, self.pinned = torch, n, cap, pinned
        self.put = (lambda a: torch.from_numpy(a).pin_memory()) if pinned else (lambda a: torch.from_numpy(a).cuda())
        self.buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        self.d_buf = self.put(np.concatenate([canary(G, 2), self.buf, canary(G, 3)]))
        rng = np.random.default_rng(seed)
        self.pay0 = canary(G + cap + G, seed + 10)
        self.offs0 = rng.integers(1, 1 << 62, n + 2 * GE).astype(np.uint64)
        self.lens0 = rng.integers(1, 1 << 16, n + 2 * GE).astype(np.uint16)
        self.subs0 = rng.integers(1, 1 << 32, n + 2 * GE).astype(np.uint32)
        self.src0 = rng.integers(1, 1 << 32, n + 2 * GE).astype(np.uint32) if src_index else None
        self.d_pay = self.put(self.pay0.copy())
        self.d_offs = self.put(self.offs0.copy().view(np.int64))
        self.d_lens = self.put(self.lens0.copy().view(np.int16))
        self.d_subs = self.put(self.subs0.copy().view(np.int32))
        self.d_src = None if self.src0 is None else self.put(self.src0.copy().view(np.int32))
        self.d_total = self.put(TOTAL0.copy().view(np.uint8))
        self.d_rec = None
        self.d_idx = None

    def frames_ptr(self):
        return self.d_buf.data_ptr() + G

    def records(self, rec):
        """Host records for the next gather (a device copy is made)."""
        self.rec = np.ascontiguousarray(rec)
        self.d_rec = self.put(self.rec.view(np.uint8).copy())
        return self

    def classify(self, ctx, stride, frame_off, stream=None):
        torch = self.torch
        self.d_rec = torch.zeros(max(self.n, 1) * 16, dtype=torch.uint8)
        self.d_rec = self.d_rec.pin_memory() if self.pinned else self.d_rec.cuda()
        ctx.udp_classify(self.frames_ptr(), stride, frame_off, self.n, self.d_rec,
                         stream if stream is not None else torch.cuda.current_stream())
        self.rec = None
        return self

    def classify_indexed(self, ctx, offsets, eth_mod16, avail):
        torch = self.torch
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        self.d_idx = self.put(self.offsets.view(np.int64).copy())
        self.d_rec = torch.zeros(max(self.n, 1) * 16, dtype=torch.uint8)
        self.d_rec = self.d_rec.pin_memory() if self.pinned else self.d_rec.cuda()
        ctx.udp_classify_indexed(self.frames_ptr(), self.d_idx, eth_mod16, self.n, avail, self.d_rec,
                                 torch.cuda.current_stream())
        self.rec = None
        return self

    def _outs(self):
        return (self.d_pay.data_ptr() + G, self.cap, self.d_offs.data_ptr() + 8 * GE, self.d_lens.data_ptr() + 2 * GE,
                self.d_subs.data_ptr() + 4 * GE, None if self.d_src is None else self.d_src.data_ptr() + 4 * GE,
                self.d_total.data_ptr() + 16)

    def gather(self, ctx, stride, frame_off, stream=None, n=None):
        self.eth_of, self.avail = ug.strided(stride, frame_off), stride - frame_off
        ctx.udp_gather(self.frames_ptr(), stride, frame_off, self.n if n is None else n, self.d_rec, *self._outs(),
                       stream if stream is not None else self.torch.cuda.current_stream())
        return self

    def gather_indexed(self, ctx, offsets, eth_mod16, avail, stream=None):
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        if self.d_idx is None:
            self.d_idx = self.put(self.offsets.view(np.int64).copy())
        self.eth_of, self.avail = ug.indexed(self.offsets, eth_mod16), avail
        ctx.udp_gather_indexed(self.frames_ptr(), self.d_idx, eth_mod16, self.n, avail, self.d_rec, *self._outs(),
                               stream if stream is not None else self.torch.cuda.current_stream())
        return self

    def host_records(self):
        self.torch.cuda.synchronize()
        return self.d_rec.cpu().numpy()[:self.n * 16].view(pa.UDP_RESULT_DTYPE).copy()

    def outputs(self):
        """(payload buffer with its guards, offs, lens, subs, src or None, the three totals), as they are now."""
        self.torch.cuda.synchronize()
        h = lambda t, dt: t.cpu().numpy().view(dt).copy()  # noqa: E731
        return (h(self.d_pay, np.uint8), h(self.d_offs, np.uint64), h(self.d_lens, np.uint16), h(self.d_subs, np.uint32),
                None if self.d_src is None else h(self.d_src, np.uint32), h(self.d_total, ug.UDP_GATHER_TOTAL_DTYPE))

    def expected(self):
        rec = self.host_records()
        e = lambda a: None if a is None else a[GE:GE + self.n]  # noqa: E731
        pay, offs, lens, subs, src, total = ug.udp_gather_np(self.buf, self.eth_of, self.avail, rec, self.cap,
                                                             self.pay0[G:], e(self.offs0), e(self.lens0), e(self.subs0),
                                                             e(self.src0))

        def around(a0, mid):
            if a0 is None:
                return None
            out = a0.copy()
            out[GE:GE + self.n] = mid
            return out

        tot = TOTAL0.copy()
        tot[1] = total[0]
        return (np.concatenate([self.pay0[:G], pay]), around(self.offs0, offs), around(self.lens0, lens),
                around(self.subs0, subs), around(self.src0, src), tot)

    def check(self):
        """Every output, guards included, against the model applied to the canaries; the frames and the records
        unchanged.  Returns the total."""
        got, exp = self.outputs(), self.expected()
        for name, g, e in zip(("payloads", "pay_offs", "pay_lens", "sub_ids", "src_index", "total"), got, exp):
            if e is None:
                assert g is None
                continue
            bad = np.flatnonzero(g != e)
            assert bad.size == 0, "%s differs at %d (of %d): got %s want %s; %d differ; total got %s want %s" % (
                name, bad[0], len(g), g[bad[0]], e[bad[0]], bad.size, got[5][1], exp[5][1])
        frames_now = self.d_buf.cpu().numpy()
        assert np.array_equal(frames_now[G:G + len(self.buf)], self.buf), "a frame byte was written"
        if self.rec is not None:
            assert np.array_equal(self.host_records(), self.rec), "a record was written"
        return exp[5][1]
