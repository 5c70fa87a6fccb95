"""The device side of the demux tests (test-only helper, shared by tests/test_gpu_udp_demux.py and
tests/test_gpu_udp_demux_indexed.py): tests/udp_gather_dev.py's buffers plus the two per-subscription arrays, each a
non-constant canary with guard entries on both sides, and the comparison of every output, whole, against
tests/udp_demux_np.py."""
import numpy as np

import udp_demux_np as ud
import udp_gather_np as ug
from udp_gather_dev import G, GE, TOTAL0, Gather, canary  # noqa: F401

NAMES = ("payloads", "pay_offs", "pay_lens", "sub_ids", "src_index", "sub_first", "sub_bytes", "total")


class Demux(Gather):
    """Gather's arguments and n_subs.  fast: compare against the vectorised model (pinned to the loops by
    tests/test_udp_demux_np.py) -- for batches above 64 Ki frames."""

    def __init__(self, buf, n, cap, n_subs, fast=False, **kw):
        super().__init__(buf, n, cap, **kw)
        self.n_subs, self.fast = n_subs, fast
        rng = np.random.default_rng(n_subs + 77)
        self.first0 = rng.integers(1 << 28, 1 << 32, n_subs + 1 + 2 * GE).astype(np.uint32)
        self.bytes0 = rng.integers(1 << 50, 1 << 62, n_subs + 1 + 2 * GE).astype(np.uint64)
        self.d_first = self.put(self.first0.copy().view(np.int32))
        self.d_sbytes = self.put(self.bytes0.copy().view(np.int64))

    def _douts(self):
        o = self._outs()
        return o[:6] + (self.d_first.data_ptr() + 4 * GE, self.d_sbytes.data_ptr() + 8 * GE, o[6])

    def demux(self, ctx, stride, frame_off, stream=None, n=None):
        self.eth_of, self.avail = ug.strided(stride, frame_off), stride - frame_off
        self.eth_index = np.arange(self.n, dtype=np.int64) * stride + frame_off
        ctx.udp_demux(self.frames_ptr(), stride, frame_off, self.n if n is None else n, self.d_rec, self.n_subs,
                      *self._douts(), stream if stream is not None else self.torch.cuda.current_stream())
        return self

    def demux_indexed(self, ctx, offsets, eth_mod16, avail, stream=None):
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        if self.d_idx is None:
            self.d_idx = self.put(self.offsets.view(np.int64).copy())
        self.eth_of, self.avail = ug.indexed(self.offsets, eth_mod16), avail
        self.eth_index = np.where(self.offsets % 16 == eth_mod16, self.offsets.astype(np.int64), -1)
        ctx.udp_demux_indexed(self.frames_ptr(), self.d_idx, eth_mod16, self.n, avail, self.d_rec, self.n_subs,
                              *self._douts(), stream if stream is not None else self.torch.cuda.current_stream())
        return self

    def outputs(self):
        """(payload buffer with its guards, offs, lens, subs, src or None, sub_first, sub_bytes, the three totals)."""
        o = super().outputs()
        h = lambda t, dt: t.cpu().numpy().view(dt).copy()  # noqa: E731
        return o[:5] + (h(self.d_first, np.uint32), h(self.d_sbytes, np.uint64), o[5])

    def expected(self):
        rec = self.host_records()
        e = lambda a: None if a is None else a[GE:GE + self.n]  # noqa: E731
        args = (self.avail, rec, self.n_subs, self.cap, self.pay0[G:], e(self.offs0), e(self.lens0), e(self.subs0),
                e(self.src0), self.first0[GE:], self.bytes0[GE:])
        if self.fast:
            out = ud.udp_demux_fast_np(self.buf, self.eth_index, *args)
        else:
            out = ud.udp_demux_np(self.buf, self.eth_of, *args)
        pay, offs, lens, subs, src, first, sbytes, total = out

        def around(a0, mid):
            if a0 is None:
                return None
            x = a0.copy()
            x[GE:GE + len(mid)] = mid
            return x

        tot = TOTAL0.copy()
        tot[1] = total[0]
        return (np.concatenate([self.pay0[:G], pay]), around(self.offs0, offs), around(self.lens0, lens),
                around(self.subs0, subs), around(self.src0, src), around(self.first0, first), around(self.bytes0, sbytes),
                tot)

    def check(self):
        """Every output, guards included, against the model applied to the canaries; the frames and the records
        unchanged.  Returns the total."""
        got, exp = self.outputs(), self.expected()
        for name, g, e in zip(NAMES, got, exp):
            if e is None:
                assert g is None
                continue
            bad = np.flatnonzero(g != e)
            assert bad.size == 0, "%s differs at %d (of %d): got %s want %s; %d differ; total got %s want %s" % (
                name, bad[0], len(g), g[bad[0]], e[bad[0]], bad.size, got[7][1], exp[7][1])
        frames_now = self.d_buf.cpu().numpy()
        assert np.array_equal(frames_now[G:G + len(self.buf)], self.buf), "a frame byte was written"
        if self.rec is not None:
            assert np.array_equal(self.host_records(), self.rec), "a record was written"
        return exp[7][1]
