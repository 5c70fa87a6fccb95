"""The records pn_udp_classify_indexed must write, from tests/udp_np.py alone (test-only): frame i's bytes
base[offsets[i] : offsets[i] + avail] are gathered into slot i of a strided twin ring (frame_off = eth_mod16,
stride = eth_mod16 + avail rounded up to 16: a ring pn_udp_classify itself accepts), the twin goes through
udp_np.udp_classify_np, and the rows whose offset is outside the call's alignment class are overwritten with the
BADOFF record.  udp_classify_np is given the twin's first eth_mod16 + avail columns, so that the avail of its
TRUNC rule is the call's also where the rounding added bytes.  No new oracle: what a frame's record is stays
defined in one place."""
import numpy as np

import udp_np as un

BADOFF = 0x4000


def badoff_record():
    r = np.zeros(1, un.UDP_RESULT_DTYPE)
    r[0] = (un.NO_SUB, 0, 0, 0, 0, BADOFF)
    return r[0]


def twin_ring(base, offsets, eth_mod16, avail):
    """(twin slots [n, stride], stride, in_class mask).  Out-of-class rows stay zero: none of their bytes is read."""
    base = np.ascontiguousarray(base, dtype=np.uint8).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.uint64)
    stride = (eth_mod16 + avail + 15) & ~15
    in_class = (offsets % np.uint64(16)) == np.uint64(eth_mod16)
    twin = np.zeros((len(offsets), stride), np.uint8)
    for i in np.flatnonzero(in_class):
        o = int(offsets[i])
        assert o + avail <= len(base), "the buffer must extend avail bytes past every Ethernet header"
        twin[i, eth_mod16:eth_mod16 + avail] = base[o:o + avail]
    return twin, stride, in_class


def udp_classify_indexed_np(base, offsets, eth_mod16, avail, subs, verify=True):
    twin, stride, in_class = twin_ring(base, offsets, eth_mod16, avail)
    # the twin's TRUNC rule is the call's only if its avail is: stride - frame_off may exceed it by the rounding
    exp = un.udp_classify_np(twin[:, :eth_mod16 + avail], eth_mod16 + avail, eth_mod16, subs, verify)
    exp[~in_class] = badoff_record()
    return exp
