"""numpy / plain-loop statement of pn_udp_gather and pn_udp_gather_indexed (include/pollnet_amd.h): the payload
buffer, the four index arrays and the total a gather must leave (test-only).  Written from the header's contract
frame by frame: walk the records in order, take a frame when its record says so, append its payload at the next
multiple of 16, zero the pad.  Every output starts from the canary it is given, so what the model leaves untouched
is what the kernels must leave untouched.  Nothing here shares code with the kernels.
tests/test_udp_gather_np.py pins it by hand and against the build and classify models."""
import numpy as np

import udp_np as un

UDP_GATHER_TOTAL_DTYPE = np.dtype([("n_bytes", "<u8"), ("n_msgs", "<u4"), ("n_fit", "<u4")])
ALIGN = 16
HDR = 42


def pad16(n):
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def strided(stride, frame_off, first_slot_at=0):
    """eth_of for a strided ring: frame i's Ethernet header at first_slot_at + i * stride + frame_off."""
    return lambda i: first_slot_at + i * stride + frame_off


def indexed(offsets, eth_mod16, base_at=0):
    """eth_of for an indexed call: base_at + offsets[i], None for an offset outside the call's class (not taken)."""
    return lambda i: base_at + int(offsets[i]) if int(offsets[i]) % 16 == eth_mod16 else None


def taken(rec, avail):
    """The header's rule for one record."""
    return bool(un.deliver(int(rec["flags"]))) and int(rec["payload_off"]) == HDR and HDR + int(rec["payload_len"]) <= avail


def udp_gather_np(buf, eth_of, avail, records, payload_cap, payloads0, offs0, lens0, subs0, src0=None):
    """(payloads, pay_offs, pay_lens, sub_ids, src_index or None, total) after a gather of len(records) frames.
    buf: the bytes the frames lie in; eth_of(i): where frame i's Ethernet header starts in buf (None: an indexed
    offset outside the class).  payloads0 is the whole payload buffer as it was (its first payload_cap bytes are the
    call's; the rest are guards), offs0 .. src0 the arrays as they were."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    pay = np.array(payloads0, dtype=np.uint8).copy()
    offs, lens, subs = np.array(offs0, np.uint64), np.array(lens0, np.uint16), np.array(subs0, np.uint32)
    src = None if src0 is None else np.array(src0, np.uint32)
    at, j, n_fit = 0, 0, 0
    for i in range(len(records)):
        r = records[i]
        eth = eth_of(i)
        if eth is None or not taken(r, avail):
            continue
        ln = int(r["payload_len"])
        offs[j], lens[j], subs[j] = at, ln, int(r["sub_id"])
        if src is not None:
            src[j] = i
        end = at + pad16(ln)
        if end <= payload_cap:
            assert n_fit == j, "the copied messages are a prefix"
            pay[at:at + ln] = buf[eth + HDR:eth + HDR + ln]
            pay[at + ln:end] = 0
            n_fit += 1
        at = end
        j += 1
    total = np.zeros(1, UDP_GATHER_TOTAL_DTYPE)
    total[0] = (at, j, n_fit)
    return pay, offs, lens, subs, src, total
