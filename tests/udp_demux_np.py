"""Plain-loop statement of pn_udp_demux and pn_udp_demux_indexed (include/pollnet_amd.h): the payload buffer, the
four per-message arrays, the two per-subscription arrays and the total a demux must leave (test-only).  Written from
the header's contract: walk the records in order, append each taken frame to its subscription's list, concatenate
the lists, lay the bytes out.  Every output starts from the canary it is given, so what the model leaves untouched is
what the kernels must leave untouched.  Nothing here shares code with the kernels.
udp_demux_fast_np is a vectorised restatement (a stable argsort) for the large GPU cases;
tests/test_udp_demux_np.py pins both, the second against the first."""
import numpy as np

import udp_gather_np as ug
import udp_np as un

HDR = 42


def taken(rec, avail, n_subs):
    """The header's rule for one record: the gather's, and a sub_id below n_subs."""
    return ug.taken(rec, avail) and int(rec["sub_id"]) < n_subs


def udp_demux_np(buf, eth_of, avail, records, n_subs, payload_cap, payloads0, offs0, lens0, subs0, src0, first0,
                 bytes0):
    """(payloads, pay_offs, pay_lens, sub_ids, src_index or None, sub_first, sub_bytes, total) after a demux of
    len(records) frames.  buf / eth_of / payloads0 / offs0 .. src0 as in udp_gather_np; first0 and bytes0 are the
    per-subscription arrays as they were (at least n_subs + 1 entries)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    pay = np.array(payloads0, dtype=np.uint8).copy()
    offs, lens, subs = np.array(offs0, np.uint64), np.array(lens0, np.uint16), np.array(subs0, np.uint32)
    src = None if src0 is None else np.array(src0, np.uint32)
    first, sbytes = np.array(first0, np.uint32), np.array(bytes0, np.uint64)
    lists = [[] for _ in range(n_subs)]
    for i in range(len(records)):
        if eth_of(i) is None or not taken(records[i], avail, n_subs):
            continue
        lists[int(records[i]["sub_id"])].append(i)
    at, j, n_fit = 0, 0, 0
    for s in range(n_subs):
        first[s], sbytes[s] = j, at
        for i in lists[s]:
            ln = int(records[i]["payload_len"])
            offs[j], lens[j], subs[j] = at, ln, s
            if src is not None:
                src[j] = i
            end = at + ug.pad16(ln)
            if end <= payload_cap:
                assert n_fit == j, "the copied messages are a prefix"
                eth = eth_of(i)
                pay[at:at + ln] = buf[eth + HDR:eth + HDR + ln]
                pay[at + ln:end] = 0
                n_fit += 1
            at = end
            j += 1
    first[n_subs], sbytes[n_subs] = j, at
    total = np.zeros(1, ug.UDP_GATHER_TOTAL_DTYPE)
    total[0] = (at, j, n_fit)
    return pay, offs, lens, subs, src, first, sbytes, total


def udp_demux_fast_np(buf, eth_index, avail, records, n_subs, payload_cap, payloads0, offs0, lens0, subs0, src0, first0,
                      bytes0):
    """The same outputs by a stable argsort, for batches too large for the loops.  eth_index: a u64 array, frame i's
    Ethernet header in buf, or -1 (as int64) for an indexed offset outside the class."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    pay = np.array(payloads0, dtype=np.uint8).copy()
    offs, lens, subs = np.array(offs0, np.uint64), np.array(lens0, np.uint16), np.array(subs0, np.uint32)
    src = None if src0 is None else np.array(src0, np.uint32)
    first, sbytes = np.array(first0, np.uint32), np.array(bytes0, np.uint64)
    eth = np.asarray(eth_index).astype(np.int64)
    rec = records
    tk = (un.deliver(rec["flags"]).astype(bool) & (rec["payload_off"] == HDR) &
          (HDR + rec["payload_len"].astype(np.int64) <= avail) & (rec["sub_id"] < n_subs) & (eth >= 0))
    idx = np.flatnonzero(tk)
    idx = idx[np.argsort(rec["sub_id"][idx], kind="stable")]
    m = len(idx)
    ln = rec["payload_len"][idx].astype(np.int64)
    pad = (ln + 15) // 16 * 16
    end = np.cumsum(pad)
    at = end - pad
    offs[:m], lens[:m], subs[:m] = at, ln, rec["sub_id"][idx]
    if src is not None:
        src[:m] = idx
    n_bytes = int(end[-1]) if m else 0
    fits = end <= payload_cap
    n_fit = m if fits.all() else int(np.argmin(fits))
    if n_fit:
        # the copied messages tile [0, end of the last one): zeros, then every message byte from its frame
        pay[:int(end[n_fit - 1])] = 0
        lf = ln[:n_fit]
        within = np.arange(int(lf.sum())) - np.repeat(np.cumsum(lf) - lf, lf)
        pay[np.repeat(at[:n_fit], lf) + within] = buf[np.repeat(eth[idx[:n_fit]] + HDR, lf) + within]
    first[:n_subs + 1] = np.searchsorted(rec["sub_id"][idx], np.arange(n_subs + 1), side="left")
    starts = np.concatenate([at, [n_bytes]]).astype(np.uint64)
    sbytes[:n_subs + 1] = starts[first[:n_subs + 1]]
    total = np.zeros(1, ug.UDP_GATHER_TOTAL_DTYPE)
    total[0] = (n_bytes, m, n_fit)
    return pay, offs, lens, subs, src, first, sbytes, total
