"""numpy / plain-byte statement of pn_udp_build (include/pollnet_amd.h): the ring a build must leave and its
frame_lens (test-only).  Written from the header's contract byte by byte: start from the ring as it was and, for
each accepted message, copy the channel's template, set tot_len and udp_len, compute the checksums, copy the
payload.  Nothing here shares code with the kernel.  tests/test_udp_build_np.py pins it to the reference's own
update_udp_pkt and to the receive side's model (tests/udp_np.py) before any GPU test trusts it."""
import numpy as np

UDP_CHANNEL_DTYPE = np.dtype([("hdr", "u1", (42,)), ("_pad", "u1", (6,))])
UB_EFVI, UB_PLAIN, UB_CSUM = 0, 1, 2
HDR = 42


def make_template(src_mac, dst_mac, src_ip, dst_ip, src_port, dst_port):
    """EfviUdpSender::init_udp_pkt's 42 bytes (Efvi.h:597-644): IHL 5, tos 0, tot_len 0, id 0, DF, ttl 64,
    protocol 17, checksum 0; udp_len 8, udp checksum 0.  Addresses as 4 network-order bytes, ports host order."""
    h = bytearray(HDR)
    h[0:6], h[6:12] = bytes(dst_mac), bytes(src_mac)
    h[12:14] = b"\x08\x00"
    h[14] = 0x45
    h[20:22] = b"\x40\x00"  # ip_frag_off_be16 = 0x0040 as stored: DF
    h[22], h[23] = 64, 17
    h[26:30], h[30:34] = bytes(src_ip), bytes(dst_ip)
    h[34:36] = int(src_port).to_bytes(2, "big")
    h[36:38] = int(dst_port).to_bytes(2, "big")
    h[38:40] = (8).to_bytes(2, "big")
    return bytes(h)


def make_channels(templates):
    c = np.zeros(len(templates), UDP_CHANNEL_DTYPE)
    for i, t in enumerate(templates):
        c["hdr"][i] = np.frombuffer(bytes(t), np.uint8)
    return c


def _ones_sum_be(data):
    """RFC 1071 over big-endian words, an odd tail zero-padded, folded to 16 bits."""
    data = bytes(data)
    if len(data) & 1:
        data += b"\0"
    b = np.frombuffer(data, np.uint8).astype(np.uint64)
    s = int((b[0::2] * 256 + b[1::2]).sum()) if len(data) else 0
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def efvi_ip_check(ip20, paylen):
    """Efvi's IPv4 checksum field as the two bytes it stores (Efvi.h:405-411, 615-619): the header's ten u16 as an
    x86 loads them, with tot_len = check = 0, folded once, then `cache += cache >> 16` (the carry stays in);
    ipsum = cache + htons(28 + paylen); ipsum += ipsum >> 16; check = ~ipsum."""
    ip = bytearray(ip20)
    ip[2:4] = b"\0\0"
    ip[10:12] = b"\0\0"
    cache = sum(ip[i] | (ip[i + 1] << 8) for i in range(0, 20, 2))
    cache = (cache >> 16) + (cache & 0xFFFF)
    cache += cache >> 16
    tot = 28 + paylen
    iplen = ((tot & 0xFF) << 8) | (tot >> 8)  # htons on x86
    ipsum = cache + iplen
    ipsum += ipsum >> 16
    chk = ~ipsum & 0xFFFF
    return bytes([chk & 0xFF, chk >> 8])  # a u16 store on x86


def build_frame(template, payload, mode):
    """The 42 + len bytes of one built frame."""
    n = len(payload)
    f = bytearray(template[:HDR]) + bytearray(payload)
    f[16:18] = (28 + n).to_bytes(2, "big")
    f[38:40] = (8 + n).to_bytes(2, "big")
    f[24:26] = b"\0\0"
    f[40:42] = b"\0\0"
    if mode == UB_EFVI:
        f[24:26] = efvi_ip_check(f[14:34], n)
    else:
        f[24:26] = ((~_ones_sum_be(f[14:34])) & 0xFFFF).to_bytes(2, "big")
    if mode == UB_CSUM:
        pseudo = bytes(f[26:34]) + bytes([0, 17]) + (8 + n).to_bytes(2, "big")
        c = (~_ones_sum_be(pseudo + bytes(f[34:]))) & 0xFFFF
        f[40:42] = (c if c else 0xFFFF).to_bytes(2, "big")
    return bytes(f)


def refused(length, chan, off, stride, frame_off, n_chans, payload_bytes):
    """The header's refusal rules, in its order."""
    return (HDR + length > stride - frame_off or HDR + length > 65535 or 28 + length > 65535 or chan >= n_chans
            or off > payload_bytes or length > payload_bytes - off)


def udp_build_np(ring, stride, frame_off, chans, payloads, payload_bytes, pay_offs, pay_lens, chan_ids, mode,
                 first_slot_at=0):
    """(ring after the build, frame_lens).  ring: flat u8, slot i at first_slot_at + i * stride (bytes before and
    after the n slots are guards and stay).  payloads: the buffer's bytes; chan_ids None = channel 0."""
    out = np.array(ring, dtype=np.uint8).reshape(-1).copy()
    pay = bytes(np.asarray(payloads, dtype=np.uint8).reshape(-1))
    n = len(pay_lens)
    frame_lens = np.zeros(n, np.uint16)
    hdrs = [bytes(chans["hdr"][i]) for i in range(len(chans))]
    for i in range(n):
        length, off = int(pay_lens[i]), int(pay_offs[i])
        ch = 0 if chan_ids is None else int(chan_ids[i])
        if refused(length, ch, off, stride, frame_off, len(hdrs), payload_bytes):
            continue
        f = build_frame(hdrs[ch], pay[off:off + length], mode)
        assert len(f) == HDR + length
        at = first_slot_at + i * stride + frame_off
        out[at:at + len(f)] = np.frombuffer(f, np.uint8)
        frame_lens[i] = HDR + length
    return out, frame_lens
