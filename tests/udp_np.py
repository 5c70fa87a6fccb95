"""numpy / plain-byte restatement of pn_udp_classify's record (include/pollnet_amd.h, PN_UF_*) and an
Ethernet / IPv4 / UDP frame builder with every field overridable (test-only).  Written from the flag table,
byte by byte in network order: nothing here shares code or word order with the kernel, which sums the words
as a little-endian machine loads them.  tests/test_udp_np.py pins the sums to the oracle's CSum and to
hand-computed datagrams before any GPU test trusts them."""
import numpy as np

UDP_SUB_DTYPE = np.dtype([("dst_ip", "<u4"), ("dst_port", "<u2"), ("_pad", "<u2")])
UDP_RESULT_DTYPE = np.dtype([("sub_id", "<u4"), ("src_ip", "<u4"), ("src_port", "<u2"), ("payload_off", "<u2"),
                             ("payload_len", "<u2"), ("flags", "<u2")])
NO_SUB = 0xFFFFFFFF
IP_OK, UDP_OK, MATCH, NOCSUM, FRAG, LEN_BAD = 0x0001, 0x0002, 0x0004, 0x0008, 0x0010, 0x0020
IHL_NE_5, NOT_UDP, TRUNC, UDP_UNCHECKED = 0x0200, 0x1000, 0x2000, 0x8000
ALL_FLAGS = (IP_OK, UDP_OK, MATCH, NOCSUM, FRAG, LEN_BAD, IHL_NE_5, NOT_UDP, TRUNC, UDP_UNCHECKED)


def ip4(s):
    """'239.1.2.3' -> its 4 bytes in network order."""
    return bytes(int(x) for x in s.split("."))


def stored_u32(b4):
    """4 network-order bytes -> the u32 a little-endian load of them gives (pn_udp_sub.dst_ip, pn_udp_result.src_ip)."""
    return int.from_bytes(bytes(b4), "little")


def stored_u16(port):
    """A host-order port -> the u16 a little-endian load of its network-order bytes gives."""
    return int.from_bytes(int(port).to_bytes(2, "big"), "little")


def make_subs(pairs):
    """[(ip bytes, host-order port)] -> a UDP_SUB_DTYPE array."""
    s = np.zeros(len(pairs), UDP_SUB_DTYPE)
    for i, (ip, port) in enumerate(pairs):
        s[i] = (stored_u32(ip), stored_u16(port), 0)
    return s


def ones_sum(data):
    """RFC 1071: the 16-bit one's-complement sum of `data` as big-endian words, an odd tail padded with a zero
    byte, folded to 16 bits."""
    data = bytes(data)
    if len(data) & 1:
        data += b"\0"
    s = int(np.frombuffer(data, ">u2").sum(dtype=np.uint64)) if data else 0
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def udp_checksum(src_ip, dst_ip, udp_hdr_and_payload, ulen):
    """The RFC 768 checksum field for a datagram whose own checksum bytes are zero: the complement of the sum over
    the pseudo-header (src, dst, 0, 17, ulen) and the first ulen bytes of the datagram; 0 is sent as 0xFFFF."""
    pseudo = bytes(src_ip) + bytes(dst_ip) + bytes([0, 17]) + int(ulen).to_bytes(2, "big")
    c = (~ones_sum(pseudo + bytes(udp_hdr_and_payload[:ulen]))) & 0xFFFF
    return c if c else 0xFFFF


def put_udp_frame(slot, frame_off, payload, src_ip, dst_ip, src_port, dst_port, *, ether_type=0x0800, ver_ihl=0x45,
                  proto=17, frag_off=0, tot_len=None, ulen=None, udp_csum="valid", ip_csum="valid", ttl=64, ip_id=0,
                  force_ffff=False):
    """Write one Ethernet / IPv4 / UDP frame at slot[frame_off:], as much of it as the slot holds.
    tot_len / ulen default to the true lengths; udp_csum: "valid" (computed over the declared ulen and the bytes
    actually present, zero beyond them) or the 16-bit field value; ip_csum likewise.  force_ffff: the first two
    payload bytes are replaced so that the datagram sums to 0xFFFF before the checksum: its checksum computes
    to 0 and is transmitted as 0xFFFF.  Returns the payload as written."""
    payload = bytearray(payload)
    true_ulen = 8 + len(payload)
    ulen = true_ulen if ulen is None else ulen
    tot_len = 20 + true_ulen if tot_len is None else tot_len
    ip = bytearray(20)
    ip[0] = ver_ihl
    ip[2:4] = int(tot_len & 0xFFFF).to_bytes(2, "big")
    ip[4:6] = int(ip_id).to_bytes(2, "big")
    ip[6:8] = int(frag_off).to_bytes(2, "big")
    ip[8] = ttl
    ip[9] = proto
    ip[12:16] = bytes(src_ip)
    ip[16:20] = bytes(dst_ip)
    if ip_csum == "valid":
        ip[10:12] = ((~ones_sum(ip)) & 0xFFFF).to_bytes(2, "big")
    else:
        ip[10:12] = int(ip_csum).to_bytes(2, "big")
    udp = bytearray(8)
    udp[0:2] = int(src_port).to_bytes(2, "big")
    udp[2:4] = int(dst_port).to_bytes(2, "big")
    udp[4:6] = int(ulen & 0xFFFF).to_bytes(2, "big")
    room = len(slot) - frame_off - 42
    body = bytes(payload[:max(room, 0)])
    if force_ffff:
        assert len(body) >= 2 and ulen >= 10
        # the complement of everything else's sum R: R + (0xFFFF - R) = 0xFFFF (and R = 0xFFFF gives 0xFFFF + 0xFFFF,
        # which folds to 0xFFFF as well)
        rest = udp_checksum(src_ip, dst_ip, bytes(udp) + b"\0\0" + body[2:], ulen)
        body = int(rest).to_bytes(2, "big") + body[2:]
        payload[0:2] = body[0:2]
    if udp_csum == "valid":
        dgram = (bytes(udp) + body).ljust(max(ulen, 8), b"\0")
        udp[6:8] = udp_checksum(src_ip, dst_ip, dgram, max(ulen, 0)).to_bytes(2, "big")
    else:
        udp[6:8] = int(udp_csum).to_bytes(2, "big")
    eth = bytes(6) + bytes([2, 0, 0, 0, 0, 1]) + int(ether_type).to_bytes(2, "big")
    frame = eth + bytes(ip) + bytes(udp) + body
    w = min(len(frame), len(slot) - frame_off)
    slot[frame_off:frame_off + w] = np.frombuffer(frame[:w], np.uint8)
    return bytes(payload)


def udp_classify_np(slots, stride, frame_off, subs, verify=True):
    """The records pn_udp_classify must write for n = len(slots) // stride slots, straight from the flag table."""
    flat = np.ascontiguousarray(slots, dtype=np.uint8).reshape(-1)
    n = len(flat) // stride
    avail = stride - frame_off
    table = {}
    for i, s in enumerate(subs):
        table[(int(s["dst_ip"]), int(s["dst_port"]))] = i
    out = np.zeros(n, UDP_RESULT_DTYPE)
    for i in range(n):
        eth = bytes(flat[i * stride + frame_off:(i + 1) * stride])
        ip = eth[14:]
        ether_type = (eth[12] << 8) | eth[13]
        version, ihl = ip[0] >> 4, ip[0] & 0xF
        tot_len = (ip[2] << 8) | ip[3]
        frag = (ip[6] << 8) | ip[7]
        proto = ip[9]
        ulen = (eth[38] << 8) | eth[39]
        csum_field = (eth[40] << 8) | eth[41]
        flags = 0
        if ones_sum(ip[:20]) == 0xFFFF:
            flags |= IP_OK
        if ether_type != 0x0800 or version != 4 or proto != 17:
            flags |= NOT_UDP
        if ihl != 5:
            flags |= IHL_NE_5
        if frag & 0x3FFF:
            flags |= FRAG
        if ulen < 8 or tot_len < 28 or ulen > tot_len - 20:
            flags |= LEN_BAD
        if 34 + ((ulen + 1) & ~1) > avail:
            flags |= TRUNC
        sub = NO_SUB
        if not flags & (NOT_UDP | IHL_NE_5 | FRAG):
            key = (int.from_bytes(eth[30:34], "little"), int.from_bytes(eth[36:38], "little"))
            if key in table:
                sub = table[key]
                flags |= MATCH
        if (flags & MATCH) and not flags & (LEN_BAD | TRUNC):  # checkable
            if csum_field == 0:
                flags |= NOCSUM
            elif not verify:
                flags |= UDP_UNCHECKED
            else:
                pseudo = eth[26:34] + bytes([0, 17]) + eth[38:40]
                if ones_sum(pseudo + eth[34:34 + ulen]) == 0xFFFF:
                    flags |= UDP_OK
        out[i] = (sub, int.from_bytes(eth[26:30], "little"), int.from_bytes(eth[34:36], "little"), 42,
                  (ulen - 8) & 0xFFFF, flags)
    return out


def deliver(flags):
    """PN_UDP_DELIVER over an array of flags."""
    f = np.asarray(flags)
    return ((f & MATCH) != 0) & ((f & IP_OK) != 0) & ((f & (UDP_OK | NOCSUM | UDP_UNCHECKED)) != 0)
