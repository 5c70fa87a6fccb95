"""Pins tests/udp_np.py (the expected records of pn_udp_classify, written from the flag table) before any GPU test
trusts it: its sums against the oracle's CSum, Efvi's own UDP frames, three datagrams computed by hand."""
import os
import re
import subprocess

import numpy as np

import pollnet_amd as pa
from oracle import pyoracle as orc

import udp_np as un

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC, DST = un.ip4("10.0.0.1"), un.ip4("10.0.0.2")
SPORT, DPORT = 1000, 2000  # 0x03E8, 0x07D0


def _bswap16(v):
    return ((v & 0xFF) << 8) | (v >> 8)


def test_sums_equal_the_oracle_csum():
    """CSum (Core.h:89-138, pinned to the reference's own by test_ref_core) adds the words as a little-endian
    machine loads them and fold() complements: the byte-swapped complement of the big-endian sum here."""
    rng = np.random.default_rng(7)
    for n in (0, 2, 4, 20, 64, 1472, 1480, 65534):
        data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        c = orc.Csum()
        c.add_bytes(data)
        assert c.fold() == _bswap16((~un.ones_sum(data)) & 0xFFFF), n
    for data in (b"\xff" * 64, b"\x00" * 64, b"\xff\xff" + b"\x00" * 30):
        c = orc.Csum()
        c.add_bytes(data)
        assert c.fold() == _bswap16((~un.ones_sum(data)) & 0xFFFF)


def test_flag_values_equal_the_header():
    hdr = open(os.path.join(ROOT, "include", "pollnet_amd.h")).read()
    for name in ("IP_OK", "UDP_OK", "MATCH", "NOCSUM", "FRAG", "LEN_BAD", "IHL_NE_5", "NOT_UDP", "TRUNC", "UDP_UNCHECKED"):
        v = int(re.search(r"#define PN_UF_%s (0x[0-9A-Fa-f]+)u" % name, hdr).group(1), 16)
        assert v == getattr(un, name) == getattr(pa.UF, name), name
    assert int(re.search(r"#define PN_UDP_MAX_SUBS (\d+)u", hdr).group(1)) == pa.PN_UDP_MAX_SUBS == 4096
    assert pa.PN_UDP_NO_SUB == un.NO_SUB == 0xFFFFFFFF
    assert pa.UDP_RESULT_DTYPE == un.UDP_RESULT_DTYPE and pa.UDP_SUB_DTYPE == un.UDP_SUB_DTYPE
    assert [pa.UDP_RESULT_DTYPE.fields[k][1] for k in ("sub_id", "src_ip", "src_port", "payload_off", "payload_len", "flags")] \
        == [0, 4, 8, 10, 12, 14]


def test_udp_symbols_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pollnet_amd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", pa.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ("pn_udp_set_subs", "pn_udp_classify"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name


def test_efvi_sender_frames_are_match_ipok_nocsum():
    """Efvi's UDP sender (update_udp_pkt, Efvi.h:611-621) sends checksum 0; with a verifying IPv4 header
    checksum (PN_TX_UDP's fill) its frames, subscribed to, are exactly MATCH | IP_OK | NOCSUM."""
    n, stride, frame_off = 300, 2048, 14
    slots, lens, _ = orc.tx_build_batch(11, n, stride, frame_off, mode=orc.TX_UDP_EFVI)
    orc.tx_fill_batch(slots, stride, frame_off, n, lens, mode=orc.TX_UDP)
    keys = {}
    for i in range(n):
        eth = slots[i, frame_off:]
        keys.setdefault((bytes(eth[30:34]), int.from_bytes(bytes(eth[36:38]), "big")), len(keys))
    subs = un.make_subs(list(keys))
    rec = un.udp_classify_np(slots, stride, frame_off, subs)
    assert (rec["flags"] == (un.MATCH | un.IP_OK | un.NOCSUM)).all(), np.unique(rec["flags"])
    assert np.array_equal(rec["payload_len"], lens)
    assert (rec["payload_off"] == 42).all() and un.deliver(rec["flags"]).all()
    for i in range(n):
        eth = slots[i, frame_off:]
        assert rec["sub_id"][i] == keys[(bytes(eth[30:34]), int.from_bytes(bytes(eth[36:38]), "big"))]
    # nobody subscribed: no MATCH, and then no checksum verdict either
    other = un.make_subs([(un.ip4("1.2.3.4"), 5)])
    rec = un.udp_classify_np(slots, stride, frame_off, other)
    assert (rec["flags"] == un.IP_OK).all() and (rec["sub_id"] == un.NO_SUB).all()


def _one(payload, csum, after=b"", **kw):
    slot = np.zeros(128, np.uint8)
    un.put_udp_frame(slot, 2, payload, SRC, DST, SPORT, DPORT, udp_csum=csum, **kw)
    if after:
        o = 2 + 42 + len(payload)
        slot[o:o + len(after)] = np.frombuffer(after, np.uint8)
    rec = un.udp_classify_np(slot, 128, 2, un.make_subs([(DST, DPORT)]))[0]
    return slot, rec


def test_hand_computed_even_length():
    # pseudo-header: 0A00 + 0001 + 0A00 + 0002 + 0011 + 000C (ulen 12)            = 1420
    # UDP header:    03E8 + 07D0 + 000C + 0000 (checksum field)                   = 0BC4
    # payload "ABCD": 4142 + 4344                                                 = 8486
    # 1420 + 0BC4 = 1FE4 ; 1FE4 + 8486 = A46A ; checksum = ~A46A                  = 5B95
    assert un.ones_sum(SRC + DST + b"\0\x11\0\x0c") == 0x1420
    assert un.udp_checksum(SRC, DST, bytes.fromhex("03e807d0000c0000") + b"ABCD", 12) == 0x5B95
    slot, rec = _one(b"ABCD", 0x5B95)
    assert rec["flags"] == un.MATCH | un.IP_OK | un.UDP_OK and rec["payload_len"] == 4 and rec["sub_id"] == 0
    assert rec["src_ip"] == 0x0100000A and rec["src_port"] == 0xE803  # as stored
    assert bytes(slot[2 + 40:2 + 42]) == b"\x5b\x95"
    _, rec = _one(b"ABCD", 0x5B96)
    assert rec["flags"] == un.MATCH | un.IP_OK
    _, rec = _one(b"ABCD", "valid")
    assert rec["flags"] == un.MATCH | un.IP_OK | un.UDP_OK


def test_hand_computed_odd_length_ignores_the_byte_after():
    # pseudo-header: 0A00 + 0001 + 0A00 + 0002 + 0011 + 000B (ulen 11)            = 141F
    # UDP header:    03E8 + 07D0 + 000B + 0000                                    = 0BC3
    # payload "ABC" zero-padded: 4142 + 4300                                      = 8442
    # 141F + 0BC3 = 1FE2 ; 1FE2 + 8442 = A424 ; checksum = ~A424                  = 5BDB
    # (with the byte after, EE, summed as 43EE the sum would be A512: it must not be)
    for after in (b"\xee\x11", b"\x00\x00", b"\xff\xff"):
        _, rec = _one(b"ABC", 0x5BDB, after=after)
        assert rec["flags"] == un.MATCH | un.IP_OK | un.UDP_OK and rec["payload_len"] == 3, after
    _, rec = _one(b"ABC", (~0xA512) & 0xFFFF, after=b"\xee")
    assert rec["flags"] == un.MATCH | un.IP_OK


def test_hand_computed_checksum_sent_as_ffff():
    # pseudo-header 1420 + UDP header 0BC4 = 1FE4 (as the even case); payload E000 + 001B = E01B
    # 1FE4 + E01B = FFFF ; checksum = ~FFFF = 0000, which RFC 768 sends as FFFF
    # the receiver's sum: FFFF + FFFF = 1FFFE -> FFFF: valid
    payload = bytes.fromhex("e000001b")
    assert un.udp_checksum(SRC, DST, bytes.fromhex("03e807d0000c0000") + payload, 12) == 0xFFFF
    slot, rec = _one(payload, 0xFFFF)
    assert rec["flags"] == un.MATCH | un.IP_OK | un.UDP_OK
    # the same datagram with the field 0 is "no checksum", not a verified one
    _, rec = _one(payload, 0)
    assert rec["flags"] == un.MATCH | un.IP_OK | un.NOCSUM
    # the builder's own route to such a datagram
    slot2 = np.zeros(128, np.uint8)
    un.put_udp_frame(slot2, 2, b"\0\0\x00\x1b", SRC, DST, SPORT, DPORT, force_ffff=True)
    assert np.array_equal(slot, slot2)


def test_release_path_and_unsubscribed():
    slot, _ = _one(b"ABCD", 0x5B95)
    subs = un.make_subs([(DST, DPORT)])
    assert un.udp_classify_np(slot, 128, 2, subs, verify=False)[0]["flags"] == un.MATCH | un.IP_OK | un.UDP_UNCHECKED
    for ip, port in ((DST, DPORT + 1), (DST, DPORT - 1), (un.ip4("10.0.0.3"), DPORT), (un.ip4("10.0.0.1"), DPORT)):
        rec = un.udp_classify_np(slot, 128, 2, un.make_subs([(ip, port)]))[0]
        assert rec["flags"] == un.IP_OK and rec["sub_id"] == un.NO_SUB
