"""CPU: the inputs of tests/test_gpu_indexed_extent.py hold what those tests are about, judged from the oracle's
records (tests/indexed_np.py) -- so that the GPU comparisons cannot pass vacuously.  For every (eth_mod16, avail)
and every layout the GPU file launches: a verified segment whose summed extent ends inside the chunk avail ends
in, at the two window phases that start the stream latest; one whose extent is avail exactly; a truncated one;
one that fails its TCP checksum through a flipped payload byte while its IP header verifies."""
import numpy as np
import pytest

import indexed_np as ixn

CLASSES = [0, 2, 4, 6, 8, 10, 12, 14]
AVAILS = [96, 98, 100, 110, 111, 112, 124, 126, 128, 2046, 2048]
SEED_AVAILS = [98, 100, 126, 2046]
FILL_SEEDS = (11, 12)
SMALL_SLOTS = [(112, 2), (112, 16), (128, 2), (128, 10), (256, 34)]


def window_form_cases(eth_mod16, avail):
    """Every launch of test_window_forms for one parameter pair, by name."""
    return {"spaced": ixn.spaced(eth_mod16, avail, FILL_SEEDS[0]),
            "packed lead 0": ixn.packed(eth_mod16, avail, 0),
            "packed lead 1": ixn.packed(eth_mod16, avail, 1),
            "packed x16": ixn.packed(eth_mod16, avail, 0, 16, 3)}


def check_case(c, phases):
    g = ixn.Geometry(c.eth_mod16, c.avail)
    fl, ext = c.exp["flags"], c.extents
    ok = (fl & ixn.TCP_OK) != 0
    assert not (fl & (ixn.BADOFF | ixn.TCP_UNCHECKED)).any()
    # what the builder says of each frame is what the records say: payload_off + payload_len = 14 + min(tot_len, 1500)
    assert np.array_equal(c.exp["payload_off"].astype(np.int64) + c.exp["payload_len"], 14 + np.minimum(c.tot_len, 1500))
    assert np.array_equal((fl & ixn.TRUNC) != 0, ext > c.avail)
    assert not (ok & c.corrupt).any()
    if g.partial and g.in_window and g.reachable:
        inside = ok & (ext > g.cs) & (ext <= c.avail)
        assert inside.any(), "no verified segment ends in the chunk avail ends in"
        if phases:
            seen = set(c.win_phase[inside].tolist())
            assert {0, 16} <= seen, sorted(seen)
    if c.avail % 2 == 0:
        assert (ok & (ext == c.avail)).any(), "no verified segment ends at avail"
    assert (ok & (ext == (c.avail & ~1) - 2)).any()
    # an odd segment: the reference's sum takes in the byte after it (non-zero here), RFC 793's pads with zero
    rfc_ok = (fl & ixn.RFC_TCP_OK) != 0
    assert (rfc_ok & (c.tot_len % 2 == 1) & (ext == (c.avail & ~1))).any(), "no odd segment whose pad byte is the last word's"
    assert (fl & ixn.TRUNC).any()
    assert (c.corrupt & ((fl & (ixn.TCP_OK | ixn.IP_OK | ixn.TRUNC)) == ixn.IP_OK)).any()
    for bit in (ixn.HIT, ixn.TW):
        assert (fl & bit).any()
    assert ((fl & ixn.HIT) == 0).any() and (fl & ixn.IHL_NE_5).any()
    end_rel = ext[ok] - 14 + g.mis  # as the stream sees it
    assert (end_rel % 4 == 2).any() and (end_rel % 4 == 0).any()


@pytest.mark.parametrize("avail", AVAILS)
@pytest.mark.parametrize("eth_mod16", CLASSES)
def test_window_form_inputs(eth_mod16, avail):
    for name, c in window_form_cases(eth_mod16, avail).items():
        assert (c.offsets % 16 == eth_mod16).all() and c.n >= 65, name
        # the spaced layout places every edge at each of the eight phases; packed frames fall where their lengths
        # put them, so there only the extents are required
        check_case(c, phases=name == "spaced")
    sp = ixn.spaced(eth_mod16, avail, FILL_SEEDS[0])
    assert set(sp.win_phase[:8].tolist()) == set(range(0, 128, 16))
    assert ixn.packed(eth_mod16, avail, 0).offsets[0] == eth_mod16 and ixn.packed(eth_mod16, avail, 0, 16, 3).n % 8 != 0


@pytest.mark.parametrize("avail", SEED_AVAILS)
@pytest.mark.parametrize("eth_mod16", CLASSES)
def test_spaced_records_do_not_depend_on_the_fill(eth_mod16, avail):
    a, b = (ixn.spaced(eth_mod16, avail, s) for s in FILL_SEEDS)
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.exp, b.exp)
    own = np.zeros(len(a.buf), bool)
    for o in a.offsets:
        own[int(o):int(o) + avail] = True
    assert np.array_equal(a.buf[own], b.buf[own]) and (a.buf[~own] != b.buf[~own]).mean() > 0.9


@pytest.mark.parametrize("stride,frame_off", SMALL_SLOTS)
def test_small_slot_inputs(stride, frame_off):
    from oracle import pyoracle as orc

    slots = ixn.small_slots(stride, frame_off)
    n, avail = len(slots), stride - frame_off
    e, m = ixn.conn_entries()
    exp = orc.classify_batch(np.ascontiguousarray(slots), stride, frame_off, n, e, m, ixn.MAX_CONN)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(frame_off)
    assert np.array_equal(ixn.expected(slots.reshape(-1), offsets, avail), exp)
    tot = exp["payload_off"].astype(np.int64) + exp["payload_len"] - 14
    ext = 14 + ((tot + 1) & ~1)
    ok = (exp["flags"] & ixn.TCP_OK) != 0
    assert (ok & (ext == avail)).any() and (ok & (ext > avail - 16) & (ext < avail)).any()
    assert (exp["flags"] & ixn.TRUNC).any() and ((exp["flags"] & (ixn.TCP_OK | ixn.IP_OK | ixn.TRUNC)) == ixn.IP_OK).any()
