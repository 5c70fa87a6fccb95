"""CPU: the tables, lookups and batches of tests/probe_np.py hold the cases tests/test_gpu_probe.py is about, so the
GPU file asserts nothing about its own inputs and cannot pass vacuously.  The model of findConnEntry agrees with the
C oracle and with the product's pn_table_find; every table is a layout an ordered walk can hold; per wave width,
every depth class of every tier is reached by a hit, by a miss on a larger key and by a miss at a run's end, with
each way a run can end; waves hold as many groups as lanes, groups that finish over three round trips, and nothing
but cooperative lanes; every conn_id boundary is hit in every tier; and each single-field key difference decides a
cooperative stop.  The UDP subscription sets have the chains, the wrap and the load they were searched for."""
import numpy as np
import pytest

from oracle import pyoracle as orc

import probe_np as pn
import udp_np as un


def test_constants_and_depth_classes():
    assert (pn.K_AHEAD, pn.K_WAVE) == (2, 64)
    assert pn.DEPTHS == (0, 1, 2, 3, 4, 65, 66, 67, 68, 129, 130, 131, 132)
    assert pn.END_DEPTHS == (1, 2, 3, 4, 66, 67, 68, 130, 131, 132)
    assert [pn.tier(d) for d in (0, 1, 2, 3)] == [1, 2, 2, 3]
    assert [pn.round_trip(d) for d in (2, 3, 66, 67, 130, 131, 194, 195)] == [0, 1, 1, 2, 2, 3, 3, 4]


def test_width_thresholds():
    """frames_per_wave restated: the ranges the issue's table gives, and the batch sizes inside them."""
    assert [pn.width_range(w) for w in pn.WIDTHS] == [(1, 16368), (16369, 32736), (32737, 65472), (65473, None)]
    for w in pn.WIDTHS:
        lo, hi = pn.width_range(w)
        assert pn.frames_per_wave(lo) == w and (hi is None or (pn.frames_per_wave(hi) == w and pn.frames_per_wave(hi + 1) == 2 * w))
        n1, nm = pn.batch_sizes(w)
        assert (n1 % w, nm % w) == (1, w - 1) and pn.frames_per_wave(n1) == w and pn.frames_per_wave(nm) == w
    assert [pn.svc_fpw(n, True) for n in (64, 512, 513, 1024, 1025, 2048, 2049, 4097)] == [8, 8, 16, 16, 32, 32, 64, 64]
    assert [pn.svc_fpw(n, False) for n in (1, 64, 513, 4097)] == [64] * 4


def test_key_inverse_and_frames():
    rng = np.random.default_rng(3)
    for k in [1, (1 << 48) - 1, 1 << 47, 0x7FFF, 1 << 15] + [int(x) for x in rng.integers(1, 1 << 48, 200)]:
        assert pn.src_to_key(*pn.key_to_src(k)) == k
    tb = pn.designed_table(0)
    ent = np.zeros(1, orc.ENTRY_DTYPE)
    ent["key"] = pn.EMPTY
    for i in (0, len(tb.lookups) // 2, len(tb.lookups) - 1):  # a frame is valid in every respect but its source
        r = orc.classify_frame(tb.images[i].tobytes(), pn.FRAME_W, ent, 0, 1)
        assert r["flags"] & 0x3E01 == 0x0C01, (i, r)  # IP_OK, RFC_IP_OK, RFC_TCP_OK; TCP, IHL 5, not truncated


@pytest.mark.parametrize("tb", pn.tables(), ids=lambda t: t.name)
def test_tables_are_ordered_layouts(tb):
    """Every live entry is where the ordered walk from its home slot stops; the mask is below the array length; the
    padding words are not zero in the hand-built tables."""
    assert tb.mask < len(tb.keys)
    live = [i for i, k in enumerate(tb.keys) if k != pn.EMPTY]
    for i in live:
        assert pn.find(tb.keys, tb.mask, tb.keys[i])[:2] == (i, True), (tb.name, i)
    if tb.name != "product":
        assert (tb.entries["_pad"] != 0).all()


def test_designed_runs_end_in_every_way():
    ends = {(R, e) for t in range(pn.N_DESIGNED) for R, e in _run_ends(pn.designed_table(t))}
    assert ends >= {(R, e) for R in pn.LENGTHS for e in "abc"}, sorted({(R, e) for R in pn.LENGTHS for e in "abc"} - ends)
    for t, R in enumerate(pn.LENGTHS):  # 'b': the array ends with the run, for R <= K_AHEAD inside the per-lane fetch
        tb = pn.designed_table(t)
        assert tb.keys[-1] != pn.EMPTY and (tb.keys[-R] & tb.mask) == len(tb.keys) - R
    g = pn.groups_table()
    assert g.mask >= 127 and len({k & g.mask for k in g.keys if k != pn.EMPTY}) >= pn.K_WAVE
    assert pn.product_table().mask > 127  # the product table expanded


def _run_ends(tb):
    out, i, n = [], 0, len(tb.keys)
    while i < n:
        if tb.keys[i] == pn.EMPTY:
            i += 1
            continue
        h, j = tb.keys[i] & tb.mask, i
        while j < n and tb.keys[j] != pn.EMPTY and tb.keys[j] & tb.mask == h:
            j += 1
        out.append((j - i, "b" if j == n else "a" if tb.keys[j] == pn.EMPTY else "c"))
        i = j
    return out


@pytest.mark.parametrize("tb", pn.tables(), ids=lambda t: t.name)
def test_model_agrees_with_the_oracle(tb):
    """conn_id, HIT and TW of every lookup's frame, and that the rest of the record is a valid frame's."""
    n = len(tb.lookups)
    exp = orc.classify_batch(pn.slots_of(tb.images, np.arange(n), 128, 2), 128, 2, n, tb.entries, tb.mask, tb.max_conn)
    hit = (exp["flags"] & pn.HIT) != 0
    assert np.array_equal(hit, tb.hit) and np.array_equal(exp["conn_id"], tb.cid)
    assert np.array_equal((exp["flags"] & pn.TW) != 0, tb.tw)
    assert ((exp["flags"] & 0x3E01) == 0x0C01).all()  # IP_OK, RFC_IP_OK, RFC_TCP_OK; TCP, IHL 5, not truncated
    # the reference's own sum takes in the non-zero byte behind an odd segment
    assert np.array_equal((exp["flags"] & 0x0002) != 0, exp["payload_len"] % 2 == 0)


def test_model_agrees_with_the_product_table():
    tb = pn.product_table()
    for i, k in enumerate(tb.lookups):
        e, hit, cid = tb.conn_table.find(k)
        assert (e, hit, cid) == (int(tb.e[i]), bool(tb.hit[i]), int(tb.cid[i])), hex(k)
    assert tb.hit.sum() > 30 and int(tb.depth[tb.hit].max()) >= pn.DEPTHS[-2]  # hits down to the third round trip


def _wave_stats(tb, wave):
    """(groups, most round trips one group finishes in, whether every lane is cooperative) of one wave."""
    d, h = tb.depth[list(wave)], tb.home[list(wave)]
    coop = d > pn.K_AHEAD
    groups = {}
    for dd, hh in zip(d[coop], h[coop]):
        groups.setdefault(int(hh), set()).add(pn.round_trip(int(dd)))
    return len(groups), max((len(r) for r in groups.values()), default=0), bool(coop.all())


@pytest.mark.parametrize("w", pn.WIDTHS)
def test_batches_reach_every_case(w):
    reached, cids, decided = set(), set(), set()
    most_groups, most_rts, all_coop, adjacent = 0, 0, False, False
    for tb in pn.tables():
        ws = pn.waves(tb, w)
        for n in pn.batch_sizes(w):
            idx = pn.batch_index(tb, w, n)
            assert len(idx) == n and pn.frames_per_wave(n) == w and n >= w * len(ws)
            assert np.array_equal(idx[:w * len(ws)], np.concatenate(ws))  # every wave whole, once, in front
            assert set(idx.tolist()) == set(range(len(tb.lookups)))
        for i in range(len(tb.lookups)):
            d = int(tb.depth[i])
            reached.add((d, tb.outcome[i], tb.ending[i]))
            if tb.hit[i]:
                cids.add((pn.tier(d), int(tb.cid[i])))
            if pn.tier(d) == 3 and tb.decided[i]:
                decided.add(tb.decided[i])
        for wave in ws:
            g, r, c = _wave_stats(tb, wave)
            most_groups, most_rts, all_coop = max(most_groups, g), max(most_rts, r), all_coop or c
        a = ws[pn.RECIPES.index("adjacent_homes")]
        # equal positions after the K_AHEAD step mean equal home slots; the nearest two groups can stand is one apart
        adjacent |= abs(int(tb.home[a[0]]) - int(tb.home[a[1]])) == 1 and all(tb.depth[i] > pn.K_AHEAD for i in a)
        same = ws[pn.RECIPES.index("same_key")]
        assert len(set(same)) == 1
        if tb.name.startswith("designed"):  # the recipes are what their names say
            asc = [int(tb.depth[i]) for i in ws[pn.RECIPES.index("ascending")]]
            assert asc == sorted(asc) and len(set(asc)) == w and asc[0] == 0 and asc[-1] >= pn.DEPTHS[-1]
            assert len({int(tb.home[i]) for i in ws[pn.RECIPES.index("ascending")]}) == 1
            assert [int(tb.depth[i]) for i in ws[pn.RECIPES.index("descending")]] == asc[::-1]
            il = ws[pn.RECIPES.index("interleaved")]
            assert all(tb.hit[i] and tb.depth[i] == 0 for i in il[0::2]) and all(tb.depth[i] == pn.DEPTHS[-2] for i in il[1::2])
            assert _wave_stats(tb, ws[pn.RECIPES.index("three_round_trips")]) == (1, 3, True)
            assert _wave_stats(tb, ws[pn.RECIPES.index("w_groups")])[0] == w
    print("\nwidth %d: wave with %d groups, a group over %d round trips, a wave of cooperative lanes only: %s"
          % (w, most_groups, most_rts, all_coop))
    print("  depth   hit(a b c)   larger(a b c)   end(a b c)")
    for d in pn.DEPTHS:
        print("  %5d   %s" % (d, "   ".join(" ".join("x" if (d, o, e) in reached else "." for e in "abc").center(10)
                                            for o in ("hit", "larger", "end"))))
    print("  conn_id edges hit per tier:", {t: sorted(c for tt, c in cids if tt == t and c in pn.CID_EDGES) for t in (1, 2, 3)})
    print("  single-field differences deciding a cooperative stop:", sorted(decided))
    for d in pn.DEPTHS:
        for e in "abc":
            assert (d, "hit", e) in reached and (d, "larger", e) in reached, (d, e)
            assert d not in pn.END_DEPTHS or (d, "end", e) in reached, (d, e)
    assert most_groups == w and most_rts >= 3 and all_coop and adjacent
    assert cids >= {(t, c) for t in (1, 2, 3) for c in pn.CID_EDGES}
    assert decided == {"hi", "b47", "lo"}


def test_release_records():
    """pn.release equals the oracle's own unverified records on these frames."""
    tb = pn.designed_table(3)
    slots, exp = pn.batch(tb, 8, 999)
    unv = orc.classify_batch(slots, 128, 2, 999, tb.entries, tb.mask, tb.max_conn, unverified=True)
    assert np.array_equal(pn.release(exp), unv)


# ---- the UDP subscription probe ----
def test_udp_hash_restated():
    """udp_sub_hash on a few values worked by hand in Python integers."""
    def h(ip, port):
        x = (ip ^ (port * 0x9E3779B1)) & 0xFFFFFFFF
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)

    for ip, port in ((0, 0), (0xFFFFFFFF, 0xFFFF), (0x030201EF, 0x3930), (1, 1)):
        assert int(pn.udp_sub_hash(ip, port)) == h(ip, port)
    ips = np.array([5, 0xFFFFFFFF, 0x01020304], np.uint64)
    assert [int(v) for v in pn.udp_sub_hash(ips, np.array([7, 9, 11]))] == [h(5, 7), h(0xFFFFFFFF, 9), h(0x01020304, 11)]


def test_udp_chains_and_wrap():
    subs, looks = pn.udp_case(32)
    tbl = pn.udp_table(subs)
    assert len(tbl) == 64 and sum(1 for e in tbl if e) == 32  # exactly half
    walks = [pn.udp_walk(tbl, un.stored_u32(ip), un.stored_u16(p)) for ip, p in looks]
    for i in range(32):
        assert walks[i][0] == i
    assert [walks[i][1] for i in range(12)] == list(range(1, 13))  # 12 pairs of one home slot: a chain of 12
    assert all(tbl[e] for e in list(range(pn.UDP_HOME_B, 64)) + list(range(6)))
    assert walks[21][1] >= 8 and walks[21][2]  # the tenth pair of home slot 60 is found behind the table's end
    absent = walks[32:48]
    assert all(w[0] == un.NO_SUB for w in absent) and max(w[1] for w in absent[:8]) >= 13
    assert any(w[2] and w[1] >= 11 for w in absent[8:])  # a miss that walks the whole wrapped chain to the empty entry
    near = walks[48:]
    assert sum(w[0] == un.NO_SUB for w in near) > 0.9 * len(near) and len(near) == 32 * 12
    subs33, looks33 = pn.udp_case(33)
    tbl33 = pn.udp_table(subs33)
    assert len(tbl33) == 128 and sum(1 for e in tbl33 if e) == 33  # the capacity doubled
    assert max(pn.udp_walk(tbl33, un.stored_u32(ip), un.stored_u16(p))[1] for ip, p in looks33) >= 3
    for n_subs, t, lk in ((32, tbl, looks), (33, tbl33, looks33)):
        img = pn.udp_images(n_subs)
        one = un.udp_classify_np(pn.slots_of(img, np.arange(len(lk)), 128, 2), 128, 2, pn.udp_case(n_subs)[0])
        ids = [pn.udp_walk(t, un.stored_u32(ip), un.stored_u16(p))[0] for ip, p in lk]
        assert one["sub_id"].tolist() == ids
        assert ((one["flags"] & un.IP_OK) != 0).all() and not (one["flags"] & (un.NOT_UDP | un.TRUNC | un.LEN_BAD)).any()
        m = (one["flags"] & un.MATCH) != 0
        assert ((one["flags"][m] & (un.UDP_OK | un.NOCSUM)) != 0).all() and (one["flags"] & un.NOCSUM).any()
