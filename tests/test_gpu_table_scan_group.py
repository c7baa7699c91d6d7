"""GPU: the grouped aggregate (stage_table_scan_group_aggregate, Table.table_scan_group_aggregate).

The oracle is the judge (table_scan_group_expect.py): the unfiltered expectation of
test_gpu_table_scan.py, table_scan_where_expect's match mask over it, and Python-integer group ids
and aggregates.  Every comparison is exact equality of all n_groups + 1 records.  Beside it, on every
call: the device's own records folded together equal the device's own stage_table_scan_aggregate
for the same arguments.  The tables, their modes (raw and the read ids) and the predicate classes
are the where tests'.  d_groups is pre-filled with 0xA5 and followed by a guard region: nothing past
(n_groups + 1) * 32 bytes is written.  Bases are quantiles of the oracle's column, and each
intended class (rest non-empty, rest empty, one hot group ...) is asserted on the oracle's result
before the device is asked."""
import numpy as np
import pytest

import oracle_lib as O
import stage
from stage import GROUP_LDS_MAX, Group, Pred
from table_scan_expect import LAST, raw_expect, snapshot_expects
from table_scan_group_expect import folded, group_aggregate
from table_scan_where_expect import column, domain
from test_gpu_table_scan import END, FILL, GUARD, Case, case, expect, modes, some_ranges  # noqa: F401
from test_gpu_table_scan_where import (PRIMARY, classes, device_aggregate, geometries, live_values,  # noqa: F401
                                       wcase)
from test_gpu_write_path import oracle_epoch

pytestmark = pytest.mark.gpu

U64, I64MIN, I64MAX = (1 << 64) - 1, -(1 << 63), (1 << 63) - 1
BYTE = (0, 1, False)  # the one-byte group column: every table's payload has it


def aggs(c):
    """test_aggregates' columns, and the counts alone"""
    p = c.payload
    return [None, PRIMARY, (0, 4, True), (p - 8, 8, False), (p - 8, 8, True), (p - 1, 1, True), (min(5, p - 3), 2, False)]


def tuples(c, rid):
    return int((expect(c, rid).status != 0).sum())


def quantile(c, rid, col, num=1, den=4):
    vals = live_values(c, rid, col)
    return int(vals[(vals.size - 1) * num // den])


# ------------------------------------------------------------------------------------------
# one device call into a 0xA5-filled, guarded d_groups

def device_group(c, a, b, rid, preds, group, agg, stream=None):
    """-> the (n_groups + 1) * 32 bytes the call left in d_groups; the guard behind them is checked"""
    sp = stream.ptr if stream else None
    n = 32 * (group.n_groups + 1)
    buf = stage.DeviceBuffer(n + GUARD)
    buf.memset(FILL, stream=sp)
    c.tab.table_scan_group_aggregate_device((a, b), rid, preds, group, agg, buf, stream=sp)
    if not stream:
        stage.lib().stage_device_sync()
    g = buf.to_numpy(np.uint8, buf.nbytes, stream=sp)
    assert (g[n:] == FILL).all(), (c.name, a, b, rid, preds, group, agg)
    return g[:n]


def packed(res):
    """(count, sum, min, max) arrays -> the bytes of the stage_scan_agg records"""
    return np.stack([np.asarray(x).astype(np.uint64) for x in res], axis=1).reshape(-1).view(np.uint8)


def unpacked(raw, agg):
    w = raw.view(np.uint64).reshape(-1, 4)
    t = np.int64 if agg is not None and agg[2] else np.uint64
    return w[:, 0].copy(), w[:, 1].astype(t), w[:, 2].astype(t), w[:, 3].astype(t)


def check_group(c, a, b, rid, preds, group, agg, stream=None, exp=None):
    """one call against the oracle, and its fold against the device's ungrouped aggregate;
    -> the oracle's (count, sum, min, max)"""
    hi = c.nl if b == END else b
    what = (c.name, a, b, rid, preds, group, agg)
    if exp is None:
        exp = group_aggregate(expect(c, rid), c.key_pad, preds, group, agg, a, hi)
    raw = device_group(c, a, b, rid, preds, group, agg, stream)
    if not np.array_equal(raw, packed(exp)):
        got = unpacked(raw, agg)
        bad = np.nonzero(np.any([g != e for g, e in zip(got, exp)], axis=0))[0]
        raise AssertionError((what, bad[:5], [[int(x[i]) for x in got] for i in bad[:5]],
                              [[int(x[i]) for x in exp] for i in bad[:5]]))
    assert folded(unpacked(raw, agg), agg) == device_aggregate(c, a, b, rid, preds, agg, stream), what
    return exp


# ------------------------------------------------------------------------------------------
# group counts and tiers

def test_few_groups(wcase):
    """1-byte group column, 4 groups from a quantile: the rest group and two groups or more hold records"""
    c = wcase
    for rid in modes(c):
        g = Group(*BYTE[:2], quantile(c, rid, BYTE), 4)
        for agg in aggs(c):
            count = check_group(c, 0, c.nl, rid, [], g, agg)[0]
            if tuples(c, rid) >= 1000:
                assert count[4] > 0 and (count[:4] > 0).sum() >= 2, (c.name, rid, count)


def test_byte_groups_cover_the_domain(wcase):
    """256 groups from the domain's smallest value, unsigned and signed: the rest group stays empty"""
    c = wcase
    for rid in modes(c):
        for signed in (False, True):
            for agg in (PRIMARY, (c.payload - 8, 8, True), None):
                g = Group(0, 1, domain(1, signed)[0], 256, signed=signed)
                count, s, mn, mx = check_group(c, 0, c.nl, rid, [], g, agg)
                assert int(count.sum()) == tuples(c, rid) and count[256] == 0
                if agg:
                    dlo, dhi = domain(agg[1], agg[2])
                    assert (s[256], mn[256], mx[256]) == (0, dhi, dlo)


def test_tier_boundary(wcase):
    """GROUP_LDS_MAX groups (a table per workgroup in LDS) and GROUP_LDS_MAX + 1 (global atomics) on
    the same 2-byte column and base: the records of the first GROUP_LDS_MAX groups are the same bytes"""
    c = wcase
    col = (0, 2, False)
    for rid in modes(c):
        base = quantile(c, rid, col)
        for agg in (PRIMARY, (c.payload - 8, 8, True), None):
            raws = []
            for n in (GROUP_LDS_MAX, GROUP_LDS_MAX + 1):
                g = Group(*col[:2], base, n)
                count = check_group(c, 0, c.nl, rid, [], g, agg)[0]
                if tuples(c, rid) >= 1000:
                    assert count[n] > 0 and (count[:n] > 0).sum() >= 2
                raws.append(device_group(c, 0, c.nl, rid, [], g, agg))
            assert np.array_equal(raws[0][:32 * GROUP_LDS_MAX], raws[1][:32 * GROUP_LDS_MAX]), (c.name, rid, agg)


def test_either_tier_and_any_combining_give_the_same_bytes(wcase):
    """stage_set_scan_group_tuning: the global tier at few groups, and no / full combining of a
    wave's equal-group lanes, leave the bytes of the default call"""
    c = wcase
    L = stage.lib()
    rid = modes(c)[1]
    shapes = [(Group(*BYTE[:2], quantile(c, rid, BYTE), 4), PRIMARY), (Group(0, 1, -128, 256, signed=True), (0, 4, True)),
              (Group(0, 2, quantile(c, rid, (0, 2, False)), GROUP_LDS_MAX + 1), (c.payload - 8, 8, False))]
    default = [device_group(c, 0, c.nl, rid, [], g, agg) for g, agg in shapes]
    try:
        for lds_max, combine in ((0, -1), (-1, 0), (-1, 64), (0, 0), (0, 64), (-1, 2), (3, -1)):
            assert L.stage_set_scan_group_tuning(c.tab.h, lds_max, combine) == 0
            for (g, agg), want in zip(shapes, default):
                assert np.array_equal(device_group(c, 0, c.nl, rid, [], g, agg), want), (c.name, lds_max, combine, g)
    finally:
        assert L.stage_set_scan_group_tuning(c.tab.h, -1, -1) == 0
    for (g, agg), want in zip(shapes, default):
        assert np.array_equal(want, packed(group_aggregate(expect(c, rid), c.key_pad, [], g, agg)))


def test_global_tier_covers_a_two_byte_domain(wcase):
    """65536 groups from the domain's smallest value: the rest group is empty, and so is some group"""
    c = wcase
    for rid in modes(c):
        for signed, agg in ((False, PRIMARY), (True, (c.payload - 1, 1, True)), (False, None)):
            g = Group(0, 2, domain(2, signed)[0], 65536, signed=signed)
            count = check_group(c, 0, c.nl, rid, [], g, agg)[0]
            assert count[65536] == 0 and int(count.sum()) == tuples(c, rid) and (count[:65536] == 0).any()


def test_global_tier_mostly_rest(wcase):
    """70 000 groups of a 4-byte and of an 8-byte column from a quantile: most records are in rest"""
    c = wcase
    for rid in modes(c):
        for col in ((0, 4, False), (c.payload - 8, 8, False), (c.payload - 8, 8, True)):
            g = Group(*col[:2], quantile(c, rid, col, 1, 2), 70000, signed=col[2])
            count = check_group(c, 0, c.nl, rid, [], g, PRIMARY)[0]
            if tuples(c, rid):
                assert count[:70000].sum() > 0
            if tuples(c, rid) >= 1000:
                assert count[70000] > tuples(c, rid) // 2


def test_one_hot_group_in_both_tiers(wcase):
    """a predicate that pins the group column: every lane of every wave updates one entry"""
    c = wcase
    for rid in modes(c):
        v = quantile(c, rid, BYTE, 1, 2)
        preds = [Pred(*BYTE[:2], v, v)]
        for n, base in ((8, max(v - 3, 0)), (GROUP_LDS_MAX + 1, 0)):
            for agg in (PRIMARY, (c.payload - 8, 8, True), None):
                count = check_group(c, 0, c.nl, rid, preds, Group(*BYTE[:2], base, n), agg)[0]
                assert (count > 0).sum() == (1 if tuples(c, rid) else 0) and count[n] == 0
                assert int(count[v - base]) == device_aggregate(c, 0, c.nl, rid, preds, agg)[0]


def test_edges_of_the_domain(wcase):
    c = wcase
    p = c.payload
    for rid in modes(c):
        top = int(live_values(c, rid, (p - 8, 8, False))[-1])
        groups = [
            Group(0, 1, 250, 16),                          # groups 6 .. 15 are unreachable: identities
            Group(p - 8, 8, U64 - 2, 3), Group(p - 8, 8, U64 - 2, 8),
            Group(p - 8, 8, top - 1, 8),                   # the column's largest value in group 1
            Group(p - 8, 8, I64MAX - 2, 8, signed=True), Group(p - 8, 8, I64MIN, 8, signed=True),
            Group(0, 2, -3, 8, signed=True),
            Group(0, 1, 300, 4), Group(0, 1, -200, 100, signed=True),  # a base outside the column's domain
        ]
        for i, g in enumerate(groups):
            agg = aggs(c)[1 + i % 6]
            count, s, mn, mx = check_group(c, 0, c.nl, rid, [], g, agg)
            dlo, dhi = domain(agg[1], agg[2])
            if i == 0:
                assert not count[6:16].any() and not s[6:16].any() and (mn[6:16] == dhi).all() and (mx[6:16] == dlo).all()
            if i == 3 and tuples(c, rid):
                assert count[1] > 0 and not count[2:8].any()
            if i == 7:
                assert int(count[4]) == tuples(c, rid)
            check_group(c, 0, c.nl, rid, [], g, None)


def test_group_column_geometries(wcase):
    """the group column at every width, sign and alignment of the where tests' geometries: crossing
    an 8-B word, a 16-B chunk and a 128-B line of the heap row, and the payload's last bytes"""
    c = wcase
    for rid in modes(c):
        for i, col in enumerate(geometries(c)):
            off, width, signed = col
            n, base = (256, domain(1, signed)[0]) if width == 1 else (64, quantile(c, rid, col))
            g = Group(off, width, base, n, signed=signed)
            count = check_group(c, 0, c.nl, rid, [], g, aggs(c)[1 + i % 6])[0]
            if tuples(c, rid):
                assert count[:n].sum() > 0, (c.name, rid, col)
            check_group(c, 0, c.nl, rid, [], g, None)


def key_groups(c):
    """a byte and an 8-byte field of the key under which the oracle shows two non-empty groups or more"""
    e = c.raw
    out = []
    for width in (1, 8):
        for off in range(0, c.key_pad - width + 1, width):
            vals = column(e.rows, 0, off, width, False)
            g = Group(off, width, int(vals.min()), 16, in_key=True)
            if (group_aggregate(e, c.key_pad, [], g, None)[0][:16] > 0).sum() >= 2:
                out.append(g)
                break
    return out


def test_key_field_as_the_group_column(wcase):
    c = wcase
    groups = key_groups(c)
    if c.name in ("ycsb", "key16", "key32"):
        assert {g.width for g in groups} == {1, 8}, (c.name, groups)
    for rid in modes(c):
        for g in groups:
            for agg in (PRIMARY, None):
                check_group(c, 0, c.nl, rid, [], g, agg)
            check_group(c, 0, c.nl, rid, classes(c, rid)["half"], g, (c.payload - 8, 8, True))
    # the field's last byte is the key pad's last byte
    check_group(c, 0, c.nl, None, [], Group(c.key_pad - 1, 1, 0, 256, in_key=True), PRIMARY)


# ------------------------------------------------------------------------------------------
# the record set: snapshot modes, predicates, ranges

def test_records_without_a_tuple_take_no_part(wcase):
    c = wcase
    seen = False
    for rid in c.rids:
        e = expect(c, rid)
        gone = int((e.status == stage.ST_NOT_FOUND).sum())
        for g in (Group(0, 1, 0, 256), Group(0, 2, 0, 65536)):
            count = check_group(c, 0, c.nl, rid, [], g, PRIMARY)[0]
            assert int(count.sum()) == e.meta.size - gone
        if gone:
            seen = True
            assert int(count.sum()) < e.meta.size
    if c.name == "ycsb":
        assert seen


def test_predicate_classes(wcase):
    c = wcase
    for rid in modes(c):
        cl = classes(c, rid)
        few = Group(*BYTE[:2], quantile(c, rid, BYTE), 4)
        many = Group(0, 2, quantile(c, rid, (0, 2, False)), GROUP_LDS_MAX + 1)
        for name in ("nothing", "half", "four", "none"):
            for g in (few, many):
                for agg in (PRIMARY, (c.payload - 8, 8, True)):
                    count, s, mn, mx = check_group(c, 0, c.nl, rid, cl[name], g, agg)
                    if name == "nothing":  # every record the identities
                        dlo, dhi = domain(agg[1], agg[2])
                        assert not count.any() and not s.any() and (mn == dhi).all() and (mx == dlo).all()
                check_group(c, 0, c.nl, rid, cl[name], g, None)


def test_ranges(wcase):
    c = wcase
    for rid in modes(c):
        preds = classes(c, rid)["half"]
        few = Group(*BYTE[:2], quantile(c, rid, BYTE), 4)
        many = Group(0, 2, quantile(c, rid, (0, 2, False)), GROUP_LDS_MAX + 1)
        for g, agg in ((few, (0, 2, True)), (many, (c.payload - 8, 8, False))):
            for a, b in some_ranges(c):
                check_group(c, a, b, rid, preds, g, agg)
            check_group(c, c.nl - 1, END, rid, preds, g, agg)
            whole = check_group(c, 0, END, rid, preds, g, agg)
            # empty ranges: all identities
            dlo, dhi = domain(agg[1], agg[2])
            n = g.n_groups + 1
            for a in (0, c.nl // 2, c.nl):
                count, s, mn, mx = check_group(c, a, a, rid, preds, g, agg)
                assert not count.any() and not s.any() and (mn == dhi).all() and (mx == dlo).all()
                assert not device_group(c, a, a, rid, [], g, None).any()  # counts alone: zeros
            # consecutive ranges fold to the whole-range result
            cuts = sorted({0, 1, c.nl // 3, c.nl // 2, c.nl - 1, c.nl})
            parts = [unpacked(device_group(c, a, b, rid, preds, g, agg), agg) for a, b in zip(cuts[:-1], cuts[1:])]
            t = whole[1].dtype
            with np.errstate(over="ignore"):
                assert np.array_equal(np.sum([p[0] for p in parts], axis=0, dtype=np.uint64), whole[0])
                assert np.array_equal(np.sum([p[1].astype(np.uint64) for p in parts], axis=0, dtype=np.uint64).astype(t),
                                      whole[1])
            assert np.array_equal(np.min([p[2] for p in parts], axis=0), whole[2])
            assert np.array_equal(np.max([p[3] for p in parts], axis=0), whole[3])
            assert len(whole[0]) == n


def test_one_block_grid_gives_the_same_bytes(wcase):
    c = wcase
    L = stage.lib()
    calls = []
    for rid in modes(c)[:2]:
        cl = classes(c, rid)
        few = Group(*BYTE[:2], quantile(c, rid, BYTE), 4)
        many = Group(0, 2, quantile(c, rid, (0, 2, False)), GROUP_LDS_MAX + 1)
        full = Group(0, 2, quantile(c, rid, (0, 2, False)), GROUP_LDS_MAX)
        for g in (few, full, many):
            for name in ("half", "none"):
                for agg in (PRIMARY, (c.payload - 8, 8, True), None):
                    calls.append((rid, cl[name], g, agg))
    default = [device_group(c, 0, c.nl, rid, preds, g, agg) for rid, preds, g, agg in calls]
    try:
        assert L.stage_set_scan_tuning(c.tab.h, 1) == 0
        for (rid, preds, g, agg), want in zip(calls, default):
            assert np.array_equal(device_group(c, 0, c.nl, rid, preds, g, agg), want), (c.name, rid, preds, g, agg)
    finally:
        assert L.stage_set_scan_tuning(c.tab.h, 0) == 0
    for (rid, preds, g, agg), want in zip(calls[::3], default[::3]):
        assert np.array_equal(want, packed(group_aggregate(expect(c, rid), c.key_pad, preds, g, agg)))


def test_call_is_ordered_on_the_callers_stream(wcase):
    """the fill, the call and the D2H copy on one caller stream and nothing else"""
    c = wcase
    s = stage.Stream()
    for rid in modes(c)[:2]:
        preds = classes(c, rid)["half"]
        for n in (4, GROUP_LDS_MAX + 1):
            check_group(c, 0, c.nl, rid, preds, Group(*BYTE[:2], 0, n), PRIMARY, stream=s)
            check_group(c, 0, c.nl, rid, preds, Group(*BYTE[:2], 0, n), None, stream=s)


def test_a_sum_that_wraps(wcase):
    c = wcase
    if c.name != "ycsb":
        return
    agg, g = (8, 8, False), Group(*BYTE[:2], 0, 4)
    x = column(c.raw.rows, c.key_pad, *agg)
    b = column(c.raw.rows, c.key_pad, *BYTE)
    assert sum(int(v) for v in x[b == 1]) >= 1 << 64  # group 1's true sum does not fit 64 bits
    for lds_max in (-1, 0):
        try:
            assert stage.lib().stage_set_scan_group_tuning(c.tab.h, lds_max, -1) == 0
            s = check_group(c, 0, c.nl, None, [], g, agg)[1]
        finally:
            assert stage.lib().stage_set_scan_group_tuning(c.tab.h, -1, -1) == 0
        assert int(s[1]) == sum(int(v) for v in x[b == 1]) % (1 << 64)


def test_high_level_form(wcase):
    c = wcase
    for rid in modes(c):
        preds = classes(c, rid)["half"]
        for g, agg in ((Group(*BYTE[:2], quantile(c, rid, BYTE), 4), (c.payload - 8, 8, True)),
                       (Group(0, 2, -32768, 65536, signed=True), PRIMARY), (Group(0, 1, 0, 256), None)):
            res = c.tab.table_scan_group_aggregate(read_id=rid, preds=preds, group=g, agg=agg)
            exp = group_aggregate(expect(c, rid), c.key_pad, preds, g, agg)
            t = np.int64 if agg and agg[2] else np.uint64
            assert isinstance(res, stage.GroupAggregates) and [x.dtype for x in res] == [np.uint64, t, t, t]
            assert all(x.shape == (g.n_groups + 1,) for x in res)
            for name, got, want in zip(res._fields, res, exp):
                assert got.dtype == want.dtype and np.array_equal(got, want), (c.name, rid, g, agg, name)
            assert np.array_equal(packed(res), device_group(c, 0, c.nl, rid, preds, g, agg))
        a, b = some_ranges(c)[1]
        res = c.tab.table_scan_group_aggregate(leaves=(a, b), read_id=rid, group=(0, 1, 0, 256))  # a plain tuple
        assert np.array_equal(res.count, group_aggregate(expect(c, rid), c.key_pad, [], Group(0, 1, 0, 256), None, a, b)[0])
        assert not res.sum.any() and not res.min.any() and not res.max.any()


# ------------------------------------------------------------------------------------------
# right behind a device write epoch

def test_group_aggregate_after_a_device_write_epoch(gpu):
    """update_batch_device, then the grouped call on the same stream with no synchronisation
    between: it groups on the byte of the patched column that the epoch sets, and sees it"""
    n, m = 4000, 1500
    base = np.arange(n, dtype=np.uint64) * 4
    c = Case()
    c.name, c.key_width = "epoch", 8
    c.tab, c.orc = stage.Table(key_width=8), O.OracleTree()
    c.tab.load_keys(base, 8, mode=1)
    c.orc.load_keys(base, 8, 1)
    c.tab.sync()
    rng = np.random.default_rng(79)
    keys = rng.choice(base, m).astype(np.uint64)
    keys[rng.random(m) < 0.05] += 1  # absent
    off, dlen = 203, 24
    deltas = rng.integers(0, 256, (m, dlen), dtype=np.uint8)
    deltas[:, 3] = 0x5A  # the patched column's top byte: 0x5A in a patched row
    wid = (10 + 2 * np.arange(m)).astype(np.uint32)
    cid = (wid + 1).astype(np.uint32)
    cid[rng.random(m) < 0.1] = 0  # left in flight
    col = (off, 4, False)
    few, many = Group(off + 3, 1, 0x58, 4), Group(off + 2, 2, 0x5A00, GROUP_LDS_MAX + 1)
    before = c.tab.table_scan_group_aggregate(group=few, agg=col).count
    d_few, d_many = stage.DeviceBuffer(32 * 5), stage.DeviceBuffer(32 * (GROUP_LDS_MAX + 2))
    rc, ok = c.tab.update_batch_device(keys, off, deltas, wid, cid)
    c.tab.table_scan_group_aggregate_device(None, None, [], few, col, d_few)
    c.tab.table_scan_group_aggregate_device(None, None, [], many, col, d_many)
    stage.lib().stage_device_sync()
    exp = oracle_epoch(c.orc, keys, 8, off, deltas, wid, cid)
    assert (rc == exp).all() and ok == int((exp == stage.RC_OK).sum()) and ok > m // 2
    raw = raw_expect(c.orc)
    c.rids = (LAST, int(cid.max()) // 2, 5)
    c.raw, c.snap = raw, snapshot_expects(c.orc, raw, 8, c.rids)
    c.nl, c.key_pad, c.payload = raw.leaves, 8, c.orc.payload_size
    want = group_aggregate(raw, 8, [], few, col)
    assert int(want[0][2]) > int(before[2]) + m // 4  # the patched rows are group 2
    assert np.array_equal(d_few.to_numpy(np.uint8, 32 * 5), packed(want))
    want = group_aggregate(raw, 8, [], many, col)
    assert int(want[0][:GROUP_LDS_MAX + 1].sum()) > m // 4
    assert np.array_equal(d_many.to_numpy(np.uint8, 32 * (GROUP_LDS_MAX + 2)), packed(want))
    # and the contract on the epoch's image, every mode
    for rid in modes(c):
        for g in (few, many):
            check_group(c, 0, c.nl, rid, [], g, col)
            check_group(c, 0, c.nl, rid, [Pred(off, 4, 0x5A000000, 0x5AFFFFFF)], g, None)
