"""GPU: filtered whole-table scans (stage_table_scan_where / _where_window / _aggregate,
Table.table_scan_where / table_scan_aggregate).

The oracle is the judge (table_scan_where_expect.py): the unfiltered expectation of
test_gpu_table_scan.py, a numpy mask over it (a tuple, and every predicate on the row bytes at
key_pad + off), and Python-integer aggregates.  Beside it the contract in its own words: the
filtered outputs are the device's unfiltered table_scan outputs indexed by that mask.  The tables,
their modes (raw and the read ids) and their windows are test_gpu_table_scan.py's.  Every buffer is
pre-filled with 0xA5 and carries a guard region: nothing at or past min(count, max_records), or
past the buffer's end, is written.  Predicate thresholds are quantiles of the oracle's column, and
each intended class (nothing, everything, half, sparse ...) is asserted on the oracle's result
before the device is asked."""
import numpy as np
import pytest

import oracle_lib as O
import stage
from stage import Pred
from table_scan_expect import LAST, raw_expect, snapshot_expects
from table_scan_where_expect import Filtered, aggregate, column, domain, match_mask, raw_slots, snapshot_slots
from test_gpu_table_scan import (END, FILL, GUARD, TABLES, Case, case, device_scan, expect, modes,  # noqa: F401
                                 some_ranges)
from test_gpu_write_path import oracle_epoch

pytestmark = pytest.mark.gpu

PRIMARY = (0, 4, False)  # the column the predicate classes are cut on: every table's payload has it


@pytest.fixture(scope="module")
def wcase(case):  # noqa: F811
    """test_gpu_table_scan's case, plus each mode's (leaf, slot) numbers from the oracle's blocks"""
    c = case
    c.payload = c.orc.payload_size
    raw = raw_slots(c.orc, c.tab.key_words)
    assert raw.size == c.raw.meta.size
    c.slots = {None: raw}
    for rid in c.rids:
        c.slots[rid] = snapshot_slots(c.raw, raw, c.key_width)
        assert c.slots[rid].size == c.snap[rid].meta.size
    c.filtered, c.classes = {}, {}
    return c


def filtered(c, rid, preds):
    key = (rid, tuple(preds))
    if key not in c.filtered:
        c.filtered[key] = Filtered(expect(c, rid), c.slots[rid], match_mask(expect(c, rid), c.key_pad, preds))
    return c.filtered[key]


def live_values(c, rid, col):
    """the column over the records that yield a tuple (raw mode's when the mode yields none)"""
    e = expect(c, rid)
    if not (e.status != 0).any():
        e = c.raw
    return np.sort(column(e.rows, c.key_pad, *col)[e.status != 0])


# ------------------------------------------------------------------------------------------
# predicate classes on the primary column, asserted on the oracle

def classes(c, rid):
    """-> {name: preds}, each class asserted on the oracle's result (once per mode)"""
    if rid not in c.classes:
        c.classes[rid] = make_classes(c, rid)
    return c.classes[rid]


def make_classes(c, rid):
    e = expect(c, rid)
    off, width, signed = PRIMARY
    vals = live_values(c, rid, PRIMARY)
    tuples = int((e.status != 0).sum())
    dlo, dhi = domain(width, signed)
    med = int(vals[(vals.size - 1) // 2])
    have = set(vals.tolist())
    absent = next(x for x in range(dlo, dhi) if x not in have)
    out = {
        "nothing": [Pred(off, width, absent, absent)],
        "everything": [Pred(off, width, dlo, dhi)],
        "half": [Pred(off, width, dlo, med)],
        "not_half": [Pred(off, width, dlo, med, negate=True)],
        "inverted": [Pred(off, width, med, med - 1)],
        "not_inverted": [Pred(off, width, med, med - 1, negate=True)],
        "none": [],
    }
    # sparse: the k smallest values, k as large as still leaves one leaf without a match and one
    # leaf with exactly one (a table of one leaf has no second leaf: one match in it)
    for k in range(max(c.nl // 2, 1), 0, -1):
        sparse = [Pred(off, width, dlo, int(vals[k - 1]))]
        per_leaf = filtered(c, rid, sparse).counts
        if (per_leaf == 1).any() and ((per_leaf == 0).any() or c.nl == 1):
            break
    out["sparse"] = sparse
    # four at once, on four columns: half on the primary, the upper three quarters of a signed
    # column, a one-byte interval at the row's end, and the complement of a two-byte interval
    p = c.payload
    s4 = (4, 4, True) if p == 8 else (6, 4, True)
    q = live_values(c, rid, s4)
    out["four"] = [Pred(off, width, dlo, med), Pred(*s4[:2], int(q[q.size // 4]), domain(4, True)[1], signed=True),
                   Pred(p - 1, 1, -100, 100, signed=True), Pred(min(5, p - 3), 2, 0, 0x0FFF, negate=True)]

    f = {name: filtered(c, rid, preds) for name, preds in out.items()}
    n = {name: int(x.offsets[-1]) for name, x in f.items()}
    assert n["nothing"] == n["inverted"] == 0 and not f["nothing"].offsets.any()
    assert n["everything"] == n["none"] == n["not_inverted"] == tuples
    assert n["half"] + n["not_half"] == tuples  # the complement among the tuple-yielding records only
    assert not (f["half"].mask & f["not_half"].mask).any()
    assert np.array_equal(f["half"].mask | f["not_half"].mask, e.status != 0)
    if tuples:
        # half: the records up to the median (a value shared by several records counts for all)
        assert (tuples + 1) // 2 <= n["half"] <= (tuples + 1) // 2 + tuples // 100
        assert 0 < n["sparse"] <= max(c.nl // 2, 1) + tuples // 100
        assert (f["sparse"].counts == 1).any() and ((f["sparse"].counts == 0).any() or c.nl == 1)
        if tuples >= 100:
            assert 0 < n["four"] < n["half"]
        if e.counts.max() > 128:  # a large-leaf table: the emit list crosses a 64-rank chunk
            assert f["half"].counts.max() > 64, (c.name, rid)
    return out


def test_not_found_records_never_match(wcase):
    """a snapshot mode with ST_NOT_FOUND records: "everything" is strictly below the unfiltered count"""
    c = wcase
    seen = False
    for rid in c.rids:
        e = expect(c, rid)
        gone = int((e.status == stage.ST_NOT_FOUND).sum())
        for preds in ([], [Pred(0, 1, 0, 255)], [Pred(0, 1, 5, 4, negate=True)]):
            assert int(filtered(c, rid, preds).offsets[-1]) == e.meta.size - gone
        if gone:
            seen = True
            assert int(filtered(c, rid, []).offsets[-1]) < e.meta.size
            got = device_where(c, 0, c.nl, rid, [])
            check_where(c, got, 0, c.nl, rid, [])
            assert got["count"][:8].view(np.uint64)[0] == e.meta.size - gone < e.meta.size
    if c.name == "ycsb":
        assert seen


# ------------------------------------------------------------------------------------------
# one device call into 0xA5-filled, guarded buffers

def device_where(c, a, b, rid, preds, window=None, max_records=None, offsets=True, meta=True, status=True, keys=True,
                 slot=True, room=None, stream=None):
    """-> dict of the raw output arrays (guards included); `room` = records the buffers hold"""
    f = filtered(c, rid, preds)
    hi = c.nl if b == END else b
    nl = hi - a
    total = int(f.offsets[hi]) - int(f.offsets[a])
    m = total if max_records is None else max_records
    room = max(total, m) if room is None else room
    width = c.stride if window is None else stage.window_stride(window[1])
    sp = stream.ptr if stream else None
    bufs = {"count": stage.DeviceBuffer(8 + GUARD)}
    if offsets:
        bufs["offsets"] = stage.DeviceBuffer((nl + 1) * 8 + GUARD)
    if m:
        bufs["out"] = stage.DeviceBuffer(room * width + GUARD)
    if meta:
        bufs["meta"] = stage.DeviceBuffer(room * 8 + GUARD)
    if status:
        bufs["status"] = stage.DeviceBuffer(room + GUARD)
    if slot:
        bufs["slot"] = stage.DeviceBuffer(room * 8 + GUARD)
    if keys and window is not None:
        bufs["keys"] = stage.DeviceBuffer(room * c.key_pad + GUARD)
    for buf in bufs.values():
        buf.memset(FILL, stream=sp)
    c.tab.table_scan_where_device((a, b), rid, preds, m, bufs["count"], bufs.get("offsets"), bufs.get("out"), window,
                                  bufs.get("keys"), bufs.get("slot"), bufs.get("meta"), bufs.get("status"), stream=sp)
    if not stream:
        stage.lib().stage_device_sync()
    got = {k: v.to_numpy(np.uint8, v.nbytes, stream=sp) for k, v in bufs.items()}
    got.update(width=width, room=room, m=m, nl=nl)
    return got


def check_where(c, got, a, b, rid, preds, window=None):
    """the raw arrays of device_where against the oracle's matching records of leaves [a, b)"""
    f = filtered(c, rid, preds)
    b = c.nl if b == END else b
    total, offs, meta, status, rows, slots = f.range(a, b)
    m, width = got["m"], got["width"]
    k = min(total, m)
    what = (c.name, a, b, rid, preds, window, m)
    cnt = got["count"]
    assert cnt[:8].view(np.uint64)[0] == total, what
    assert (cnt[8:] == FILL).all(), what
    if "offsets" in got:
        o = got["offsets"]
        assert np.array_equal(o[:(got["nl"] + 1) * 8].view(np.uint64), offs), what
        assert (o[(got["nl"] + 1) * 8:] == FILL).all(), what
    for name, exp in (("meta", meta), ("slot", slots)):
        if name in got:
            g = got[name]
            assert np.array_equal(g[:k * 8].view(np.uint64), exp[:k]), (what, name)
            assert (g[k * 8:] == FILL).all(), (what, name)
    if "status" in got:
        g = got["status"]
        assert np.array_equal(g[:k], status[:k]), what
        assert (g[k:] == FILL).all(), what
        assert (g[:k] != stage.ST_NOT_FOUND).all(), what
    if "out" not in got:
        return
    out = got["out"]
    assert (out[k * width:] == FILL).all(), what  # past min(count, max_records), and the guard
    out = out[:k * width].reshape(k, width)
    if window is None:
        bad = np.nonzero((out[:, :c.row] != rows[:k]).any(axis=1))[0]
        assert bad.size == 0, (what, bad[:5])
    else:
        off, ln = window
        bad = np.nonzero((out[:, :ln] != rows[:k, c.key_pad + off:c.key_pad + off + ln]).any(axis=1))[0]
        assert bad.size == 0, (what, bad[:5])
        assert not out[:, ln:].any(), what
        if "keys" in got:
            g = got["keys"]
            assert np.array_equal(g[:k * c.key_pad].reshape(k, c.key_pad), rows[:k, :c.key_pad]), what
            assert (g[k * c.key_pad:] == FILL).all(), what
    return out


def device_aggregate(c, a, b, rid, preds, agg, stream=None):
    """-> (count, sum, min, max) as Table.table_scan_aggregate returns them, from a guarded d_agg"""
    sp = stream.ptr if stream else None
    buf = stage.DeviceBuffer(32 + GUARD)
    buf.memset(FILL, stream=sp)
    c.tab.table_scan_aggregate_device((a, b), rid, preds, agg, buf, stream=sp)
    if not stream:
        stage.lib().stage_device_sync()
    g = buf.to_numpy(np.uint8, buf.nbytes, stream=sp)
    assert (g[32:] == FILL).all(), (c.name, a, b, rid, preds, agg)
    signed = agg is not None and agg[2]
    w = g[:32].view(np.int64 if signed else np.uint64)
    return (int(g[:8].view(np.uint64)[0]),) + tuple(int(x) for x in w[1:])


# ------------------------------------------------------------------------------------------
# rows, windows, optional outputs

def test_predicate_classes_rows(wcase):
    c = wcase
    for rid in modes(c):
        for name, preds in classes(c, rid).items():
            got = device_where(c, 0, c.nl, rid, preds)
            check_where(c, got, 0, c.nl, rid, preds)
            if name in ("nothing", "inverted"):
                assert "out" not in got  # no record byte to write: count 0, every offset 0
                assert not got["offsets"][:(c.nl + 1) * 8].any()
                assert (got["meta"] == FILL).all() and (got["status"] == FILL).all() and (got["slot"] == FILL).all()
                # ... and none written into a buffer that has room
                got = device_where(c, 0, END, rid, preds, max_records=7, room=7)
                check_where(c, got, 0, END, rid, preds)
                assert (got["out"] == FILL).all()


def test_predicate_classes_windows(wcase):
    c = wcase
    for rid in modes(c):
        cl = classes(c, rid)
        for name in ("half", "sparse", "four", "not_half", "none"):
            for window in c.windows if name in ("half", "sparse") else c.windows[:1]:
                check_where(c, device_where(c, 0, c.nl, rid, cl[name], window=window), 0, c.nl, rid, cl[name], window)
        res = c.tab.table_scan_where(read_id=rid, preds=cl["half"], window=c.windows[-1], row_keys=True, row_meta=True,
                                     row_slot=True)
        f = filtered(c, rid, cl["half"])
        off, ln = c.windows[-1]
        assert res.count == int(f.offsets[-1]) and res.records.shape == (res.count, stage.window_stride(ln))
        assert np.array_equal(res.records[:, :ln], f.rows[:, c.key_pad + off:c.key_pad + off + ln])
        assert np.array_equal(res.keys, f.rows[:, :c.key_pad]) and np.array_equal(res.slots, f.slots)
        assert np.array_equal(res.meta, f.meta) and np.array_equal(res.status, f.status)
        assert np.array_equal(res.offsets, f.offsets)


def test_count_only_and_optional_outputs(wcase):
    c = wcase
    for rid in modes(c):
        preds = classes(c, rid)["half"]
        for window in (None, c.windows[0]):
            got = device_where(c, 0, c.nl, rid, preds, window=window, max_records=0)  # null record buffer
            assert "out" not in got
            check_where(c, got, 0, c.nl, rid, preds, window)
            got = device_where(c, 0, END, rid, preds, window=window, max_records=0, offsets=False, meta=False,
                               status=False, keys=False, slot=False)
            assert set(got) == {"count", "width", "room", "m", "nl"}
            check_where(c, got, 0, END, rid, preds, window)
            got = device_where(c, 0, c.nl, rid, preds, window=window, offsets=False, meta=False, status=False,
                               keys=False, slot=False)
            check_where(c, got, 0, c.nl, rid, preds, window)
            for absent in ("offsets", "meta", "status", "keys", "slot"):  # each optional output absent
                got = device_where(c, 0, c.nl, rid, preds, window=window, **{absent: False})
                assert absent not in got
                check_where(c, got, 0, c.nl, rid, preds, window)


# ------------------------------------------------------------------------------------------
# column geometries: widths, signs, alignments, the row's last bytes

def geometries(c):
    """(off, width, signed) columns: every width signed and unsigned at offset 0, the row's last
    bytes, and the offsets that cross an 8-B word, a 16-B chunk and a 128-B line of the heap row
    (with key_pad 8: width 4 at 6 and at 118; width 2 at 5 and width 8 at 0 on an 8-byte payload)"""
    p, kp = c.payload, c.key_pad
    g = [(0, w, s) for w in (1, 2, 4, 8) for s in (False, True)]
    g += [(p - 8, 8, False), (p - 8, 8, True), (p - 1, 1, False), (p - 1, 1, True), (5, 2, False), (5, 2, True)]
    chunk = (14 - kp) % 16          # row bytes 14..17 mod 16: two 16-B chunks (and two 8-B words)
    line = 126 - kp                 # row bytes 126..129: two 128-B lines
    for off in (chunk, line, 3):
        for w in (4, 8):
            if off + w <= p:
                g += [(off, w, False), (off, w, True)]
    if kp == 8 and p >= 122:
        assert (6, 4, False) in g and (118, 4, True) in g
    return sorted(set(g))


def geometry_preds(c, rid, col):
    """per column: its lower half, and the sign / top-bit half that the extension decides"""
    off, width, signed = col
    vals = live_values(c, rid, col)
    dlo, dhi = domain(width, signed)
    med = int(vals[(vals.size - 1) // 2])
    if signed:
        top = Pred(off, width, dlo, -1, signed=True)                  # the negatives among the values
        assert vals.size < 100 or ((vals < 0).any() and (vals >= 0).any()), (c.name, col)
    else:
        top = Pred(off, width, (dhi >> 1) + 1, dhi)                   # width 8: the values above 2^63
        assert vals.size < 100 or ((vals > np.uint64(dhi >> 1)).any() and (vals <= np.uint64(dhi >> 1)).any()), \
            (c.name, col)
    return [[Pred(off, width, dlo, med, signed=signed)], [top]]


def test_column_geometries(wcase):
    c = wcase
    window = c.windows[0]
    for rid in modes(c):
        tuples = int((expect(c, rid).status != 0).sum())
        for col in geometries(c):
            for preds in geometry_preds(c, rid, col):
                n = int(filtered(c, rid, preds).offsets[-1])
                assert tuples < 100 or 0 < n < tuples, (c.name, rid, preds, n)
                got = device_where(c, 0, c.nl, rid, preds, window=window, meta=False, keys=False)
                check_where(c, got, 0, c.nl, rid, preds, window)
                assert device_aggregate(c, 0, END, rid, preds, col) == aggregate(expect(c, rid), c.key_pad, preds,
                                                                                  col), (c.name, rid, preds)
            assert device_aggregate(c, 0, c.nl, rid, [], col) == aggregate(expect(c, rid), c.key_pad, [], col)


# ------------------------------------------------------------------------------------------
# ranges, truncation, the grid cap, a caller's stream

def test_sub_ranges_and_concatenation(wcase):
    c = wcase
    for rid in modes(c):
        cl = classes(c, rid)
        for name in ("half", "sparse"):
            preds = cl[name]
            for a, b in some_ranges(c) + [(0, 0), (c.nl // 2, c.nl // 2), (c.nl, c.nl)]:
                check_where(c, device_where(c, a, b, rid, preds), a, b, rid, preds)
                check_where(c, device_where(c, a, b, rid, preds, window=c.windows[0]), a, b, rid, preds, c.windows[0])
                assert device_aggregate(c, a, b, rid, preds, PRIMARY) == aggregate(expect(c, rid), c.key_pad, preds,
                                                                                   PRIMARY, a, b)
            check_where(c, device_where(c, c.nl - 1, END, rid, preds), c.nl - 1, END, rid, preds)
            check_where(c, device_where(c, 0, END, rid, preds, window=c.windows[0]), 0, END, rid, preds, c.windows[0])
        # consecutive ranges concatenate to the whole-range result
        preds = cl["half"]
        cuts = sorted({0, 1, c.nl // 3, c.nl // 2, c.nl - 1, c.nl})
        parts = [c.tab.table_scan_where(leaves=(a, b), read_id=rid, preds=preds, row_meta=True, row_slot=True)
                 for a, b in zip(cuts[:-1], cuts[1:])]
        whole = c.tab.table_scan_where(read_id=rid, preds=preds, row_meta=True, row_slot=True)
        assert sum(p.count for p in parts) == whole.count == int(filtered(c, rid, preds).offsets[-1])
        for f in ("records", "meta", "status", "slots"):
            assert np.array_equal(np.concatenate([getattr(p, f) for p in parts]), getattr(whole, f)), f
        assert np.array_equal(np.concatenate([p.offsets[:-1] + whole.offsets[a] for p, a in zip(parts, cuts)]),
                              whole.offsets[:-1])


def test_truncation_leaves_the_rest_untouched(wcase):
    c = wcase
    for rid in modes(c):
        preds = classes(c, rid)["half"]
        f = filtered(c, rid, preds)
        total = int(f.offsets[-1])
        for m in sorted({max(total - 5, 1), 1}):
            for window in (None, c.windows[0]):
                got = device_where(c, 0, c.nl, rid, preds, window=window, max_records=m, room=max(total, m))
                check_where(c, got, 0, c.nl, rid, preds, window)  # d_count is the total; bytes at and past m keep the fill
        if not total:
            continue
        # a caller whose output was cut resumes at the first leaf that was not delivered whole
        whole = c.tab.table_scan_where(read_id=rid, preds=preds)
        for m in sorted({int(f.offsets[c.nl // 2]), int(f.offsets[c.nl // 2]) + 1, 2}):
            first = c.tab.table_scan_where(read_id=rid, preds=preds, max_records=m)
            assert first.count == whole.count and first.records.shape[0] == min(m, whole.count)
            assert np.array_equal(first.offsets, whole.offsets)
            nxt = int(np.nonzero(first.offsets[1:] > m)[0][0]) if m < whole.count else c.nl
            if nxt < c.nl:
                assert first.offsets[nxt] <= m < first.offsets[nxt + 1]  # the leaf the cut fell into
            rest = c.tab.table_scan_where(leaves=(nxt, END), read_id=rid, preds=preds)
            keep = int(first.offsets[nxt])
            assert np.array_equal(np.concatenate([first.records[:keep], rest.records]), whole.records)


def test_one_block_grid_strides_over_the_leaves(wcase):
    c = wcase
    L = stage.lib()
    aggs = [None, PRIMARY, (c.payload - 8, 8, False), (0, 2, True)]
    default = {}
    for rid in modes(c)[:2]:
        for name, preds in classes(c, rid).items():
            for agg in aggs:
                default[rid, name, agg] = device_aggregate(c, 0, c.nl, rid, preds, agg)
                assert default[rid, name, agg] == aggregate(expect(c, rid), c.key_pad, preds, agg)
    try:
        assert L.stage_set_scan_tuning(c.tab.h, 1) == 0
        for rid in modes(c)[:2]:
            cl = classes(c, rid)
            for name in ("half", "sparse"):
                check_where(c, device_where(c, 0, c.nl, rid, cl[name]), 0, c.nl, rid, cl[name])
                check_where(c, device_where(c, 0, END, rid, cl[name], window=c.windows[0]), 0, END, rid, cl[name],
                            c.windows[0])
            for name, preds in cl.items():  # the aggregate does not depend on the grid
                for agg in aggs:
                    assert device_aggregate(c, 0, c.nl, rid, preds, agg) == default[rid, name, agg]
    finally:
        assert L.stage_set_scan_tuning(c.tab.h, 0) == 0


def test_scan_is_ordered_on_the_callers_stream(wcase):
    """fills, the scan and the D2H copies on one caller stream and nothing else"""
    c = wcase
    s = stage.Stream()
    for rid in modes(c)[:2]:
        preds = classes(c, rid)["half"]
        check_where(c, device_where(c, 0, c.nl, rid, preds, stream=s), 0, c.nl, rid, preds)
        check_where(c, device_where(c, 0, c.nl, rid, preds, window=c.windows[0], stream=s), 0, c.nl, rid, preds,
                    c.windows[0])
        assert device_aggregate(c, 0, c.nl, rid, preds, PRIMARY, stream=s) == aggregate(expect(c, rid), c.key_pad,
                                                                                        preds, PRIMARY)


# ------------------------------------------------------------------------------------------
# the contract in its own words

def test_filtered_is_the_unfiltered_scan_indexed_by_the_mask(wcase):
    """on the same table and mode: the device's filtered outputs equal the device's unfiltered
    table_scan outputs indexed by the numpy mask over the unfiltered rows and status"""
    c = wcase
    for rid in modes(c):
        un = c.tab.table_scan(read_id=rid, row_meta=True)
        leaf_of = np.repeat(np.arange(c.nl), np.diff(un.offsets.astype(np.int64)))
        cl = classes(c, rid)
        for name in ("everything", "half", "not_half", "sparse", "four", "none", "nothing"):
            preds = cl[name]
            mask = un.status != stage.ST_NOT_FOUND
            for p in preds:
                x = column(un.records, c.key_pad, p.off, p.width, p.signed)
                t = np.int64 if p.signed else np.uint64
                mask &= ((x >= t(p.lo)) & (x <= t(p.hi))) != p.negate
            res = c.tab.table_scan_where(read_id=rid, preds=preds, row_meta=True, row_slot=True)
            assert res.count == int(mask.sum()), (c.name, rid, name)
            assert np.array_equal(res.records, un.records[mask]) and np.array_equal(res.meta, un.meta[mask])
            assert np.array_equal(res.status, un.status[mask])
            assert np.array_equal(res.slots >> np.uint64(16), leaf_of[mask].astype(np.uint64))
            assert np.array_equal(res.offsets[1:], np.cumsum(np.bincount(leaf_of[mask], minlength=c.nl)))
            for window in c.windows[:2]:
                w = c.tab.table_scan_where(read_id=rid, preds=preds, window=window, row_keys=True)
                uw = c.tab.table_scan(read_id=rid, window=window, row_keys=True)
                assert np.array_equal(w.records, uw.records[mask]) and np.array_equal(w.keys, uw.keys[mask])
            got = c.tab.table_scan_aggregate(read_id=rid, preds=preds, agg=PRIMARY)
            x = column(un.records, c.key_pad, *PRIMARY)[mask]
            assert got[0] == res.count and got[1] == sum(int(v) for v in x) % (1 << 64)
            if res.count:
                assert got[2:] == (int(x.min()), int(x.max()))


# ------------------------------------------------------------------------------------------
# the emit loop both families share: groups and leaves without a match, a cut between two groups

def group_matches(c, rid, mask):
    """-> [leaf, 64-slot group]: the group holds a match, from the oracle's (leaf, slot) numbers"""
    s = c.slots[rid][mask]
    g = np.zeros((c.nl, c.tab.leaf_capacity // 64), bool)
    g[(s >> np.uint64(16)).astype(np.int64), ((s & np.uint64(0xFFFF)) >> np.uint64(6)).astype(np.int64)] = True
    return g


def loop_paths(g):
    """-> (a leaf whose first matching group lies behind a group without a match, a leaf without a
    match between two leaves that have some, a leaf with matches in two or more groups); -1: none"""
    has = g.any(axis=1)
    some = np.nonzero(has)[0]
    late = np.nonzero(has & (g.argmax(axis=1) > 0))[0]
    empty = np.nonzero(~has[some[0]:some[-1]])[0] + some[0] if some.size else some
    two = np.nonzero(g.sum(axis=1) >= 2)[0]
    return tuple(int(x[0]) if x.size else -1 for x in (late, empty, two))


def loop_interval(c, rid):
    """an interval predicate on the primary column that takes every path of loop_paths: the k
    smallest values as make_classes' "sparse" does, else k consecutive values of the sorted column
    (the oracle's per-slot values), k as large as it can be"""
    e = expect(c, rid)
    off, width, signed = PRIMARY
    x, live = column(e.rows, c.key_pad, *PRIMARY), e.status != stage.ST_NOT_FOUND
    vals = np.sort(x[live])
    for k in range(min(vals.size, 8 * c.nl), 2, -1):  # as many matches as still leave a leaf without one
        for i in [0] + list(range(k, vals.size - k + 1, k)):
            if min(loop_paths(group_matches(c, rid, live & (x >= vals[i]) & (x <= vals[i + k - 1])))) >= 0:
                return [Pred(off, width, int(vals[i]), int(vals[i + k - 1]))]
    raise AssertionError((c.name, rid, "no interval of the primary column takes every path"))


@pytest.mark.parametrize("case", ["key8_large_leaves", "key16", "key32"], indirect=True)
def test_groups_and_leaves_without_a_match_and_a_cut_between_groups(wcase):
    """a predicate under which a leaf's first groups hold no match, a whole leaf between two
    matching ones holds none, and a leaf's matches span two groups -- asserted on the oracle --
    then rows and one window, raw and one snapshot mode, every optional output, whole and cut
    inside the leaf whose matches span two groups: the device's unfiltered scan indexed by the
    numpy mask, and nothing past the cut"""
    c = wcase
    assert c.tab.leaf_capacity >= 512, (c.name, c.tab.leaf_capacity)  # eight or more 64-slot groups per leaf
    window = c.windows[0]
    for rid in (None, c.rids[1]):
        preds = loop_interval(c, rid)
        f = filtered(c, rid, preds)
        g = group_matches(c, rid, f.mask)
        late, empty, two = loop_paths(g)
        what = (c.name, rid, preds)
        assert g.shape[1] >= 8 and g[late].any() and not g[late, 0], what
        assert not g[empty].any() and g[:empty].any() and g[empty + 1:].any(), what
        assert g[two].sum() >= 2, what
        # the cut: behind the matches of the leaf's first matching group, before those of its next
        in_group = (f.slots >> np.uint64(16) == two) & ((f.slots & np.uint64(0xFFFF)) >> np.uint64(6) == g[two].argmax())
        cut = int(f.offsets[two]) + int(in_group.sum())
        total = int(f.offsets[-1])
        assert f.offsets[two] < cut < f.offsets[two + 1] <= total, what

        rows = device_scan(c, 0, c.nl, rid)
        n = expect(c, rid).meta.size
        un = {"rows": rows["out"][:n * c.stride].reshape(n, c.stride), "meta": rows["meta"][:n * 8].view(np.uint64),
              "status": rows["status"][:n], "offsets": rows["offsets"][:(c.nl + 1) * 8].view(np.uint64)}
        mask = un["status"] != stage.ST_NOT_FOUND
        x = column(un["rows"], c.key_pad, *PRIMARY)
        mask &= (x >= np.uint64(preds[0].lo)) & (x <= np.uint64(preds[0].hi))
        assert np.array_equal(mask, f.mask), what
        leaf_of = np.repeat(np.arange(c.nl), np.diff(un["offsets"].astype(np.int64)))
        offsets = np.concatenate([[0], np.cumsum(np.bincount(leaf_of[mask], minlength=c.nl))]).astype(np.uint64)
        win = device_scan(c, 0, c.nl, rid, window=window)
        ws = win["width"]
        un["win"] = win["out"][:n * ws].reshape(n, ws)
        un["keys"] = win["keys"][:n * c.key_pad].reshape(n, c.key_pad)

        for m in (None, cut):
            k = total if m is None else m
            for w in (None, window):
                got = device_where(c, 0, c.nl, rid, preds, window=w, max_records=m, room=total)
                assert got["count"][:8].view(np.uint64)[0] == total and (got["count"][8:] == FILL).all(), (what, m, w)
                assert np.array_equal(got["offsets"][:(c.nl + 1) * 8].view(np.uint64), offsets), (what, m, w)
                assert (got["offsets"][(c.nl + 1) * 8:] == FILL).all(), (what, m, w)
                exp = {"out": un["rows" if w is None else "win"][mask][:k], "meta": un["meta"][mask][:k],
                       "status": un["status"][mask][:k], "slot": c.slots[rid][mask][:k]}
                if w is not None:
                    exp["keys"] = un["keys"][mask][:k]
                for name, want in exp.items():
                    nb = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
                    assert np.array_equal(got[name][:nb.size], nb), (what, m, w, name)
                    assert (got[name][nb.size:] == FILL).all(), (what, m, w, name)  # past the cut, and the guard
                assert np.array_equal(exp["slot"] >> np.uint64(16), leaf_of[mask][:k].astype(np.uint64)), (what, m, w)


# ------------------------------------------------------------------------------------------
# aggregates

def test_aggregates(wcase):
    c = wcase
    p = c.payload
    aggs = [None, PRIMARY, (0, 4, True), (p - 8, 8, False), (p - 8, 8, True), (p - 1, 1, True), (min(5, p - 3), 2, False)]
    for rid in modes(c):
        e = expect(c, rid)
        for name, preds in classes(c, rid).items():
            for agg in aggs:
                exp = aggregate(e, c.key_pad, preds, agg)
                assert device_aggregate(c, 0, c.nl, rid, preds, agg) == exp, (c.name, rid, name, agg)
                if agg and name in ("nothing", "inverted"):  # the identities: largest, smallest
                    assert exp == (0, 0, domain(agg[1], agg[2])[1], domain(agg[1], agg[2])[0])
        # an empty range: count 0 and the identities
        for a in (0, c.nl // 2, c.nl):
            assert device_aggregate(c, a, a, rid, [], (0, 2, True)) == (0, 0, 32767, -32768)
            assert device_aggregate(c, a, a, rid, [], (0, 8, False)) == (0, 0, (1 << 64) - 1, 0)
            assert device_aggregate(c, a, a, rid, [], None) == (0, 0, 0, 0)
        # the high-level form returns the same Python ints
        assert c.tab.table_scan_aggregate(read_id=rid, preds=classes(c, rid)["half"], agg=(p - 8, 8, True)) == \
            aggregate(e, c.key_pad, classes(c, rid)["half"], (p - 8, 8, True))
        assert c.tab.table_scan_aggregate(read_id=rid) == ((e.status != 0).sum(), 0, 0, 0)
    if c.name == "ycsb":  # a sum that wraps: random 8-byte unsigned values over 20 000 rows
        x = column(c.raw.rows, c.key_pad, 8, 8, False)
        assert sum(int(v) for v in x) >= 1 << 64
        assert device_aggregate(c, 0, c.nl, None, [], (8, 8, False)) == aggregate(c.raw, c.key_pad, [], (8, 8, False))


# ------------------------------------------------------------------------------------------
# right behind a device write epoch

def test_where_after_a_device_write_epoch(gpu):
    """update_batch_device, then the filtered scan and the aggregate on the same stream with no
    synchronisation between: the predicate is on the patched column and sees the epoch's new bytes"""
    n, m = 4000, 1500
    base = np.arange(n, dtype=np.uint64) * 4
    c = Case()
    c.name, c.key_width, c.windows = "epoch", 8, [(203, 24)]
    c.tab, c.orc = stage.Table(key_width=8), O.OracleTree()
    c.tab.load_keys(base, 8, mode=1)
    c.orc.load_keys(base, 8, 1)
    c.tab.sync()
    rng = np.random.default_rng(79)
    keys = rng.choice(base, m).astype(np.uint64)
    keys[rng.random(m) < 0.05] += 1  # absent
    off, dlen = c.windows[0]
    deltas = rng.integers(0, 256, (m, dlen), dtype=np.uint8)
    deltas[:, 3] = 0x5A  # the patched column's top byte: 0x5A in a patched row
    wid = (10 + 2 * np.arange(m)).astype(np.uint32)
    cid = (wid + 1).astype(np.uint32)
    cid[rng.random(m) < 0.1] = 0  # left in flight
    col = (off, 4, False)
    preds = [Pred(off, 4, 0x5A000000, 0x5AFFFFFF)]
    before = c.tab.table_scan_where(preds=preds).count
    d_cnt, d_agg = stage.DeviceBuffer(8), stage.DeviceBuffer(32)
    d_out = stage.DeviceBuffer(n * c.tab.stride)
    d_slot = stage.DeviceBuffer(n * 8)
    rc, ok = c.tab.update_batch_device(keys, off, deltas, wid, cid)
    c.tab.table_scan_where_device(None, None, preds, n, d_cnt, d_out=d_out, d_row_slot=d_slot)
    c.tab.table_scan_aggregate_device(None, None, preds, col, d_agg)
    stage.lib().stage_device_sync()
    exp = oracle_epoch(c.orc, keys, 8, off, deltas, wid, cid)
    assert (rc == exp).all() and ok == int((exp == stage.RC_OK).sum()) and ok > m // 2
    raw = raw_expect(c.orc)
    c.rids = (LAST, int(cid.max()) // 2, 5)
    c.raw, c.snap = raw, snapshot_expects(c.orc, raw, 8, c.rids)
    c.nl, c.key_pad, c.row, c.stride, c.payload = raw.leaves, 8, c.orc.row, c.tab.stride, c.orc.payload_size
    slots = raw_slots(c.orc)
    c.slots = {None: slots}
    c.slots.update({rid: snapshot_slots(raw, slots, 8) for rid in c.rids})
    c.filtered, c.classes = {}, {}
    f = filtered(c, None, preds)
    k = int(f.offsets[-1])
    assert k > before + m // 4  # the patched rows are what matches
    assert int(d_cnt.to_numpy(np.uint64, 1)[0]) == k
    rows = d_out.to_numpy(np.uint8, k * c.stride).reshape(k, c.stride)
    assert np.array_equal(rows[:, :c.row], f.rows)
    assert np.array_equal(d_slot.to_numpy(np.uint64, k), f.slots)
    w = d_agg.to_numpy(np.uint64, 4)
    assert tuple(int(x) for x in w) == aggregate(raw, 8, preds, col)
    # and the whole contract on the epoch's image
    for rid in modes(c):
        for pr in (preds, [Pred(off, 4, 0x5A000000, 0x5AFFFFFF, negate=True)]):
            check_where(c, device_where(c, 0, c.nl, rid, pr), 0, c.nl, rid, pr)
            check_where(c, device_where(c, 0, c.nl, rid, pr, window=c.windows[0]), 0, c.nl, rid, pr, c.windows[0])
            assert device_aggregate(c, 0, c.nl, rid, pr, col) == aggregate(expect(c, rid), 8, pr, col)
