"""GPU: whole-table scans (stage_table_scan / stage_table_scan_window, Table.table_scan).

The oracle is the judge (table_scan_expect.py).  Raw mode: the device's count, leaf offsets, meta
words and rows equal the parse of the oracle's reference-format leaf blocks, byte for byte and in
order.  Snapshot mode: the considered slots are raw mode's visible ones in the same order -- the
device's meta words and, where a record is produced, its key pin that -- and each slot's (status,
row) is the oracle's index_scan from the smallest key at the same read id, matched by key order.
The window form delivers the row form's bytes at key_pad + off, zero past len, and the rows' heads
as keys.  Every buffer is pre-filled with 0xA5 and carries a guard region: nothing at or past
max_records, or past the buffer's end, is written."""
import numpy as np
import pytest

import oracle_lib as O
import stage
from table_scan_expect import LAST, raw_expect, snapshot_expects
from test_gpu_probe_window import add_versions, varlen_family
from test_gpu_write_path import oracle_epoch
from test_wide_keys import build, tpcc_like

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256
END = stage.LEAF_END


# ------------------------------------------------------------------------------------------
# the tables

def one_leaf():
    tab, orc = stage.Table(key_width=8), O.OracleTree()
    rng = np.random.default_rng(1)
    for k in (7, 3, 5):
        p = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
        assert tab.insert(k, 8, p, commit_id=4) == orc.insert(k, 8, p, 4) == stage.RC_OK
    return tab, orc, (LAST, 2)


def ycsb_random():
    """20 000 rows of 1000 B loaded in random key order (splits, unsorted slot tails), then holes
    with meta 0 (delete, delete_key_owned), committed updates at 11 and 16 (chains of 1-2
    versions), one in-flight update (an overwrite copy) and one in-flight insert"""
    n = 20000
    rng = np.random.default_rng(31)
    keys = (rng.permutation(n).astype(np.uint64) * 3 + 1)
    tab, orc = stage.Table(key_width=8), O.OracleTree()
    assert tab.load_keys(keys, 8, mode=1) == orc.load_keys(keys, 8, 1) == n
    hot = rng.choice(keys, 400, replace=False)
    for i, k in enumerate(hot[:300]):
        for wid in (10, 15)[:2 if i < 200 else 1]:
            d = rng.integers(0, 256, 100, dtype=np.uint8).tobytes()
            assert tab.update(int(k), 100, d, wid) == orc.update(int(k), 8, 100, d, wid) == stage.RC_OK
            assert tab.commit_update(int(k), wid + 1, wid + 1) == orc.commit_update(int(k), 8, wid + 1, wid + 1)
    for k in hot[300:350]:
        assert tab.delete(int(k), 20) == orc.delete(int(k), 8, 20)
    for k in hot[350:]:
        kb = int(k).to_bytes(8, "little")
        assert tab.delete_key_owned(kb) == orc.delete_owned(kb, 8)
    k = int(hot[0])  # in flight on a twice-updated row
    assert tab.update(k, 7, b"\xEE" * 50, 25) == orc.update(k, 8, 7, b"\xEE" * 50, 25) == stage.RC_OK
    p = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    kb = (3 * 777).to_bytes(8, "little")  # absent: keys are 1 mod 3
    assert tab.insert_key_inflight(kb, p, 26) == orc.insert_inflight(kb, 8, p, 26) == stage.RC_OK
    return tab, orc, (LAST, 13, 2)


def varlen():
    tab, orc, _, _, _ = varlen_family()
    return tab, orc, (LAST, 2)


def key8_large_leaves():
    """8-byte keys, 8-byte payload, 32 KiB leaves: hundreds of records per leaf"""
    tab = stage.Table(payload_size=8, leaf_node_size=32768, split_threshold=8192, merge_threshold=16384, key_width=8)
    orc = O.OracleTree(32768, 8192, 8, 16384)
    rng = np.random.default_rng(12)
    keys = rng.permutation(np.arange(6000, dtype=np.uint64) * 5 + 2)
    pays = rng.integers(0, 256, (keys.size, 8), dtype=np.uint8)
    for k, p in zip(keys, pays):
        assert tab.insert(int(k), 8, p.tobytes(), commit_id=5) == orc.insert(int(k), 8, p.tobytes(), 5) == stage.RC_OK
    for k in keys[:120]:
        assert tab.delete(int(k), 9) == orc.delete(int(k), 8, 9)
    add_versions(tab, orc, np.ascontiguousarray(keys[200:2000]).view(np.uint8).reshape(-1, 8), 8, 8, rng)
    return tab, orc, (LAST, 13, 2)


def wide(width, payload):
    def make():
        keys = tpcc_like(width, n_w=1)[:5000]
        tab, orc, _ = build(width, payload, keys)
        rng = np.random.default_rng(width)
        add_versions(tab, orc, keys, width, payload, rng)
        for k in keys[rng.choice(keys.shape[0], 60, replace=False)]:
            assert tab.delete_key(k.tobytes(), 22) == orc.delete(k.tobytes(), width, 22)
        return tab, orc, (LAST, 13)
    return make


TABLES = {
    # name: (builder, key width, leaf capacities, windows)
    "one_leaf": (one_leaf, 8, (64,), [(100, 100), (0, 4)]),
    "ycsb": (ycsb_random, 8, (64,), [(100, 100), (0, 4), (999, 1), (0, 1000)]),
    "varlen128": (varlen, 0, (128,), [(0, 8), (3, 5)]),
    "key8_large_leaves": (key8_large_leaves, 8, (512, 1024), [(0, 8), (3, 5)]),
    "key16": (wide(16, 40), 16, (512, 1024), [(0, 4), (39, 1), (0, 40)]),
    "key32": (wide(32, 60), 32, (256, 512, 1024), [(1, 7), (59, 1)]),
}


class Case:
    pass


@pytest.fixture(scope="module", params=list(TABLES))
def case(gpu, request):
    """the table, published, and the oracle's expected records of every mode, computed once"""
    builder, key_width, caps, windows = TABLES[request.param]
    c = Case()
    c.name, c.windows, c.key_width = request.param, windows, key_width
    c.tab, c.orc, c.rids = builder()
    c.tab.sync()
    assert c.tab.leaf_capacity in caps, (c.name, c.tab.leaf_capacity)
    c.raw = raw_expect(c.orc, kwords=c.tab.key_words)
    c.snap = snapshot_expects(c.orc, c.raw, key_width, c.rids)
    c.nl = c.raw.leaves
    assert c.nl == c.tab.stats()["leaves"]
    c.key_pad, c.row, c.stride = c.tab.key_pad, c.orc.row, c.tab.stride
    if c.name == "one_leaf":
        assert c.nl == 1 and c.raw.counts[0] == 3
    else:
        assert c.nl >= 8
    if c.name == "ycsb":
        assert c.nl > 300 and (c.raw.meta == 0).sum() == 0 and c.raw.meta.size < 20001
        seen = set()
        for e in c.snap.values():
            seen |= set(np.unique(e.status).tolist())
        assert seen >= {stage.ST_LATEST, stage.ST_OLD, stage.ST_NOT_FOUND}, seen
    if c.name in ("varlen128", "key8_large_leaves"):
        assert c.raw.counts.max() > 64 and c.snap[LAST].counts.max() > 64  # a leaf crosses 64-rank chunks
    return c


def expect(c, rid):
    return c.raw if rid is None else c.snap[rid]


def modes(c):
    return [None] + list(c.rids)


# ------------------------------------------------------------------------------------------
# one device call into 0xA5-filled, guarded buffers

def device_scan(c, a, b, rid, window=None, max_records=None, offsets=True, meta=True, status=True, keys=True,
                room=None, stream=None):
    """-> dict of the raw output arrays (guards included); `room` = records the buffers hold"""
    e = expect(c, rid)
    nl = (c.nl if b == END else b) - a
    total = e.range(a, c.nl if b == END else b)[0]
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
    if keys and window is not None:
        bufs["keys"] = stage.DeviceBuffer(room * c.key_pad + GUARD)
    for buf in bufs.values():
        buf.memset(FILL, stream=sp)
    c.tab.table_scan_device((a, b), rid, m, bufs["count"], bufs.get("offsets"), bufs.get("out"), window,
                            bufs.get("keys"), bufs.get("meta"), bufs.get("status"), stream=sp)
    if not stream:
        stage.lib().stage_device_sync()
    got = {k: v.to_numpy(np.uint8, v.nbytes, stream=sp) for k, v in bufs.items()}
    got.update(width=width, room=room, m=m, nl=nl)
    return got


def check(c, got, a, b, rid, window=None, rows_of=None):
    """the raw arrays of device_scan against the oracle's records of leaves [a, b)"""
    e = expect(c, rid)
    b = c.nl if b == END else b
    total, offs, meta, status, rows = e.range(a, b)
    m, width, room = got["m"], got["width"], got["room"]
    k = min(total, m)
    what = (c.name, a, b, rid, window, m)
    cnt = got["count"]
    assert cnt[:8].view(np.uint64)[0] == total, what
    assert (cnt[8:] == FILL).all(), what
    if "offsets" in got:
        o = got["offsets"]
        assert np.array_equal(o[:(got["nl"] + 1) * 8].view(np.uint64), offs), what
        assert (o[(got["nl"] + 1) * 8:] == FILL).all(), what
    if "meta" in got:
        g = got["meta"]
        assert np.array_equal(g[:k * 8].view(np.uint64), meta[:k]), what
        assert (g[k * 8:] == FILL).all(), what
    if "status" in got:
        g = got["status"]
        assert np.array_equal(g[:k], status[:k]), what
        assert (g[k:] == FILL).all(), what
    if "out" not in got:
        return
    out = got["out"]
    assert (out[k * width:] == FILL).all(), what  # past max_records, and the guard
    out = out[:k * width].reshape(k, width)
    if window is None:
        bad = np.nonzero((out[:, :c.row] != rows[:k]).any(axis=1))[0]
        assert bad.size == 0, (what, bad[:5])
        gone = status[:k] == stage.ST_NOT_FOUND
        assert not out[gone].any(), what
    else:
        off, ln = window
        exp = rows[:k, c.key_pad + off:c.key_pad + off + ln]
        bad = np.nonzero((out[:, :ln] != exp).any(axis=1))[0]
        assert bad.size == 0, (what, bad[:5])
        assert not out[:, ln:].any(), what
        if rows_of is not None:  # the contract in its own words: the row form's bytes
            assert np.array_equal(out[:, :ln], rows_of[:k, c.key_pad + off:c.key_pad + off + ln]), what
        if "keys" in got:
            g = got["keys"]
            assert np.array_equal(g[:k * c.key_pad].reshape(k, c.key_pad), rows[:k, :c.key_pad]), what
            assert (g[k * c.key_pad:] == FILL).all(), what
            if rows_of is not None:
                assert np.array_equal(g[:k * c.key_pad].reshape(k, c.key_pad), rows_of[:k, :c.key_pad]), what
    return out


def some_ranges(c):
    k = min(c.nl // 2, max(c.nl - 3, 0))
    return [(0, 1), (k, min(k + 3, c.nl)), (c.nl - 1, c.nl)]


# ------------------------------------------------------------------------------------------
# rows

def test_whole_range_rows(case):
    c = case
    for rid in modes(c):
        got = device_scan(c, 0, c.nl, rid)
        check(c, got, 0, c.nl, rid)
        got = device_scan(c, 0, END, rid)  # through the last leaf
        check(c, got, 0, END, rid)


def test_snapshot_order_is_the_raw_order(case):
    """the snapshot's records are raw mode's visible slots, in raw mode's order: the same meta
    words, and the same key wherever a tuple is produced"""
    c = case
    raw = c.tab.table_scan(row_meta=True)
    assert raw.count == c.raw.meta.size and np.array_equal(raw.meta, c.raw.meta)
    vis = (raw.meta & np.uint64(1 << 62)) != 0
    if c.key_width:
        vis &= ((raw.meta >> np.uint64(48)) & np.uint64(0x2FFF)) == c.key_width
    for rid in c.rids:
        snap = c.tab.table_scan(read_id=rid, row_meta=True)
        assert snap.count == int(vis.sum())
        assert np.array_equal(snap.meta, raw.meta[vis])
        made = snap.status != stage.ST_NOT_FOUND
        assert np.array_equal(snap.records[made, :c.key_pad], raw.records[vis][made, :c.key_pad])
        assert np.array_equal(snap.offsets, c.snap[rid].offsets)


def test_sub_ranges_and_concatenation(case):
    c = case
    for rid in modes(c):
        for a, b in some_ranges(c) + [(0, 0), (c.nl // 2, c.nl // 2), (c.nl, c.nl)]:
            check(c, device_scan(c, a, b, rid), a, b, rid)
        check(c, device_scan(c, c.nl - 1, END, rid), c.nl - 1, END, rid)
        # consecutive ranges concatenate to the whole-range result
        cuts = sorted({0, 1, c.nl // 3, c.nl // 2, c.nl - 1, c.nl})
        parts = [c.tab.table_scan(leaves=(a, b), read_id=rid, row_meta=True) for a, b in zip(cuts[:-1], cuts[1:])]
        whole = c.tab.table_scan(read_id=rid, row_meta=True)
        assert sum(p.count for p in parts) == whole.count
        for f in ("records", "meta", "status"):
            assert np.array_equal(np.concatenate([getattr(p, f) for p in parts]), getattr(whole, f)), f
        assert np.array_equal(np.concatenate([p.offsets[:-1] + whole.offsets[a] for p, a in zip(parts, cuts)]),
                              whole.offsets[:-1])


def test_count_only_and_optional_outputs(case):
    c = case
    for rid in modes(c):
        for window in (None, c.windows[0]):
            got = device_scan(c, 0, c.nl, rid, window=window, max_records=0)  # null record buffer
            assert "out" not in got
            check(c, got, 0, c.nl, rid, window)
            got = device_scan(c, 0, END, rid, window=window, max_records=0, offsets=False, meta=False, status=False,
                              keys=False)
            assert set(got) == {"count", "width", "room", "m", "nl"}
            check(c, got, 0, END, rid, window)
            got = device_scan(c, 0, c.nl, rid, window=window, offsets=False, meta=False, status=False, keys=False)
            check(c, got, 0, c.nl, rid, window)


def test_truncation_leaves_the_rest_untouched(case):
    c = case
    for rid in modes(c):
        total = expect(c, rid).range(0, c.nl)[0]
        for m in sorted({max(total - 5, 1), 1}):
            for window in (None, c.windows[0]):
                got = device_scan(c, 0, c.nl, rid, window=window, max_records=m, room=total)
                check(c, got, 0, c.nl, rid, window)  # d_count is the total; bytes at and past m keep the fill
        # a caller whose output was cut resumes at the first leaf that was not delivered whole
        # (a cut on a leaf boundary: the first leaf whose offset is >= max_records)
        offs = expect(c, rid).offsets
        whole = c.tab.table_scan(read_id=rid)
        for m in sorted({int(offs[c.nl // 2]), int(offs[c.nl // 2]) + 1, 2}):
            first = c.tab.table_scan(read_id=rid, max_records=m)
            assert first.count == whole.count and first.records.shape[0] == min(m, whole.count)
            assert np.array_equal(first.offsets, whole.offsets)
            nxt = int(np.nonzero(first.offsets[1:] > m)[0][0]) if m < whole.count else c.nl
            if nxt < c.nl:
                assert first.offsets[nxt] <= m < first.offsets[nxt + 1]  # the leaf the cut fell into
            rest = c.tab.table_scan(leaves=(nxt, END), read_id=rid)
            keep = int(first.offsets[nxt])
            assert np.array_equal(np.concatenate([first.records[:keep], rest.records]), whole.records)


# ------------------------------------------------------------------------------------------
# windows

def test_windows(case):
    c = case
    for rid in modes(c):
        rows_of = c.tab.table_scan(read_id=rid).records
        for window in c.windows:
            check(c, device_scan(c, 0, c.nl, rid, window=window), 0, c.nl, rid, window, rows_of)
            a, b = some_ranges(c)[1]
            lo = int(expect(c, rid).offsets[a])
            check(c, device_scan(c, a, b, rid, window=window, keys=False), a, b, rid, window, rows_of[lo:])
        res = c.tab.table_scan(read_id=rid, window=c.windows[-1], row_keys=True, row_meta=True)
        off, ln = c.windows[-1]
        assert res.records.shape == (res.count, stage.window_stride(ln))
        assert np.array_equal(res.records[:, :ln], rows_of[:, c.key_pad + off:c.key_pad + off + ln])
        assert np.array_equal(res.keys, rows_of[:, :c.key_pad])


# ------------------------------------------------------------------------------------------
# the grid cap, a caller's stream, a device write epoch

def test_one_block_grid_strides_over_the_leaves(case):
    c = case
    L = stage.lib()
    try:
        assert L.stage_set_scan_tuning(c.tab.h, 1) == 0
        for rid in modes(c)[:2]:
            check(c, device_scan(c, 0, c.nl, rid), 0, c.nl, rid)
            check(c, device_scan(c, 0, END, rid, window=c.windows[0]), 0, END, rid, c.windows[0])
    finally:
        assert L.stage_set_scan_tuning(c.tab.h, 0) == 0


def test_scan_is_ordered_on_the_callers_stream(case):
    """fills, the scan and the D2H copies on one caller stream and nothing else"""
    c = case
    s = stage.Stream()
    for rid in modes(c)[:2]:
        check(c, device_scan(c, 0, c.nl, rid, stream=s), 0, c.nl, rid)
        check(c, device_scan(c, 0, c.nl, rid, window=c.windows[0], stream=s), 0, c.nl, rid, c.windows[0])


def test_scan_after_a_device_write_epoch(gpu):
    """update_batch_device, then the scan on the same stream with no synchronisation between: the
    rows are the epoch's new bytes"""
    n, m = 4000, 1500
    base = np.arange(n, dtype=np.uint64) * 4
    c = Case()
    c.name, c.key_width, c.windows = "epoch", 8, [(203, 24)]
    c.tab, c.orc = stage.Table(key_width=8), O.OracleTree()
    c.tab.load_keys(base, 8, mode=1)
    c.orc.load_keys(base, 8, 1)
    c.tab.sync()
    rng = np.random.default_rng(78)
    keys = rng.choice(base, m).astype(np.uint64)
    keys[rng.random(m) < 0.05] += 1  # absent
    off, dlen = c.windows[0]
    deltas = rng.integers(0, 256, (m, dlen), dtype=np.uint8)
    wid = (10 + 2 * np.arange(m)).astype(np.uint32)
    cid = (wid + 1).astype(np.uint32)
    cid[rng.random(m) < 0.1] = 0  # left in flight
    before = c.tab.table_scan().records
    # the epoch and the scan: both on the table's stream, the scan enqueued right behind the epoch
    d_cnt = stage.DeviceBuffer(8)
    d_out = stage.DeviceBuffer(n * c.tab.stride)
    d_win = stage.DeviceBuffer(n * stage.window_stride(dlen))
    rc, ok = c.tab.update_batch_device(keys, off, deltas, wid, cid)
    c.tab.table_scan_device(None, None, n, d_cnt, d_out=d_out)
    c.tab.table_scan_device(None, None, n, d_cnt, d_out=d_win, window=c.windows[0])
    stage.lib().stage_device_sync()
    exp = oracle_epoch(c.orc, keys, 8, off, deltas, wid, cid)
    assert (rc == exp).all() and ok == int((exp == stage.RC_OK).sum()) and ok > m // 2
    raw = raw_expect(c.orc)
    assert int(d_cnt.to_numpy(np.uint64, 1)[0]) == n == raw.meta.size
    rows = d_out.to_numpy(np.uint8, n * c.tab.stride).reshape(n, c.tab.stride)
    assert np.array_equal(rows[:, :c.orc.row], raw.rows)
    assert (rows != before).any()
    win = d_win.to_numpy(np.uint8, n * 32).reshape(n, 32)
    assert np.array_equal(win[:, :dlen], raw.rows[:, 8 + off:8 + off + dlen]) and not win[:, dlen:].any()
    # and the whole contract on the epoch's image
    c.rids = (LAST, int(cid.max()) // 2, 5)
    c.raw, c.snap = raw, snapshot_expects(c.orc, raw, 8, c.rids)
    c.nl, c.key_pad, c.row, c.stride = raw.leaves, 8, c.orc.row, c.tab.stride
    for rid in modes(c):
        check(c, device_scan(c, 0, c.nl, rid), 0, c.nl, rid)
        check(c, device_scan(c, 0, c.nl, rid, window=c.windows[0]), 0, c.nl, rid, c.windows[0])
