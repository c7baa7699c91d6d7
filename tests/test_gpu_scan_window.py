"""GPU: column-window range scans (stage_scan_batch_window / stage_index_scan_batch_window,
Table.range_scan / Table.index_scan(..., window=(payload_off, len), row_keys=...)).

The oracle is the judge: the expected window of scanned record j is bytes
[key_pad + off, key_pad + off + len) of the oracle's row j, the bytes past len up to
window_stride(len) are zero, counts and per-record statuses equal the oracle's, and the windows
equal the same slice of the rows Table.range_scan / Table.index_scan deliver for the same call.
Positions at and past a scan's count are never written.

Both kernel forms run: the direct one (scan_window_kernel: keys of <= 8 bytes in 64- / 128-slot
leaves at any size, every table above 63 records) and the compact one
(scan_window_kernel_compact: wide keys and large leaves up to 63 records), each with and without
per-record visibility."""
import numpy as np
import pytest

import oracle_lib as O
import stage
from test_gpu_probe_window import FAMILIES, YCSB_WINDOWS, family_windows, ycsb  # noqa: F401  (ycsb: fixture)
from test_gpu_write_path import oracle_epoch

pytestmark = pytest.mark.gpu

YCSB_SIZES = (1, 2, 63, 64, 65, 100, 300)
FAMILY_SIZES = (1, 10, 63, 64, 100)
LAST = 0xFFFFFFFE


def oracle_index_scans(orc, starts, key_size, size, rids):
    """orc.index_scan per start -> counts[n], rows[n, size, row] (zero past the count), status[n, size]"""
    n = len(starts)
    counts = np.zeros(n, np.uint32)
    rows = np.zeros((n, size, orc.row), np.uint8)
    st = np.zeros((n, size), np.uint8)
    for i in range(n):
        k = starts[i].tobytes() if isinstance(starts[i], np.ndarray) else int(starts[i])
        c, r, s = orc.index_scan(k, key_size, size, int(rids[i]))
        counts[i], rows[i, :c], st[i, :c] = c, r, s
    return counts, rows, st


def check_scan(got, o_counts, o_rows, key_pad, window, rows0=None, fill=0):
    """(counts, win[, keys]) of a window scan against the oracle's counts and rows (and the row
    form's rows): window bytes, zero padding, keys; positions >= count hold `fill`"""
    counts, win = got[0], got[1]
    off, ln = window
    n, size = o_rows.shape[:2]
    assert np.array_equal(counts, o_counts), (window, np.nonzero(counts != o_counts)[0][:5])
    assert win.shape == (n, size, stage.window_stride(ln)) and win.shape[2] == (ln + 15) // 16 * 16
    live = np.arange(size)[None, :] < o_counts[:, None]
    exp = o_rows[:, :, key_pad + off:key_pad + off + ln]
    assert exp.shape[2] == ln
    bad = np.argwhere(live & (win[:, :, :ln] != exp).any(axis=2))
    assert bad.size == 0, (window, size, bad[:5])
    assert (win[:, :, ln:][live] == 0).all(), (window, size)
    assert (win[~live] == fill).all(), (window, size)
    if rows0 is not None:  # the contract in its own words: the bytes the row form delivers
        assert np.array_equal(win[:, :, :ln][live], rows0[:, :, key_pad + off:key_pad + off + ln][live])
    if len(got) > 2 and got[2].ndim == 3 and got[2].shape[2] == key_pad:
        keys = got[2]
        assert keys.shape == (n, size, key_pad)
        assert np.array_equal(keys[live], o_rows[:, :, :key_pad][live]), (window, size)
        assert (keys[~live] == fill).all()
        if rows0 is not None:
            assert np.array_equal(keys[live], rows0[:, :, :key_pad][live])


# ------------------------------------------------------------------------------------------
# 1. / 2. the YCSB geometry (scan_window_kernel<false, 1, 1, VIS>)

@pytest.fixture(scope="module")
def ycsb_scans(ycsb):
    """~260 start keys over the ycsb table (3012 keys: 0 .. 3011): present, deleted and absent
    ones, 0, the last key, keys past the end, and a run near the end whose scans come up short;
    per scan size the oracle's answer and the row forms', computed once and left unchanged."""
    tab, orc, keys197, _, _ = ycsb
    rng = np.random.default_rng(5)
    edge = np.array([0, 3011, 3012, 4000, 1 << 63, (1 << 64) - 1], np.uint64)
    starts = rng.permutation(np.concatenate([keys197, edge, np.arange(2955, 3012, dtype=np.uint64)]))
    assert starts.dtype == np.uint64
    assert 255 <= starts.size <= 265
    rids = rng.integers(0, 34, starts.size).astype(np.uint32)
    rids[rng.random(starts.size) < 0.2] = LAST
    ref = {}
    seen = set()
    for size in YCSB_SIZES:
        oc, orows = orc.scan_batch(starts, 8, size)
        c0, rows0 = tab.range_scan(starts, size)
        assert np.array_equal(c0, oc) and np.array_equal(rows0[:, :, :orc.row], orows)
        ic, irows, ist = oracle_index_scans(orc, starts, 8, size, rids)
        c1, rows1, st1 = tab.index_scan(starts, size, read_ids=rids)
        assert np.array_equal(c1, ic) and np.array_equal(st1, ist) and np.array_equal(rows1[:, :, :orc.row], irows)
        live = np.arange(size)[None, :] < ic[:, None]
        seen |= set(np.unique(ist[live]).tolist())
        ref[size] = (oc, orows, rows0, ic, irows, ist, rows1)
    assert seen >= {stage.ST_LATEST, stage.ST_OLD, stage.ST_NOT_FOUND}, seen
    assert (ref[100][0] < 100).any() and (ref[100][0] == 100).any() and (ref[300][0] == 0).any()
    return tab, starts, rids, ref


@pytest.mark.parametrize("size", YCSB_SIZES)
def test_ycsb_scan_windows(ycsb_scans, size):
    tab, starts, _, ref = ycsb_scans
    oc, orows, rows0 = ref[size][:3]
    for window in YCSB_WINDOWS:
        check_scan(tab.range_scan(starts, size, window=window, row_keys=True), oc, orows, 8, window, rows0)
    for b in (0, 1, 5):  # the empty launch, one wave, fewer scans than a block's waves
        for window in ((100, 100), (0, 1000), (3, 5)):
            got = tab.range_scan(starts[:b], size, window=window, row_keys=b != 1)
            assert len(got) == (3 if b != 1 else 2)
            check_scan(got, oc[:b], orows[:b], 8, window, rows0[:b])


@pytest.mark.parametrize("size", YCSB_SIZES)
def test_ycsb_index_scan_windows(ycsb_scans, size):
    tab, starts, rids, ref = ycsb_scans
    ic, irows, ist, rows1 = ref[size][3:]
    live = np.arange(size)[None, :] < ic[:, None]
    for window in YCSB_WINDOWS:
        counts, win, keys, st = tab.index_scan(starts, size, read_ids=rids, window=window, row_keys=True)
        assert np.array_equal(st, ist)  # zero past the count, as the row form's
        check_scan((counts, win, keys), ic, irows, 8, window, rows1)
        gone = live & (ist == stage.ST_NOT_FOUND)
        assert (win[gone] == 0).all() and (keys[gone] == 0).all()
    for b in (0, 1, 5):
        counts, win, st = tab.index_scan(starts[:b], size, read_ids=rids[:b], window=(7, 50))
        assert np.array_equal(st, ist[:b])
        check_scan((counts, win), ic[:b], irows[:b], 8, (7, 50), rows1[:b])
    # no read ids: every record's latest image
    oc, orows, _ = ref[size][:3]
    counts, win, st = tab.index_scan(starts, size, window=(100, 100))
    c2, rows2, st2 = tab.index_scan(starts, size)
    assert np.array_equal(counts, c2) and np.array_equal(st, st2)
    check_scan((counts, win), c2, rows2, 8, (100, 100))


def test_empty_scans_are_a_no_op(ycsb_scans):
    tab, starts, rids, _ = ycsb_scans
    counts, win, keys = tab.range_scan(starts[:9], 0, window=(0, 4), row_keys=True)
    assert (counts == 0).all() and win.shape == (9, 0, 16) and keys.shape == (9, 0, 8)
    counts, win, st = tab.index_scan(starts[:9], 0, read_ids=rids[:9], window=(0, 4))
    assert (counts == 0).all() and win.size == 0 and st.size == 0


# ------------------------------------------------------------------------------------------
# 3. unwritten positions, stream order

@pytest.mark.parametrize("index", [False, True])
def test_unwritten_positions_and_stream_order(ycsb_scans, index):
    """scan_device_window into buffers pre-filled with 0xAA: positions >= count keep the fill,
    written ones have zero padding; then the same on a caller stream followed by D2H copies on
    that stream and nothing else -- the copies see the finished scan"""
    tab, starts, rids, ref = ycsb_scans
    size, window = 100, (100, 100)
    oc, orows = (ref[size][3], ref[size][4]) if index else (ref[size][0], ref[size][1])
    ws, n = stage.window_stride(window[1]), starts.size
    for own_stream in (False, True):
        s = stage.Stream() if own_stream else None
        sp = s.ptr if s else None
        d_keys = stage.DeviceBuffer.from_numpy(starts, stream=sp)
        d_rids = stage.DeviceBuffer.from_numpy(rids, stream=sp)
        d_cnt, d_win = stage.DeviceBuffer(n * 4), stage.DeviceBuffer(n * size * ws)
        d_key, d_st = stage.DeviceBuffer(n * size * 8), stage.DeviceBuffer(n * size)
        for b in (d_cnt, d_win, d_key, d_st):
            b.memset(0xAA, stream=sp)
        tab.scan_device_window(d_keys.ptr, n, size, window, d_cnt.ptr, d_win.ptr, d_row_keys=d_key.ptr,
                               d_row_status=d_st.ptr if index else None, d_read_ids=d_rids.ptr if index else None,
                               stream=sp)
        if not own_stream:
            stage.lib().stage_device_sync()
        win = d_win.to_numpy(np.uint8, n * size * ws, stream=sp).reshape(n, size, ws)
        keys = d_key.to_numpy(np.uint8, n * size * 8, stream=sp).reshape(n, size, 8)
        counts = d_cnt.to_numpy(np.uint32, n, stream=sp)
        st = d_st.to_numpy(np.uint8, n * size, stream=sp).reshape(n, size)
        check_scan((counts, win, keys), oc, orows, 8, window, fill=0xAA)
        live = np.arange(size)[None, :] < oc[:, None]
        assert (~live).any()
        if index:
            assert np.array_equal(st[live], ref[size][5][live]) and (st[~live] == 0xAA).all()
        else:
            assert (st == 0xAA).all()
        # without the optional keys nothing else changes
        d_win.memset(0xAA, stream=sp)
        tab.scan_device_window(d_keys.ptr, n, size, window, d_cnt.ptr, d_win.ptr,
                               d_row_status=d_st.ptr if index else None, d_read_ids=d_rids.ptr if index else None,
                               stream=sp)
        if not own_stream:
            stage.lib().stage_device_sync()
        win2 = d_win.to_numpy(np.uint8, n * size * ws, stream=sp).reshape(n, size, ws)
        assert np.array_equal(win2, win)


# ------------------------------------------------------------------------------------------
# 4. images that exist only in HBM: after a device write epoch

def test_scan_windows_after_a_device_write_epoch(gpu):
    n, m = 4000, 1500
    base = np.arange(n, dtype=np.uint64) * 4
    tab = stage.Table(key_width=8)
    orc = O.OracleTree()
    tab.load_keys(base, 8, mode=1)
    orc.load_keys(base, 8, 1)
    tab.sync()
    rng = np.random.default_rng(77)
    keys = rng.choice(base, m).astype(np.uint64)  # repeats: chains inside the epoch
    keys[rng.random(m) < 0.05] += 1               # absent
    off, dlen = 203, 24
    deltas = rng.integers(0, 256, (m, dlen), dtype=np.uint8)
    wid = (10 + 2 * np.arange(m)).astype(np.uint32)
    cid = (wid + 1).astype(np.uint32)
    cid[rng.random(m) < 0.1] = 0  # left in flight
    rc, ok = tab.update_batch_device(keys, off, deltas, wid, cid)
    exp = oracle_epoch(orc, keys, 8, off, deltas, wid, cid)
    assert (rc == exp).all() and ok == int((exp == stage.RC_OK).sum()) and ok > m // 2
    starts = np.concatenate([keys[:100], rng.choice(base, 40), np.array([0, 4 * n - 4, 4 * n], np.uint64)])
    assert starts.dtype == np.uint64
    windows = ((off, dlen), (500, 64))  # the epoch's column, and a disjoint one
    seen = set()
    for size in (10, 100):
        oc, orows = orc.scan_batch(starts, 8, size)
        c0, rows0 = tab.range_scan(starts, size)
        for window in windows:
            check_scan(tab.range_scan(starts, size, window=window, row_keys=True), oc, orows, 8, window, rows0)
        for rid in (5, int(cid.max()) // 2, LAST):  # below, inside and above the epoch's commit ids
            r = np.full(starts.size, rid, np.uint32)
            ic, irows, ist = oracle_index_scans(orc, starts, 8, size, r)
            c1, rows1, st1 = tab.index_scan(starts, size, read_ids=r)
            seen |= set(np.unique(ist).tolist())
            for window in windows:
                counts, win, keys_, st = tab.index_scan(starts, size, read_ids=r, window=window, row_keys=True)
                assert np.array_equal(st, ist) and np.array_equal(st, st1)
                check_scan((counts, win, keys_), ic, irows, 8, window, rows1)
    assert {stage.ST_LATEST, stage.ST_OLD} <= seen


# ------------------------------------------------------------------------------------------
# 5. the other families: variable-length keys in 128-slot leaves, 8-byte keys in large leaves,
#    wide keys in large and in small leaves

@pytest.fixture(scope="module", params=sorted(FAMILIES))
def scan_family(gpu, request):
    builder, payload, caps, with_rids = FAMILIES[request.param]
    tab, orc, key_pad, base, _ = builder()
    tab.sync()
    assert tab.leaf_capacity in caps, (request.param, tab.leaf_capacity)
    rng = np.random.default_rng(len(request.param) + 40)
    if request.param == "varlen128":
        words, lens = base
        # leaves are in key order and every record is visible: leaf L's first key is record
        # sum(rc[:L]) of the whole table in key order ("0" is the smallest key)
        rcnt = tab.export_leaves()[0]
        total, allrows = orc.scan(b"0", 1, 5000)
        assert total == int(rcnt.sum()) == 4600
        big = np.nonzero(rcnt > 64)[0]
        assert big.size > 0, "no 128-slot leaf holds more than 64 records"
        first = allrows[np.cumsum(rcnt)[big[:4]] - rcnt[big[:4]], :8]
        f_lens = (first != 0).sum(axis=1).astype(np.uint16)
        idx = rng.integers(0, words.size, 120)
        starts = np.concatenate([words[idx], np.ascontiguousarray(first).view(np.uint64).reshape(-1)])
        lens = np.concatenate([lens[idx], f_lens]).astype(np.uint16)
        # a 100-record scan from such a key emits min(records of the leaf, 100) > 64 records in
        # its first leaf visit
        long_visit = np.arange(120, starts.size)
        args = dict(start_keys=starts, lens=lens)
    else:
        idx = rng.integers(0, base.shape[0], 120)
        srt = base[:5000][np.lexsort(base[:5000].T[::-1])]  # the table's keys in memcmp order
        starts = np.concatenate([base[idx], srt[:1], srt[-1:], srt[-40:-38]])
        # every key is a visible record and leaves are in key order (keys of 8 bytes order by signed
        # bytes, wider ones by unsigned bytes), so leaf L holds records [sum(rcnt[:L]), sum(rcnt[:L + 1]))
        # of the table in key order.  A 100-record scan from the first key of a leaf of more than
        # 64 records emits min(records of the leaf, 100) > 64 records in its first leaf visit: two
        # store_windows chunks from the LDS list.
        tord = base[:5000][np.lexsort((base[:5000].view(np.int8) if base.shape[1] == 8 else base[:5000]).T[::-1])]
        rcnt, _, _, keyw = tab.export_leaves()
        assert int(rcnt.sum()) == tord.shape[0]
        big = np.nonzero(rcnt > 64)[0]
        assert big.size > 0, f"{request.param}: no leaf holds more than 64 records, the largest holds {rcnt.max()}"
        lo = (np.cumsum(rcnt) - rcnt)[big[:4]]
        for L, p in zip(big[:4], lo):  # the leaf's records are those keys (their first 8 bytes)
            head = np.ascontiguousarray(tord[p:p + rcnt[L], :8]).view(np.uint64).reshape(-1)
            assert np.array_equal(np.sort(keyw[L, :rcnt[L]]), np.sort(head)), (request.param, L)
        first = tord[lo]
        long_visit = np.arange(starts.shape[0], starts.shape[0] + first.shape[0])
        starts = np.ascontiguousarray(np.concatenate([starts, first]))
        args = dict(start_keys=starts)
    rids = None
    if with_rids:  # the long-visit starts' read ids are drawn after the others'
        pool, n0 = np.array([5, 11, 13, 16, 20, LAST], np.uint32), len(starts) - long_visit.size
        rids = np.concatenate([rng.choice(pool, n0), rng.choice(pool, long_visit.size)])
    return request.param, tab, orc, key_pad, payload, args, rids, long_visit


def test_family_scan_windows(scan_family):
    name, tab, orc, key_pad, payload, args, rids, long_visit = scan_family
    starts = args["start_keys"]
    seen = set()
    short = False  # some scan ends before its size: the end of the table
    for size in FAMILY_SIZES:
        if name == "varlen128":  # the oracle's scan per start
            oc = np.zeros(starts.size, np.uint32)
            orows = np.zeros((starts.size, size, orc.row), np.uint8)
            for i in range(starts.size):
                ln = int(args["lens"][i])
                c, r = orc.scan(int(starts[i]).to_bytes(8, "little")[:ln], ln, size)
                oc[i], orows[i, :c] = c, r
        else:
            oc, orows = orc.scan_batch_k(starts, size)
        if size == 100:
            assert (oc[long_visit] > 64).all(), (name, oc[long_visit])
        c0, rows0 = tab.range_scan(scan_size=size, **args)
        assert np.array_equal(c0, oc)
        assert (oc == size).any()
        short = short or bool((oc < size).any())
        for window in family_windows(payload):
            got = tab.range_scan(scan_size=size, window=window, row_keys=True, **args)
            check_scan(got, oc, orows, key_pad, window, rows0)
        if rids is None:
            continue
        ic, irows, ist = oracle_index_scans(orc, starts, starts.shape[1], size, rids)
        c1, rows1, st1 = tab.index_scan(scan_size=size, read_ids=rids, **args)
        seen |= set(np.unique(ist).tolist())
        for window in family_windows(payload):
            counts, win, keys, st = tab.index_scan(scan_size=size, read_ids=rids, window=window, row_keys=True, **args)
            assert np.array_equal(st, ist) and np.array_equal(st, st1)
            check_scan((counts, win, keys), ic, irows, key_pad, window, rows1)
    assert short or name == "varlen128"
    if rids is not None:
        assert {stage.ST_LATEST, stage.ST_OLD} <= seen


# ------------------------------------------------------------------------------------------
# 6. the grid cap

def test_max_blocks_applies_to_the_window_scan(ycsb_scans):
    """stage_set_scan_tuning's grid cap: one block's four waves stride over ~260 scans"""
    tab, starts, rids, ref = ycsb_scans
    oc, orows, rows0, ic, irows, ist, rows1 = ref[65]
    L = stage.lib()
    try:
        assert L.stage_set_scan_tuning(tab.h, 1) == 0
        check_scan(tab.range_scan(starts, 65, window=(100, 100), row_keys=True), oc, orows, 8, (100, 100), rows0)
        counts, win, st = tab.index_scan(starts, 65, read_ids=rids, window=(3, 5))
        assert np.array_equal(st, ist)
        check_scan((counts, win), ic, irows, 8, (3, 5), rows1)
        c0, r0 = tab.range_scan(starts, 65)  # the row form under the same cap
        assert np.array_equal(c0, oc) and np.array_equal(r0, rows0)
    finally:
        assert L.stage_set_scan_tuning(tab.h, 0) == 0
