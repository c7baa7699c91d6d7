"""GPU: column-window probes (stage_probe_batch_window / stage_probe_host_window,
Table.probe(..., window=(payload_off, len))).

The oracle is the judge: the expected window of a probe is bytes [key_pad + off, key_pad + off + len)
of the oracle's row (all zero when the read yields no tuple), the bytes past len up to
window_stride(len) are zero, and the status records equal the oracle's field by field (as
check_probe compares them) and stage_probe_batch's of the same batch byte for byte.

Every probe kernel family is covered: the fused probe_window_kernel (8-byte keys in 64-slot
leaves with 32- and 16-B status records, variable-length keys in 128-slot leaves) and the
status-only probe + window_gather_kernel composition (probe_lane_kernel and probe_split_kernel
tables)."""
import numpy as np
import pytest

import oracle_lib as O
import stage
from test_gpu_write_path import oracle_epoch
from test_wide_keys import build, tpcc_like

pytestmark = pytest.mark.gpu

STATUS_FIELDS = ("status", "hops", "cstamp", "rec_cstamp", "copy_sstamp")
YCSB_WINDOWS = [(0, 100), (100, 100), (3, 5), (999, 1), (896, 104), (0, 1000), (7, 50)]
YCSB_BATCHES = (0, 1, 63, 64, 65, 197)


def check_status(out, o_out):
    for f in STATUS_FIELDS:
        bad = np.nonzero(out[f] != o_out[f])[0]
        assert bad.size == 0, (f, bad[:5], out[f][bad[:5]], o_out[f][bad[:5]])
    assert ((out["flags"] & 1) == o_out["copy_present"]).all()


def check_window(win, o_rec, key_pad, window):
    """win against the oracle's rows: the window's bytes, then zero padding"""
    off, ln = window
    assert win.shape == (o_rec.shape[0], stage.window_stride(ln)) and win.shape[1] == (ln + 15) // 16 * 16
    exp = o_rec[:, key_pad + off:key_pad + off + ln]
    assert exp.shape[1] == ln
    bad = np.nonzero((win[:, :ln] != exp).any(axis=1))[0]
    assert bad.size == 0, (window, bad[:5], win[bad[:1], :ln], exp[bad[:1]])
    assert (win[:, ln:] == 0).all(), window


# ------------------------------------------------------------------------------------------
# 1. the YCSB geometry (probe_window_kernel<false, 1, 8, 32 / 16>)

@pytest.fixture(scope="module")
def ycsb(gpu):
    """The table of test_gpu_probe_tuning's versioned8 fixture (3000 rows of 1000 B in payload
    mode 1, committed chains of 1-2 versions, in-flight copies, deletes), built the same way.
    That recipe's old read ids end in FAIL_INVALID_TS (the loaded rows carry commit id 0), never in
    CHAIN_MISS, so 12 more rows are inserted at commit id 30: read below 30 they have no chain to
    walk.  Returns the table, the oracle, 197 keys and read ids, and per batch size the oracle's
    answer and stage_probe_batch's, computed once."""
    n = 3000
    tab = stage.Table(key_width=8)
    orc = O.OracleTree()
    tab.load_ycsb(0, n, 8, mode=1)
    orc.load_ycsb(0, n, 8, 1)
    rng = np.random.default_rng(21)
    hot = rng.choice(n, 300, replace=False)
    cid = 10
    for rnd in range(2):  # committed updates: version chains of length 1..2
        for k in hot[: 300 - 100 * rnd]:
            d = bytes([rnd * 17 + 3]) * 100
            assert tab.update(int(k), 100 * rnd, d, cid) == orc.update(int(k), 8, 100 * rnd, d, cid)
            assert tab.commit_update(int(k), cid + 1, cid + 1) == orc.commit_update(int(k), 8, cid + 1, cid + 1)
        cid += 5
    for k in hot[:80]:  # in flight: exactly window (7, 50)
        assert tab.update(int(k), 7, b"\xEE" * 50, cid) == orc.update(int(k), 8, 7, b"\xEE" * 50, cid)
    for k in hot[280:]:
        assert tab.delete(int(k), cid) == orc.delete(int(k), 8, cid)
    late = np.arange(n, n + 12, dtype=np.uint64)  # committed at 30, no older version
    for k in late:
        p = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
        assert tab.insert(int(k), 8, p, commit_id=30) == orc.insert(int(k), 8, p, 30) == stage.RC_OK
    tab.sync()
    assert tab.leaf_capacity == 64 and tab.stride >= 1008 and tab.stats()["leaves"] > 8
    keys = np.concatenate([hot[:90], hot[:20], hot[270:], rng.integers(0, n, 28), late, rng.integers(n, 2 * n, 17)])
    keys = rng.permutation(keys).astype(np.uint64)
    assert keys.size == 64 * 3 + 5 and np.unique(keys).size < keys.size
    rids = rng.integers(0, 34, keys.size).astype(np.uint32)
    ref = {}
    for b in YCSB_BATCHES:
        o_out, o_rec = orc.read_batch(keys[:b], 8, rids[:b])
        out, rows = tab.probe(keys[:b], read_ids=rids[:b])
        check_status(out, o_out)
        assert (rows[:, :orc.row] == o_rec).all()
        ref[b] = (o_out, o_rec, out, rows)
    seen = set(np.unique(ref[197][0]["status"]).tolist())
    assert seen >= {stage.ST_LATEST, stage.ST_COPY, stage.ST_OLD, stage.ST_NOT_FOUND, stage.ST_CHAIN_MISS,
                    stage.ST_FAIL_INVALID_TS}, seen
    return tab, orc, keys, rids, ref


@pytest.mark.parametrize("window", YCSB_WINDOWS)
def test_ycsb_windows(ycsb, window):
    tab, orc, keys, rids, ref = ycsb
    for b in YCSB_BATCHES:
        o_out, o_rec, out0, rows0 = ref[b]
        out, win = tab.probe(keys[:b], read_ids=rids[:b], window=window)
        assert out.dtype == out0.dtype and out.tobytes() == out0.tobytes(), (window, b)
        check_status(out, o_out)
        check_window(win, o_rec, 8, window)
        # the contract in its own words: the bytes the row form delivers
        assert np.array_equal(win[:, :window[1]], rows0[:, 8 + window[0]:8 + window[0] + window[1]])


def test_ycsb_windows_without_read_ids(ycsb):
    tab, orc, keys, _, _ = ycsb
    o_out, o_rec = orc.read_batch(keys, 8)
    out0, _ = tab.probe(keys, records=False)
    for window in ((100, 100), (7, 50)):
        out, win = tab.probe(keys, window=window)
        assert out.tobytes() == out0.tobytes()
        check_status(out, o_out)
        check_window(win, o_rec, 8, window)


def test_ycsb_windows_with_host_leaf_ids(ycsb):
    tab, orc, keys, rids, ref = ycsb
    leaf = tab.traverse(keys)
    for b in (65, 197):
        o_out, o_rec, out0, _ = ref[b]
        for window in ((100, 100), (999, 1), (0, 1000)):
            out, win = tab.probe(keys[:b], read_ids=rids[:b], leaf_ids=leaf[:b], window=window)
            assert out.tobytes() == out0.tobytes()
            check_window(win, o_rec, 8, window)


def test_ycsb_windows_with_lean_status_records(ycsb):
    tab, orc, keys, rids, ref = ycsb
    try:
        tab.set_output_layout(0, 16)
        for b in YCSB_BATCHES:
            o_out, o_rec, _, _ = ref[b]
            out0, _ = tab.probe(keys[:b], read_ids=rids[:b], records=False)
            assert out0.dtype == stage.PROBE_OUT16_DTYPE
            for window in ((100, 100), (3, 5), (0, 1000)):
                out, win = tab.probe(keys[:b], read_ids=rids[:b], window=window)
                assert out.dtype == stage.PROBE_OUT16_DTYPE and out.tobytes() == out0.tobytes(), (window, b)
                check_status(out, o_out)
                check_window(win, o_rec, 8, window)
    finally:
        tab.set_output_layout(0, 32)


def test_max_blocks_applies_to_the_window_probe(ycsb):
    """stage_set_probe_tuning's grid cap: one block strides over all four wave chunks"""
    tab, orc, keys, rids, ref = ycsb
    o_out, o_rec, out0, _ = ref[197]
    L = stage.lib()
    try:
        assert L.stage_set_probe_tuning(tab.h, 8, 1) == 0
        k4, r4 = np.tile(keys, 7), np.tile(rids, 7)  # 22 chunks over the block's 4 waves
        out, win = tab.probe(k4, read_ids=r4, window=(100, 100))
        assert out.tobytes() == np.tile(out0, 7).tobytes()
        check_window(win, np.tile(o_rec, (7, 1)), 8, (100, 100))
    finally:
        assert L.stage_set_probe_tuning(tab.h, 8, 0) == 0


# ------------------------------------------------------------------------------------------
# 2. images that exist only in HBM: after a device write epoch

def test_windows_after_a_device_write_epoch(gpu):
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
    probe = np.concatenate([keys, rng.choice(base, 500)]).astype(np.uint64)
    seen = set()
    for rid in (5, int(cid.max()) // 2, 0xFFFFFFFE):
        r = np.full(probe.size, rid, np.uint32)
        o_out, o_rec = orc.read_batch(probe, 8, r)
        out0, _ = tab.probe(probe, read_ids=r, records=False)
        seen |= set(np.unique(o_out["status"]).tolist())
        for window in ((off, dlen), (500, 64)):  # the epoch's column, and a disjoint one
            out, win = tab.probe(probe, read_ids=r, window=window)
            assert out.tobytes() == out0.tobytes()
            check_status(out, o_out)
            check_window(win, o_rec, 8, window)
    assert {stage.ST_LATEST, stage.ST_COPY, stage.ST_OLD} <= seen


# ------------------------------------------------------------------------------------------
# 3. the other kernel families

FAMILY_BATCHES = (1, 65, 20000)


def family_windows(payload):
    return [(0, 4), (4, 4), (1, 7), (payload - 1, 1), (0, payload)]


def add_versions(tab, orc, keys, width, payload, rng):
    """host write path: updates committed at 11 (300 rows) and 16 (200 of them), in-flight ones
    by writer 20 (100 of those): chains of 1-2 versions and overwrite copies"""
    pick = keys[rng.choice(keys.shape[0], 300, replace=False)]
    for i, k in enumerate(pick):
        for wid in (10, 15)[:2 if i < 200 else 1]:
            d = rng.integers(0, 256, 3, dtype=np.uint8).tobytes()
            assert tab.update_key(k.tobytes(), 2, d, wid) == orc.update(k.tobytes(), width, 2, d, wid)
            assert tab.commit_update_key(k.tobytes(), wid + 1, wid + 1) == \
                orc.commit_update(k.tobytes(), width, wid + 1, wid + 1)
        if i < 100:
            assert tab.update_key(k.tobytes(), payload - 2, b"\xEE\xEE", 20) == \
                orc.update(k.tobytes(), width, payload - 2, b"\xEE\xEE", 20)


def wide_family(width, payload, keys):
    """-> table, oracle, key pad, base key set (table keys + absent keys), oracle reader of it"""
    tab, orc, _ = build(width, payload, keys)
    rng = np.random.default_rng(width * 1000 + payload)
    add_versions(tab, orc, keys, width, payload, rng)
    base = np.concatenate([keys, rng.integers(0, 256, (400, width), dtype=np.uint8)])
    return tab, orc, (width + 7) // 8 * 8, base, lambda idx, rids: orc.read_batch_k(base[idx], rids)


def varlen_family():
    """variable-length decimal-string keys of 1..4 bytes (testing_btree.cpp's Insert keys)"""
    tab = stage.Table(payload_size=8, leaf_node_size=4096, split_threshold=3072, merge_threshold=1024, key_width=0)
    orc = O.OracleTree(4096, 3072, 8, 1024)
    rng = np.random.default_rng(8)
    words, lens = [], []
    for i in range(5000):
        k = str(i).encode()
        p = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
        if i < 4600:
            assert tab.insert(int.from_bytes(k, "little"), len(k), p, commit_id=5) == stage.RC_OK
            assert orc.insert(k, len(k), p, 5) == stage.RC_OK
        words.append(int.from_bytes(k, "little"))  # the last 400 are absent
        lens.append(len(k))
    base, blens = np.array(words, np.uint64), np.array(lens, np.uint16)

    def read(idx, rids):
        o_out = np.zeros(idx.size, O.READ_OUT_DTYPE)
        o_rec = np.zeros((idx.size, orc.row), np.uint8)
        uniq, inv = np.unique(idx, return_inverse=True)
        assert rids is None
        for j, u in enumerate(uniq):  # one oracle read per distinct key
            sel = inv == j
            o_out[sel], o_rec[sel] = orc.read(int(base[u]).to_bytes(8, "little")[:blens[u]], int(blens[u]))
        return o_out, o_rec

    return tab, orc, 8, (base, blens), read


FAMILIES = {
    # name: (builder, payload, leaf capacities that select the kernel, takes read ids)
    "varlen128": (varlen_family, 8, (128,), False),                         # probe_window_kernel<true, 2, 4, 32>
    "key8_large_leaves": (lambda: wide_family(8, 40, np.ascontiguousarray(  # probe_split_kernel, KW = 1
        np.random.default_rng(2).permutation(np.arange(5000, dtype=np.int64) * 3 + 1)).view(np.uint8).reshape(-1, 8)),
        40, (512, 1024), True),
    "key16_split": (lambda: wide_family(16, 40, tpcc_like(16, n_w=1)[:5000]), 40, (512, 1024), True),
    "key16_lane": (lambda: wide_family(16, 320, tpcc_like(16, n_w=1)[:5000]), 320, (64, 128, 256), True),
}


@pytest.fixture(scope="module", params=sorted(FAMILIES))
def family(gpu, request):
    builder, payload, caps, with_rids = FAMILIES[request.param]
    tab, orc, key_pad, base, read = builder()
    tab.sync()
    assert tab.leaf_capacity in caps, (request.param, tab.leaf_capacity)
    if request.param == "varlen128":
        assert tab.key_width == 0
    else:
        assert tab.key_words > 1 or tab.leaf_capacity > 128  # not probe_kernel's tables
    rng = np.random.default_rng(len(request.param))
    nbase = base[0].size if isinstance(base, tuple) else base.shape[0]
    idx = rng.integers(0, nbase, max(FAMILY_BATCHES))
    rids = rng.choice(np.array([5, 11, 13, 16, 20, 0xFFFFFFFE], np.uint32), idx.size) if with_rids else None
    o_out, o_rec = read(idx, rids)  # the oracle's answer, once
    if isinstance(base, tuple):
        args = dict(keys=base[0][idx], lens=base[1][idx])
    else:
        args = dict(keys=np.ascontiguousarray(base[idx]))
    found = set(np.unique(o_out["status"]).tolist())
    assert {stage.ST_LATEST, stage.ST_NOT_FOUND} <= found
    if with_rids:
        assert {stage.ST_COPY, stage.ST_OLD} <= found
    return tab, key_pad, payload, args, rids, o_out, o_rec


def test_family_windows(family):
    tab, key_pad, payload, args, rids, o_out, o_rec = family
    for b in FAMILY_BATCHES:
        a = {k: v[:b] for k, v in args.items()}
        r = None if rids is None else rids[:b]
        out0, rows0 = tab.probe(read_ids=r, **a)
        check_status(out0, o_out[:b])
        assert (rows0[:, :key_pad + payload] == o_rec[:b]).all()
        for window in family_windows(payload):
            out, win = tab.probe(read_ids=r, window=window, **a)
            assert out.tobytes() == out0.tobytes(), (window, b)
            check_window(win, o_rec[:b], key_pad, window)


# ------------------------------------------------------------------------------------------
# 4. the host form

def test_host_window_spans_pipeline_chunks(ycsb):
    tab, orc, keys197, _, _ = ycsb
    window = (100, 100)
    n = (1 << 17) + 100  # two chunks of the host pipeline
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 3400, n).astype(np.uint64)  # duplicates, and misses above 3011
    keys[:197] = keys197
    rids = rng.integers(0, 34, n).astype(np.uint32)
    ws = stage.window_stride(window[1])
    sample = rng.choice(n, 5000, replace=False)
    for r in (rids, None):
        out0, win0 = tab.probe(keys, read_ids=r, window=window)
        o_out, o_rec = orc.read_batch(keys[sample], 8, None if r is None else r[sample])
        check_status(out0[sample], o_out)
        check_window(win0[sample], o_rec, 8, window)
        for pinned in (True, False):
            if pinned:
                out, win = stage.pinned_empty(n, stage.PROBE_OUT_DTYPE), stage.pinned_empty((n, ws), np.uint8)
            else:
                out, win = np.empty(n, stage.PROBE_OUT_DTYPE), np.empty((n, ws), np.uint8)
            out.view(np.uint8)[:] = 0xAA
            win[:] = 0xAA
            got_out, got_win = tab.probe_host(keys, read_ids=r, out=out, rows=win, window=window)
            assert got_out is out and got_win is win
            assert out.tobytes() == out0.tobytes(), (pinned, r is None)
            assert np.array_equal(win, win0), (pinned, r is None)
    # the pipeline's buffers are left usable by the row form
    out, rows = tab.probe_host(keys[:1000], read_ids=rids[:1000])
    out0, rows0 = tab.probe(keys[:1000], read_ids=rids[:1000])
    assert out.tobytes() == out0.tobytes() and np.array_equal(rows, rows0)
    # a fresh-array call and an empty batch
    out, win = tab.probe_host(keys[:300], read_ids=rids[:300], window=(3, 5))
    o_out, o_rec = orc.read_batch(keys[:300], 8, rids[:300])
    check_status(out, o_out)
    check_window(win, o_rec, 8, (3, 5))
    out, win = tab.probe_host(keys[:0], window=window)
    assert out.size == 0 and win.shape == (0, ws)


# ------------------------------------------------------------------------------------------
# 5. stream order

def test_window_probe_is_ordered_on_the_callers_stream(ycsb, family):
    """probe_device_window on a caller stream, then a D2H on that stream and nothing else: the
    copy sees the finished windows (one launch on the YCSB table, two on a composed family)"""
    cases = [(ycsb[0], dict(keys=ycsb[2]), ycsb[3], (100, 100))]
    tab, key_pad, payload, args, rids, _, _ = family
    cases.append((tab, {k: v[:4000] for k, v in args.items()}, None if rids is None else rids[:4000], (1, 7)))
    for tab, args, rids, window in cases:
        out0, win0 = tab.probe(read_ids=rids, window=window, **args)
        s = stage.Stream()
        words, n = tab.key_buffer(args["keys"])
        d_keys = stage.DeviceBuffer.from_numpy(words, stream=s.ptr)
        d_rids = None if rids is None else stage.DeviceBuffer.from_numpy(rids, stream=s.ptr)
        d_lens = stage.DeviceBuffer.from_numpy(args["lens"], stream=s.ptr) if "lens" in args else None
        d_out = stage.DeviceBuffer(n * 32)
        d_win = stage.DeviceBuffer(n * win0.shape[1])
        d_out.memset(0xAA, stream=s.ptr)
        d_win.memset(0xAA, stream=s.ptr)
        tab.probe_device_window(d_keys.ptr, n, window, d_out.ptr, d_win.ptr, d_read_ids=d_rids and d_rids.ptr,
                                d_lens=d_lens and d_lens.ptr, stream=s.ptr)
        win = d_win.to_numpy(np.uint8, n * win0.shape[1], stream=s.ptr).reshape(win0.shape)
        out = d_out.to_numpy(stage.PROBE_OUT_DTYPE, n, stream=s.ptr)
        assert np.array_equal(win, win0) and out.tobytes() == out0.tobytes()
