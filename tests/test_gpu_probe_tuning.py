"""GPU: probe kernel instances that only a tuning knob or a batch size selects.

stage_set_probe_tuning / stage_set_probe_store pick probe_kernel's G = 1, 2, 4 and store policy
0 / 2 instances; the batch size picks probe_split_kernel's 4-, 16- and 64-probe wave chunks.  The
knobs and the chunk size are launch shapes, not semantics: every shape must write the bytes the
default does, and the default is held against the oracle.
"""
import numpy as np
import pytest

import oracle_lib as O
import stage
from stage._lib import check
from test_gpu_parity import check_probe
from test_wide_keys import tpcc_like

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 4, 8)
STORES = (0, 1, 2)


def set_shape(tab, group, store):
    check(stage.lib().stage_set_probe_tuning(tab.h, group, 0), "stage_set_probe_tuning")
    check(stage.lib().stage_set_probe_store(tab.h, store), "stage_set_probe_store")


@pytest.fixture(scope="module")
def versioned8(gpu):
    """8-byte keys, 64-slot leaves, 1000-byte rows over ~60 leaves; committed older versions,
    in-flight copies and deletes, so visibility()'s slow path runs"""
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
    for k in hot[:80]:  # in flight: readers see the copy or walk from its chain
        assert tab.update(int(k), 7, b"\xEE" * 50, cid) == orc.update(int(k), 8, 7, b"\xEE" * 50, cid)
    for k in hot[280:]:
        assert tab.delete(int(k), cid) == orc.delete(int(k), 8, cid)
    tab.sync()
    assert tab.leaf_capacity == 64 and tab.stride >= 1008 and tab.stats()["leaves"] > 8
    # 64 * 3 + 5 probes: more than one wave chunk, and the last group of every G is partial
    keys = np.concatenate([hot[:90], hot[:20], hot[270:], rng.integers(0, n, 40), rng.integers(n, 2 * n, 17)])
    keys = rng.permutation(keys).astype(np.uint64)
    assert keys.size == 64 * 3 + 5 and np.unique(keys).size < keys.size
    rids = rng.integers(0, cid + 4, keys.size).astype(np.uint32)
    return tab, orc, keys, rids


@pytest.mark.parametrize("count", [197, 1])
def test_knob_selected_probe_kernels_write_the_default_bytes(versioned8, count):
    tab, orc, keys, rids = versioned8
    keys, rids = keys[:count], rids[:count]
    try:
        set_shape(tab, 8, 1)
        out0, rows0 = check_probe(tab, orc, keys, 8, read_ids=rids)
        if count > 1:
            seen = set(np.unique(out0["status"]).tolist())
            assert {stage.ST_LATEST, stage.ST_COPY, stage.ST_OLD, stage.ST_NOT_FOUND} <= seen
        for group in GROUPS:
            for store in STORES:
                set_shape(tab, group, store)
                out, rows = tab.probe(keys, read_ids=rids)
                assert out.tobytes() == out0.tobytes(), (group, store)
                assert np.array_equal(rows, rows0), (group, store)
                out, rows = tab.probe(keys, read_ids=rids, records=False)  # recs == nullptr
                assert rows is None and out.tobytes() == out0.tobytes(), (group, store)
    finally:
        set_shape(tab, 8, 1)


def test_split_probe_chunk_sizes_agree(gpu):
    """probe_split_kernel's 4-, 16- and 64-probe wave chunks (batches below 65,521 probes, below
    1,048,513, and above: kSmallBelow) write the same status records and rows.  The 4-probe form
    is held against the oracle by test_wide_probe_and_scan."""
    keys = tpcc_like(16)
    rng = np.random.default_rng(5)
    tab = stage.Table(payload_size=40, key_width=16)
    rc, ins = tab.load_rows(keys, rng.integers(0, 256, (keys.shape[0], 40), dtype=np.uint8), commit_id=0)
    assert ins == keys.shape[0]
    tab.sync()
    assert tab.leaf_capacity > 256  # above the lane kernel's leaves: the split kernel
    n = 1_050_000
    probe = keys[rng.integers(0, keys.shape[0], n)]
    miss = rng.choice(n, 50_000, replace=False)
    probe[miss] = rng.integers(0, 256, (miss.size, 16), dtype=np.uint8)
    probe = np.ascontiguousarray(probe)
    parts = [tab.probe(probe[a:a + 20_000]) for a in range(0, n, 20_000)]  # 4-probe chunks
    out4 = np.concatenate([p[0] for p in parts])
    rows4 = np.concatenate([p[1] for p in parts])
    hits = np.count_nonzero(out4["status"] == stage.ST_LATEST)
    assert n - 50_000 <= hits < n and np.count_nonzero(out4["status"] == stage.ST_NOT_FOUND) == n - hits
    a = 140_000
    out16, rows16 = tab.probe(probe[a:a + 70_000])  # 16-probe chunks
    assert out16.tobytes() == out4[a:a + 70_000].tobytes()
    assert np.array_equal(rows16, rows4[a:a + 70_000])
    out64, rows64 = tab.probe(probe)  # 64-probe chunks
    assert out64.tobytes() == out4.tobytes()
    assert np.array_equal(rows64, rows4)
