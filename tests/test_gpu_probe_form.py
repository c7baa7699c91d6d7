"""GPU: the point probe's lane-per-probe form (stage_set_probe_form, probe_rows_kernel).

A launch shape, not a semantic: the LANE form is held against the oracle (check_probe) and must
write, byte for byte, what the WAVE form (probe_kernel) writes -- status records and rows, with
and without rows, with caller-supplied leaf ids, in both status sizes and row strides, in 64- and
128-slot leaves, and where a key's fingerprint has more candidates than the three confirmed in
rounds (the walk of the rest of the head).
"""
import numpy as np
import pytest

import oracle_lib as O
import stage
from stage._lib import check
from test_gpu_parity import check_probe

pytestmark = pytest.mark.gpu

WAVE, LANE = 0, 1
COUNTS = (1, 63, 64, 65, 197)  # a lone probe, a partial / full chunk, a partial last row group


def set_form(tab, form):
    check(stage.lib().stage_set_probe_form(tab.h, form), "stage_set_probe_form")


def versioned(payload):
    """test_gpu_probe_tuning's versioned8 recipe at a payload size: 8-byte keys over ~60 leaves,
    committed version chains, in-flight copies and deletes; 197 probes with duplicates and misses"""
    n = 3000 if payload == 1000 else 6000
    tab = stage.Table(key_width=8, payload_size=payload)
    orc = O.OracleTree(payload_size=payload)
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
    keys = np.concatenate([hot[:90], hot[:20], hot[270:], rng.integers(0, n, 40), rng.integers(n, 2 * n, 17)])
    keys = rng.permutation(keys).astype(np.uint64)
    assert keys.size == 197 and np.unique(keys).size < keys.size
    rids = rng.integers(0, cid + 4, keys.size).astype(np.uint32)
    return tab, orc, keys, rids


@pytest.fixture(scope="module")
def versioned8(gpu):
    tab, orc, keys, rids = versioned(1000)
    assert tab.leaf_capacity == 64 and tab.stride >= 1008 and tab.stats()["leaves"] > 8
    return tab, orc, keys, rids


@pytest.fixture(scope="module")
def versioned128(gpu):
    tab, orc, keys, rids = versioned(600)  # 103 records per 64-KiB leaf
    assert tab.leaf_capacity == 128 and tab.stats()["leaves"] > 8
    return tab, orc, keys, rids


def forms_agree(tab, orc, keys, rids, leaf_ids=None):
    """LANE against the oracle, then WAVE's bytes: status records and rows, and without rows"""
    try:
        set_form(tab, LANE)
        out1, rows1 = check_probe(tab, orc, keys, 8, read_ids=rids, leaf_ids=leaf_ids)
        bare1, none1 = tab.probe(keys, read_ids=rids, leaf_ids=leaf_ids, records=False)
        set_form(tab, WAVE)
        out0, rows0 = tab.probe(keys, read_ids=rids, leaf_ids=leaf_ids)
        assert out1.tobytes() == out0.tobytes()
        assert np.array_equal(rows1, rows0)
        assert none1 is None and bare1.tobytes() == out0.tobytes()
    finally:
        set_form(tab, LANE)  # the default
    return out1


@pytest.mark.parametrize("count", COUNTS)
def test_lane_form_on_a_versioned_table(versioned8, count):
    tab, orc, keys, rids = versioned8
    out = forms_agree(tab, orc, keys[:count], rids[:count])
    if count == 197:
        seen = set(np.unique(out["status"]).tolist())
        assert {stage.ST_LATEST, stage.ST_COPY, stage.ST_OLD, stage.ST_NOT_FOUND} <= seen


@pytest.mark.parametrize("count", COUNTS)
def test_lane_form_with_leaf_ids(versioned8, count):
    tab, orc, keys, rids = versioned8
    forms_agree(tab, orc, keys[:count], rids[:count], leaf_ids=tab.traverse(keys[:count]))


def test_lane_form_without_read_ids(versioned8):
    tab, orc, keys, _ = versioned8
    forms_agree(tab, orc, keys, None)


@pytest.mark.parametrize("count", COUNTS)
def test_lane_form_in_128_slot_leaves(versioned128, count):
    tab, orc, keys, rids = versioned128
    out = forms_agree(tab, orc, keys[:count], rids[:count])
    if count == 197:
        seen = set(np.unique(out["status"]).tolist())
        assert {stage.ST_LATEST, stage.ST_COPY, stage.ST_OLD, stage.ST_NOT_FOUND} <= seen


@pytest.mark.parametrize("stride,sb", [(0, 16), (1008, 32), (1008, 16)])
def test_lane_form_output_layouts(versioned8, stride, sb):
    """16-B status records and a 1008-B row stride: the LANE form's bytes are the WAVE form's,
    whose layouts test_gpu_output_layout holds against the default one"""
    tab, orc, keys, rids = versioned8
    try:
        tab.set_output_layout(stride, sb)
        assert tab.stride == (stride or 1024)
        set_form(tab, WAVE)
        out0, rows0 = tab.probe(keys, read_ids=rids)
        set_form(tab, LANE)
        out1, rows1 = tab.probe(keys, read_ids=rids)
        assert out1.dtype == (stage.PROBE_OUT16_DTYPE if sb == 16 else stage.PROBE_OUT_DTYPE)
        assert out1.tobytes() == out0.tobytes()
        assert np.array_equal(rows1, rows0)
        bare, none = tab.probe(keys, read_ids=rids, records=False)
        assert none is None and bare.tobytes() == out0.tobytes()
        o_out, o_rec = orc.read_batch(keys, 8, rids)
        assert (out1["status"] == o_out["status"]).all() and (rows1[:, :orc.row] == o_rec).all()
    finally:
        set_form(tab, LANE)  # the default
        tab.set_output_layout(0, 32)


def fingerprints(keys):
    """key_fp_words for one order word (stage_core.hpp): the top byte of order_key x
    0x9E3779B97F4A7C15, 0 -> 1; order_key of an 8-byte key = its bytes, sign bits flipped, big-endian"""
    k = np.ascontiguousarray(keys, np.uint64)
    ok = (k ^ np.uint64(0x8080808080808080)).byteswap()
    fp = ((ok * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(56)).astype(np.uint32)
    return np.where(fp == 0, 1, fp)


def test_lane_form_walks_a_crowded_fingerprint(gpu):
    """one leaf of 46 keys, six of them with one fingerprint: the hits behind the third
    candidate, and two absent keys with that fingerprint, take the walk of the rest of the head"""
    pool = np.arange(1, 40000, dtype=np.uint64)
    fp = fingerprints(pool)
    counts = np.bincount(fp, minlength=256)
    f = int(np.argmax(counts))
    same = pool[fp == f]
    assert same.size >= 8
    crowd, absent = same[:6], same[6:8]
    others = pool[fp != f][:40]
    rng = np.random.default_rng(3)
    members = rng.permutation(np.concatenate([crowd, others]))
    tab = stage.Table(key_width=8)
    orc = O.OracleTree()
    assert tab.load_keys(members, 8, 1) == members.size
    assert orc.load_keys(members, 8, 1) == members.size
    tab.sync()
    assert tab.stats()["leaves"] == 1
    keys = np.concatenate([crowd, absent, others[:5]]).astype(np.uint64)
    out = forms_agree(tab, orc, keys, None)
    assert (out["status"][:6] == stage.ST_LATEST).all() and (out["status"][6:8] == stage.ST_NOT_FOUND).all()
    assert np.unique(out["slot"][:6]).size == 6  # six slots, one fingerprint: three lie behind three candidates
