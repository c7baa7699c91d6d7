"""CPU: the write script of publish_states.py keeps the host table and the oracle identical, and
reaches the states the GPU test (test_gpu_publish_states.py) is about.

No publish happens here.  After every phase the host layout and the reference-format leaf blocks
equal the oracle's, and the states are read back from both sides rather than assumed: a leaf with
an empty slot group beside live ones, a leaf with records but none visible, visible slots behind a
leaf's sorted ones, an in-flight insert without a copy, a record count that fell with an aborted
insert and rose again, and scans that end at the emptied leaf.  The oracle's answers for every
read entry point are computed too, so the GPU test's inputs are known to be valid before it runs.

test_epoch_script_reaches_its_codes does the same for the steps of test_gpu_device_epochs.py, with
every epoch applied through the host's per-key calls instead of the device: host and oracle stay
identical, and the oracle's codes show that every epoch holds the cases it was drawn for.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import stage
from publish_states import EPOCH_SEED, EPOCH_STEPS, FINISH_BEFORE, GEOMETRIES, M_CONTROL, PHASES, State
from scan_semantics import LeafScanner
from test_host_layout import compare_layout


def oracle_record_meta(orc, k):
    """the meta word and next handle of the oracle's record of key k, whatever a reader would see"""
    meta, loc, nxt = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
    assert O.lib().orc_record_meta(orc.t, k, len(k), ctypes.byref(meta), ctypes.byref(loc), ctypes.byref(nxt)) == 0
    return meta.value, nxt.value


def check_states(st, phase, x):
    tab, orc = st.tab, st.orc
    v = x.view
    rc, sc, meta, _ = tab.export_leaves()
    o_rc, o_sc, o_meta, _ = orc.export_leaves(st.cap)
    vis = (meta & np.uint64(1 << 62)) != 0
    o_vis = (o_meta & np.uint64(1 << 62)) != 0
    if st.hole_key:  # no visible slot in 64..127, visible slots elsewhere
        a = st.hole_leaf()
        for m in (vis, o_vis):
            assert not m[a, 64:128].any() and m[a, :64].any()
        assert rc[a] > 64 and not v[a].vis[64:128].any() and v[a].vis[:64].any()
    # visible slots beyond the sorted count
    assert any(vis[i, sc[i]:rc[i]].any() and o_vis[i, o_sc[i]:o_rc[i]].any() for i in range(rc.size))
    # in-flight inserts: the control bit, visible, and no copy behind them
    assert st.inflight
    for k in st.inflight:
        m, nxt = oracle_record_meta(orc, k)
        assert m & M_CONTROL and m & (1 << 62) and nxt == 0, (k, hex(m), nxt)
        assert any(k in l.visible_keys() for l in v)
    assert st.refused_rc == stage.RC_INVALID
    for before, after in st.abort_counts:  # the aborted insert took the leaf's last slot away, on both sides
        assert before[0] == before[1] and after[0] == after[1] == before[0] - 1
    if phase == "P1":
        assert not x.empty
        return
    # the emptied leaf: records, none visible; the scans from the five keys before it stop there
    assert len(x.empty) == 1
    e = x.empty[0]
    assert e == st.leaf_of([st.empty_key])[0]
    for c, m in ((rc, vis), (o_rc, o_vis)):
        assert c[e] > 0 and not m[e].any() and m[e + 1:].any()
    five = x.starts[x.five[0][0]:x.five[0][-1] + 1]
    assert [orc.scan(k, len(k), 10)[0] for k in five] == [5, 4, 3, 2, 1]
    for size in (63, 100):
        assert x.scans[size][0][x.five[0]].tolist() == [5, 4, 3, 2, 1]
    if phase == "P2":  # the slot an aborted insert freed is taken again
        for k, (_, after) in zip(st.aborted, st.abort_counts):
            assert all(c > after[0] for c in st.counts(st.leaf_of([k])[0]))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_script_reaches_its_states(name):
    st = State(name)
    rng = np.random.default_rng(5)
    leaves = {}
    for phase in PHASES:
        st.run(phase)
        compare_layout(st.tab, st.orc)
        b, sk, sl = st.tab.export_leaf_images()
        ob, osk, osl = st.orc.export_leaf_images(kwords=st.kw)
        assert np.array_equal(b, ob) and np.array_equal(sk, osk) and np.array_equal(sl, osl)
        leaves[phase] = st.tab.stats()["leaves"]
        assert leaves[phase] == st.orc.stats()["leaves"]
        x = st.expected_reads(rng)
        if phase != "P0":
            check_states(st, phase, x)
        if st.width == 8:  # LeafScanner over the exported leaves reproduces the oracle's scans
            scanner = LeafScanner(st.tab)
            for i in list(range(0, len(x.starts), 4)) + [j for five in x.five for j in five]:
                for size in (7, 100):
                    oc, orows = x.scans[size]
                    got = scanner.scan(int.from_bytes(x.starts[i], "little"), size)
                    exp = np.ascontiguousarray(orows[i, :oc[i], :8]).view(np.uint64).reshape(-1)
                    assert np.array_equal(got, exp), (phase, i, size)
    assert leaves["P0"] == leaves["P1"] == leaves["P2"] < leaves["P3"] == leaves["P4"]
    assert st.halves and all(len(h) > 30 for h in st.halves)


def same_tables(st):
    compare_layout(st.tab, st.orc)
    b, sk, sl = st.tab.export_leaf_images()
    ob, osk, osl = st.orc.export_leaf_images(kwords=st.kw)
    assert np.array_equal(b, ob) and np.array_equal(sk, osk) and np.array_equal(sl, osl)
    assert st.tab.stats()["versions"] == st.orc.stats()["versions"]


def check_epoch(st, step, ep, codes, new_probes):
    """the oracle's codes alone: the epoch reaches what it was drawn for"""
    n = {rc: int((codes == rc).sum()) for rc in (stage.RC_OK, stage.RC_NOT_FOUND, stage.RC_NOT_NEEDED_UPDATE,
                                                 stage.RC_DIRTY, stage.RC_INVALID)}
    what = (st.name, step, n)
    group = codes[[i for i, k in enumerate(ep.keys) if k == ep.hot]]
    assert group.size == 200, what
    fails = np.nonzero(group != stage.RC_OK)[0]
    assert fails.size and 200 - fails[0] >= 128, what  # kJumpFrom ops from the first failure on
    if step == "E4":  # past the payload: INVALID on a live record, DIRTY in flight, NOT_FOUND
        assert n[stage.RC_OK] == 0 and min(n[stage.RC_INVALID], n[stage.RC_DIRTY], n[stage.RC_NOT_FOUND]) >= 20, what
        assert sum(n.values()) == codes.size and not new_probes, what
        return
    assert n[stage.RC_OK] >= 0.3 * codes.size and n[stage.RC_INVALID] == 0, what
    assert min(n[stage.RC_NOT_FOUND], n[stage.RC_NOT_NEEDED_UPDATE], n[stage.RC_DIRTY]) >= 20, what
    # both codes interleave in the hot group; the second hot group is DIRTY behind its uncommitted op
    assert (group == stage.RC_OK).sum() >= 40 and (group == stage.RC_NOT_NEEDED_UPDATE).sum() >= 40, what
    at = ep.where[("hot2", 35)]
    group2 = codes[[i for i, k in enumerate(ep.keys) if k == ep.hot2]]
    assert codes[at] == stage.RC_OK and ep.cid[at] == 0 and (group2[36:] == stage.RC_DIRTY).all(), what
    if ep.head_repeat:
        assert codes[ep.where[("hot", 0)]] == stage.RC_NOT_NEEDED_UPDATE, what
    for k in st.inflight:  # an insert in flight is found by the locate probe and must be DIRTY
        assert all(codes[i] == stage.RC_DIRTY for i, x in enumerate(ep.keys) if x == k), what
    if st.width == 0:  # a live key's bytes and one more zero byte: the same key word, not the key
        longer = [i for i, k in enumerate(ep.keys) if k.endswith(b"\0")]
        assert len(longer) == 10 and (codes[longer] == stage.RC_NOT_FOUND).all(), what
    if ep.sst is None:
        assert not new_probes, what
        return
    # a retired version that ends two ids before the commit: a read between them finds no version
    assert len(new_probes) >= 20, what
    for k, rid in new_probes:
        out, _ = st.orc.read(k, len(k), rid)
        assert out["status"] == (stage.ST_CHAIN_MISS if rid % 4 == 1 else stage.ST_OLD), (what, k, rid, out)
        assert st.orc.read(k, len(k), rid | 3)[0]["status"] in (stage.ST_LATEST, stage.ST_OLD, stage.ST_COPY), what


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_epoch_script_reaches_its_codes(name):
    st = State(name)
    rng, erng = np.random.default_rng(5), np.random.default_rng(EPOCH_SEED)
    for step in EPOCH_STEPS:
        if step in PHASES:
            if step in FINISH_BEFORE:
                assert st.finish_device_flying(erng) >= 8, (name, step)
            st.run(step)
        else:
            eps = st.draw_step(erng, step)
            for ep in eps:
                before = len(st.sst_probes)
                codes = st.apply_epoch_on_host(ep)
                check_epoch(st, step, ep, codes, st.sst_probes[before:])
        assert st.busy == {k for l in st.view() for k, m in zip(l.keys, l.meta.tolist())
                           if m & M_CONTROL and k not in st.inflight}, (name, step)
        same_tables(st)
        x = st.expected_reads(rng)
        if step in ("P2", "P3", "P4", "E5"):  # the states the phases made last through the epochs
            check_states(st, "P2" if step == "P2" else "P4", x)
    assert st.rc_seen >= {stage.RC_OK, stage.RC_NOT_FOUND, stage.RC_NOT_NEEDED_UPDATE, stage.RC_DIRTY,
                          stage.RC_INVALID}
    assert st.halves and all(len(h) > 30 for h in st.halves)
