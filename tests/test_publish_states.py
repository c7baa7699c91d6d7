"""CPU: the write script of publish_states.py keeps the host table and the oracle identical, and
reaches the states the GPU test (test_gpu_publish_states.py) is about.

No publish happens here.  After every phase the host layout and the reference-format leaf blocks
equal the oracle's, and the states are read back from both sides rather than assumed: a leaf with
an empty slot group beside live ones, a leaf with records but none visible, visible slots behind a
leaf's sorted ones, an in-flight insert without a copy, a record count that fell with an aborted
insert and rose again, and scans that end at the emptied leaf.  The oracle's answers for every
read entry point are computed too, so the GPU test's inputs are known to be valid before it runs.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import stage
from publish_states import GEOMETRIES, M_CONTROL, PHASES, State
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
