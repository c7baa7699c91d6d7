"""GPU: device write epochs (stage_update_batch_device) in every leaf geometry, on images with
history, and every read entry point after them.

test_gpu_write_path.py covers the write path's kernels on freshly loaded tables of 8-byte keys in
64-slot leaves.  Here the epochs of publish_states.py run between the publishes of its write
phases, in all seven geometries -- variable-length keys (d_lens), 16- and 32-byte keys, 128- to
1024-slot leaves, payloads of 8 to 1000 bytes (heap rows of one to 63 16-byte chunks) -- so the
image an epoch locates its keys in and writes to holds slots behind the sorted prefix, deleted
slots, an empty slot group, an emptied leaf, host updates in flight and inserts in flight (which the
locate probe reports as not found, with their slot: the epoch must answer DIRTY).  Windows: the
whole payload, its last byte, an odd offset and length, and one past the payload's end; end stamps
(d_sstamps) below, at and above the commit id.  Steps (EPOCH_STEPS):

  P0, P1     the phases, published
  E1         an epoch, whole payload, no end stamps                         -> every read path
  P2         the host commits and aborts updates E1 left in flight (copy headers the device wrote),
             then the phase; an incremental publish on top of the epoch
  E2         last byte, mixed end stamps                                    -> every read path
  E3         two epochs enqueued back to back on one stream, no host wait
  P3         the host finishes more of them and inserts until leaves split: a full publish that
             must carry the device-written rows                             -> every read path
  P4         incremental
  E4         a window past the payload: no op succeeds, no read changes
  E5         the whole payload again, mixed end stamps                      -> every read path

Every epoch's codes equal the oracle's, applied op by op.  At the end the settled host table equals
the oracle's: layout, leaf blocks, version count.  test_publish_states.py shows on the CPU that
the epochs hold the cases they are drawn for.
"""
import numpy as np
import pytest

import stage
from publish_states import (EPOCH_SEED, EPOCH_STEPS, FINISH_BEFORE, GEOMETRIES, INCREMENTAL, PHASES, State,
                            check_all_reads)
from stage._lib import check
from test_host_layout import compare_layout

pytestmark = pytest.mark.gpu

READS_AFTER = ("E1", "E2", "P3", "E5")


def probe_bytes(st, keys, rids):
    words, lens = st.pack(keys)
    out, rows = st.tab.probe(words, read_ids=rids, lens=lens)
    return out.tobytes(), rows.tobytes()


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_device_epochs_between_publishes(gpu, name):
    st = State(name)
    rng, erng = np.random.default_rng(len(name)), np.random.default_rng(EPOCH_SEED)
    leaves = None
    for step in EPOCH_STEPS:
        if step in PHASES:
            if step in FINISH_BEFORE:
                assert st.finish_device_flying(erng) >= 8, step
            st.run(step)
            st.tab.sync()
            info = st.tab.sync_info()
            print(name, step, info)  # shown with a failure: the step it happened in
            assert info["incremental"] == (step in INCREMENTAL), (step, info)
            if step == "P3":
                assert st.tab.stats()["leaves"] > leaves, step  # leaves split
            leaves = st.tab.stats()["leaves"]
        elif step == "E3":
            codes = st.device_epochs_pipelined(st.draw_step(erng, step))
            assert all((c == stage.RC_OK).sum() > 0.3 * c.size for c in codes)
        elif step == "E4":  # nothing succeeds, so nothing a reader sees may change
            ep, = st.draw_step(erng, step)
            keys = (st.some(rng, ep.keys, 200) + st.some(rng, st.everything, 60) + st.inflight
                    + st.some(rng, sorted(st.busy), 20) + st.some(rng, st.deleted, 20))[:300]
            rids = rng.choice(st.read_id_pool(), len(keys)).astype(np.uint32)
            before = probe_bytes(st, keys, rids)
            codes = st.device_epoch(ep)
            assert not (codes == stage.RC_OK).any() and (codes == stage.RC_INVALID).any()
            assert probe_bytes(st, keys, rids) == before
        else:
            ep, = st.draw_step(erng, step)
            st.device_epoch(ep)
        if step == "E2":  # the last probes: read ids at an end stamp two below its commit id, and between the two
            x = st.expected_reads(rng)
            tail = x.reads[True][0]["status"][-len(st.sst_probes):]
            assert len(st.sst_probes) >= 40 and tail.tolist() == [stage.ST_CHAIN_MISS, stage.ST_OLD] * (tail.size // 2)
            st.compare_reads(x)
            assert stage.ST_CHAIN_MISS in st.seen
        elif step in READS_AFTER:
            check_all_reads(st, rng)
    check(stage.lib().stage_settle(st.tab.h), "settle")
    compare_layout(st.tab, st.orc)
    b, sk, sl = st.tab.export_leaf_images()
    ob, osk, osl = st.orc.export_leaf_images(kwords=st.kw)
    assert np.array_equal(b, ob) and np.array_equal(sk, osk) and np.array_equal(sl, osl)
    assert st.tab.stats()["versions"] == st.orc.stats()["versions"]
    assert st.seen >= {stage.ST_LATEST, stage.ST_COPY, stage.ST_OLD, stage.ST_NOT_FOUND, stage.ST_CHAIN_MISS}, st.seen
    assert st.rc_seen >= {stage.RC_OK, stage.RC_NOT_FOUND, stage.RC_NOT_NEEDED_UPDATE, stage.RC_DIRTY,
                          stage.RC_INVALID}, st.rc_seen
