"""GPU: every read entry point after full and incremental publishes, in every leaf geometry.

publish_states.py drives one table per geometry (8-byte keys in 64- and 128-slot leaves,
variable-length keys, 8-, 16- and 32-byte keys in leaves of up to 1024 slots) through five write
phases; the table is published after each -- P0 and P3 rebuild every leaf, P1, P2 and P4 go
through patch_device / patch_kernel -- and probe, range_scan, index_scan, index_scan_first,
table_scan and resolve are then held against the oracle, exactly.  What the patched leaves hold is
what the kernels' derived structures are for: key-plane words of wide keys written slot by slot,
a slot group left without a visible record, a leaf left without any (a scan that reaches it ends
there), counts that fell and rose, slots behind the monotone prefix.  test_publish_states.py shows
on the CPU that the script reaches those states.
"""
import numpy as np
import pytest

import stage
from publish_states import GEOMETRIES, INCREMENTAL, PHASES, State, check_all_reads

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_reads_after_every_publish(gpu, name):
    st = State(name)
    rng = np.random.default_rng(len(name))
    leaves = None
    for phase in PHASES:
        st.run(phase)
        st.tab.sync()
        info = st.tab.sync_info()
        assert info["incremental"] == (phase in INCREMENTAL), (phase, info)
        if phase in INCREMENTAL:
            assert info["leaves"] > 0 and info["slots"] > 0, (phase, info)
            assert st.tab.stats()["leaves"] == leaves, phase
        elif leaves is not None:
            assert st.tab.stats()["leaves"] > leaves, phase  # P3: leaves split
        leaves = st.tab.stats()["leaves"]
        print(name, phase, info)  # shown with a failure: the phase it happened in
        check_all_reads(st, rng)
    assert st.seen >= {stage.ST_LATEST, stage.ST_COPY, stage.ST_OLD, stage.ST_NOT_FOUND}, st.seen
    # scans from the keys before the emptied leaf returned fewer records than asked for although
    # larger keys exist
    assert st.stops > 0
