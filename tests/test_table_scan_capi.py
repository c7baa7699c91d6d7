"""CPU: argument checks of the whole-table scans (stage_table_scan, stage_table_scan_window) on a
created, unsynced table.  The range, the buffers and the window are validated before the "needs
stage_sync" state, so both errors are visible without a device; nothing is launched."""
import ctypes

import pytest

import stage
from stage._lib import LIB_PATH, SIGNATURES

E_ARG, E_STATE = -1, -4
PAYLOAD = 1000
END = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def unsynced():
    tab = stage.Table(key_width=8, payload_size=PAYLOAD)
    tab.load_ycsb(0, 100, 8)
    return tab


def rid(value):
    return None if value is None else ctypes.byref(ctypes.c_uint32(value))


def scan(h, begin=0, end=END, read_id=None, max_records=10, count=16, offsets=16, recs=16, meta=16, status=16):
    """stage_table_scan with placeholder device pointers (never dereferenced: every call here ends
    in an argument or state error)"""
    return stage.lib().stage_table_scan(h, begin, end, rid(read_id), max_records, count, offsets, recs, meta, status,
                                        None)


def scan_window(h, begin=0, end=END, read_id=None, off=100, ln=100, max_records=10, count=16, offsets=16, recs=16,
                keys=16, meta=16, status=16):
    return stage.lib().stage_table_scan_window(h, begin, end, rid(read_id), off, ln, max_records, count, offsets, recs,
                                               keys, meta, status, None)


def last_error():
    return stage.lib().stage_last_error()


def test_symbols_are_exported_with_signatures():
    L = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("stage_table_scan", 11), ("stage_table_scan_window", 14)):
        assert hasattr(L, name), name
        res, args = SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert getattr(stage.lib(), name).argtypes == args


@pytest.mark.parametrize("call", [scan, scan_window])
@pytest.mark.parametrize("read_id", [None, 7])
def test_argument_errors_come_before_the_state_error(unsynced, call, read_id):
    h = unsynced.h
    bad = [
        dict(h=None),                  # null table
        dict(h=h, begin=2, end=1),     # leaf_begin > leaf_end
        dict(h=h, begin=END, end=5),
        dict(h=h, count=None),         # null d_count
        dict(h=h, count=None, max_records=0, recs=None),
        dict(h=h, recs=None),          # max_records != 0 with a null d_records / d_window
        dict(h=h, recs=None, max_records=1 << 40),
    ]
    if call is scan_window:
        bad += [
            dict(h=h, ln=0),                      # empty window
            dict(h=h, off=PAYLOAD, ln=1),         # starts past the payload
            dict(h=h, off=PAYLOAD - 99, ln=100),  # ends one byte past it
            dict(h=h, off=0xFFFFFFFF, ln=2),      # off + len wraps in 32 bits
            dict(h=h, ln=0, max_records=0, recs=None),
        ]
    for kw in bad:
        assert stage.lib().stage_set_probe_tuning(h, 3, 0) == E_ARG  # leaves another message behind
        before = last_error()
        assert call(read_id=read_id, **kw) == E_ARG, kw
        msg = last_error()
        assert len(msg) > 0 and msg != before and b"stage_sync" not in msg, (kw, msg)


@pytest.mark.parametrize("call", [scan, scan_window])
@pytest.mark.parametrize("read_id", [None, 7])
def test_valid_call_reaches_the_state_error(unsynced, call, read_id):
    h = unsynced.h
    cases = [
        dict(),
        dict(begin=0, end=1),
        dict(begin=3, end=3),                                    # an empty range
        dict(begin=5, end=1 << 40),                              # the leaf count is checked after the state
        dict(offsets=None, meta=None, status=None),              # the optional outputs
        dict(max_records=0, recs=None),                          # count only
        dict(max_records=0, recs=None, offsets=None, meta=None, status=None),
    ]
    if call is scan_window:
        cases += [dict(off=0, ln=PAYLOAD), dict(off=PAYLOAD - 1, ln=1), dict(off=3, ln=5), dict(keys=None),
                  dict(max_records=0, recs=None, keys=None)]
    for kw in cases:
        assert call(h, read_id=read_id, **kw) == E_STATE, kw
        assert b"stage_sync" in last_error()


def test_python_table_scan_reaches_the_c_entry_points(unsynced):
    # table_scan_device takes raw pointers too: placeholders, as above
    with pytest.raises(stage.StageError, match="payload_size"):
        unsynced.table_scan_device(None, None, 0, 16, window=(PAYLOAD, 1))
    with pytest.raises(stage.StageError, match="leaf_begin"):
        unsynced.table_scan_device((4, 2), None, 0, 16)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_device(None, None, 0, 16)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_device((0, 1), 5, 10, 16, 16, 16, window=(0, 4), d_row_keys=16, d_row_meta=16,
                                   d_row_status=16)
    with pytest.raises(ValueError):
        unsynced.table_scan(row_keys=True)  # the rows carry their keys
    assert stage.LEAF_END == END
