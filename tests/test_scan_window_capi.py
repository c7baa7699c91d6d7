"""CPU: argument checks of the column-window scans (stage_scan_batch_window,
stage_index_scan_batch_window) on a created, unsynced table.  The window and the buffers are
validated before the "needs stage_sync" state, so both errors are visible without a device;
nothing is launched."""
import pytest

import stage

E_ARG, E_STATE = -1, -4
PAYLOAD = 1000


@pytest.fixture(scope="module")
def unsynced():
    tab = stage.Table(key_width=8, payload_size=PAYLOAD)
    tab.load_ycsb(0, 100, 8)
    return tab


def scan_window(h, n=1, size=10, off=100, ln=100, keys=16, counts=16, win=16, row_keys=16):
    """stage_scan_batch_window with placeholder device pointers (never dereferenced: every call
    here ends in an argument or state error)"""
    return stage.lib().stage_scan_batch_window(h, keys, None, n, size, off, ln, counts, win, row_keys, None)


def index_scan_window(h, n=1, size=10, off=100, ln=100, keys=16, counts=16, win=16, row_keys=16, status=16):
    return stage.lib().stage_index_scan_batch_window(h, keys, None, None, n, size, off, ln, counts, win, row_keys,
                                                     status, None)


def last_error():
    return stage.lib().stage_last_error()


@pytest.mark.parametrize("call", [scan_window, index_scan_window])
def test_argument_errors_come_before_the_state_error(unsynced, call):
    h = unsynced.h
    bad = [
        dict(h=None),                         # null table
        dict(h=h, ln=0),                      # empty window
        dict(h=h, off=PAYLOAD, ln=1),         # starts past the payload
        dict(h=h, off=PAYLOAD - 99, ln=100),  # ends one byte past it
        dict(h=h, off=0xFFFFFFFF, ln=2),      # off + len wraps in 32 bits
        dict(h=h, win=None),
        dict(h=h, counts=None),
        dict(h=h, keys=None),
    ]
    if call is index_scan_window:
        bad.append(dict(h=h, status=None))
    for kw in bad:
        assert stage.lib().stage_set_probe_tuning(h, 3, 0) == E_ARG  # leaves another message behind
        before = last_error()
        assert call(**kw) == E_ARG, kw
        msg = last_error()
        assert len(msg) > 0 and msg != before and b"stage_sync" not in msg, (kw, msg)


@pytest.mark.parametrize("call", [scan_window, index_scan_window])
@pytest.mark.parametrize("off,ln", [(100, 100), (0, PAYLOAD), (PAYLOAD - 1, 1), (3, 5)])
def test_valid_window_reaches_the_state_error(unsynced, call, off, ln):
    assert call(unsynced.h, off=off, ln=ln) == E_STATE
    assert b"stage_sync" in last_error()
    assert call(unsynced.h, off=off, ln=ln, row_keys=None) == E_STATE  # the keys are optional
    assert b"stage_sync" in last_error()
    # null buffers are fine for an empty batch and for empty scans; the stale image is still reported
    none = dict(keys=None, counts=None, win=None, row_keys=None)
    if call is index_scan_window:
        none["status"] = None
    assert call(unsynced.h, n=0, off=off, ln=ln, **none) == E_STATE
    assert call(unsynced.h, size=0, off=off, ln=ln, **none) == E_STATE
    assert b"stage_sync" in last_error()


def test_scan_tuning_arguments(unsynced):
    L = stage.lib()
    assert L.stage_set_scan_tuning(None, 0) == E_ARG
    assert L.stage_set_scan_tuning(unsynced.h, -1) == E_ARG
    assert L.stage_set_scan_tuning(unsynced.h, 1) == 0
    assert L.stage_set_scan_tuning(unsynced.h, 0) == 0


def test_python_window_reaches_the_c_entry_point(unsynced):
    # a bad window is the library's argument error, a good one its state error
    with pytest.raises(stage.StageError, match="payload_size"):
        unsynced.range_scan([1], 10, window=(PAYLOAD, 1))
    with pytest.raises(stage.StageError, match="payload_size"):
        unsynced.index_scan([1], 10, window=(PAYLOAD - 3, 4), row_keys=True)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.range_scan([1], 10, window=(0, 4))
    with pytest.raises(ValueError):
        unsynced.range_scan([1], 10, row_keys=True)  # the rows carry their keys
    assert unsynced.key_pad == 8
