"""CPU: argument checks of the column-window probes (stage_probe_batch_window,
stage_probe_host_window) on a created, unsynced table.  The window is validated against the
table's parameters before the "needs stage_sync" state, so both errors are visible without a
device; nothing is launched."""
import ctypes

import pytest

import stage

E_ARG, E_STATE = -1, -4
PAYLOAD = 1000


@pytest.fixture(scope="module")
def unsynced():
    tab = stage.Table(key_width=8, payload_size=PAYLOAD)
    tab.load_ycsb(0, 100, 8)
    return tab


def batch_window(h, n=1, off=100, ln=100, keys=16, out=16, win=16):
    """stage_probe_batch_window with placeholder device pointers (never dereferenced: every call
    here ends in an argument or state error)"""
    return stage.lib().stage_probe_batch_window(h, keys, None, None, None, n, off, ln, out, win, None)


def host_window(h, n=1, off=100, ln=100, keys=16, out=16, win=16):
    return stage.lib().stage_probe_host_window(h, keys, None, None, n, off, ln, out, win)


def last_error():
    return stage.lib().stage_last_error()


@pytest.mark.parametrize("call", [batch_window, host_window])
def test_argument_errors_come_before_the_state_error(unsynced, call):
    h = unsynced.h
    bad = [
        dict(h=None),                       # null table
        dict(h=h, ln=0),                    # empty window
        dict(h=h, off=PAYLOAD, ln=1),       # starts past the payload
        dict(h=h, off=PAYLOAD - 99, ln=100),  # ends one byte past it
        dict(h=h, off=0, ln=PAYLOAD + 1),
        dict(h=h, off=0xFFFFFFFF, ln=2),    # off + len wraps in 32 bits
        dict(h=h, win=None),
        dict(h=h, out=None),
        dict(h=h, keys=None),
    ]
    for kw in bad:
        assert stage.lib().stage_set_probe_tuning(h, 3, 0) == E_ARG  # leaves another message behind
        before = last_error()
        assert call(**kw) == E_ARG, kw
        msg = last_error()
        assert len(msg) > 0 and msg != before and b"stage_sync" not in msg, (kw, msg)


@pytest.mark.parametrize("call", [batch_window, host_window])
@pytest.mark.parametrize("off,ln", [(100, 100), (0, PAYLOAD), (PAYLOAD - 1, 1), (3, 5)])
def test_valid_window_reaches_the_state_error(unsynced, call, off, ln):
    assert call(unsynced.h, off=off, ln=ln) == E_STATE
    assert b"stage_sync" in last_error()
    # null buffers are fine for an empty batch; the stale image is still reported
    assert call(unsynced.h, n=0, off=off, ln=ln, keys=None, out=None, win=None) == E_STATE


def test_window_stride():
    L = stage.lib()
    for ln, exp in [(1, 16), (16, 16), (17, 32), (100, 112), (1000, 1008)]:
        assert L.stage_window_stride(ln) == exp == (ln + 15) & ~15
        assert stage.window_stride(ln) == exp


def test_python_window_rejects_for_update(unsynced):
    with pytest.raises(ValueError):
        unsynced.probe([1], window=(0, 4), for_update=[1])
    # the keyword reaches the C entry point: a bad window is the library's argument error
    with pytest.raises(stage.StageError, match="payload_size"):
        unsynced.probe_host([1], window=(PAYLOAD, 1))
