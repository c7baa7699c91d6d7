"""CPU: argument checks of the filtered whole-table scans (stage_table_scan_where,
stage_table_scan_where_window, stage_table_scan_aggregate) on a created, unsynced table.  The
predicates, the aggregate column, the range, the buffers and the window are validated before the
"needs stage_sync" state, so both errors are visible without a device; nothing is launched."""
import ctypes

import pytest

import stage
from stage._lib import LIB_PATH, PRED_MAX, SIGNATURES, ScanAgg, ScanPred

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


def pred(off=0, width=4, lo=0, hi=10, is_signed=0, negate=0, pad=0):
    return ScanPred(off, width, is_signed, negate, pad, lo, hi)


ONE = (pred(),)


def pred_args(preds, n_pred, null_preds):
    arr = (ScanPred * max(len(preds), 1))(*preds)
    return (None if null_preds else arr), (len(preds) if n_pred is None else n_pred)


# placeholder device pointers (never dereferenced: every call here ends in an argument or state error)
def where(h, begin=0, end=END, read_id=None, preds=ONE, n_pred=None, null_preds=False, max_records=10, count=16,
          offsets=16, recs=16, slot=16, meta=16, status=16):
    arr, n = pred_args(preds, n_pred, null_preds)
    return stage.lib().stage_table_scan_where(h, begin, end, rid(read_id), arr, n, max_records, count, offsets, recs,
                                              slot, meta, status, None)


def where_window(h, begin=0, end=END, read_id=None, preds=ONE, n_pred=None, null_preds=False, off=100, ln=100,
                 max_records=10, count=16, offsets=16, recs=16, keys=16, slot=16, meta=16, status=16):
    arr, n = pred_args(preds, n_pred, null_preds)
    return stage.lib().stage_table_scan_where_window(h, begin, end, rid(read_id), arr, n, off, ln, max_records, count,
                                                     offsets, recs, keys, slot, meta, status, None)


def aggregate(h, begin=0, end=END, read_id=None, preds=ONE, n_pred=None, null_preds=False, agg_off=0, agg_width=4,
              agg_signed=0, agg=16):
    arr, n = pred_args(preds, n_pred, null_preds)
    return stage.lib().stage_table_scan_aggregate(h, begin, end, rid(read_id), arr, n, agg_off, agg_width, agg_signed,
                                                  agg, None)


CALLS = [where, where_window, aggregate]


def last_error():
    return stage.lib().stage_last_error()


def test_symbols_are_exported_with_signatures():
    L = ctypes.CDLL(LIB_PATH)
    for name, nargs in (("stage_table_scan_where", 14), ("stage_table_scan_where_window", 17),
                        ("stage_table_scan_aggregate", 11)):
        assert hasattr(L, name), name
        res, args = SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert getattr(stage.lib(), name).argtypes == args


def test_struct_sizes():
    assert ctypes.sizeof(ScanPred) == 24 and ctypes.sizeof(ScanAgg) == 32
    assert PRED_MAX == 4
    assert [f[0] for f in ScanPred._fields_] == ["payload_off", "width", "is_signed", "negate", "pad", "lo", "hi"]
    assert ScanPred.lo.offset == 8 and ScanPred.hi.offset == 16 and ScanPred.width.offset == 4
    assert [getattr(ScanAgg, f).offset for f in ("count", "sum", "min", "max")] == [0, 8, 16, 24]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("read_id", [None, 7])
def test_argument_errors_come_before_the_state_error(unsynced, call, read_id):
    h = unsynced.h
    bad = [
        dict(h=None),                                              # null table
        dict(h=h, preds=(pred(),) * 5),                            # n_pred > STAGE_PRED_MAX
        dict(h=h, n_pred=5),
        dict(h=h, n_pred=0xFFFFFFFF),
        dict(h=h, null_preds=True),                                # null preds with n_pred != 0
        dict(h=h, null_preds=True, n_pred=4),
        dict(h=h, preds=(pred(width=0),)),                         # a width outside {1, 2, 4, 8}
        dict(h=h, preds=(pred(width=3),)),
        dict(h=h, preds=(pred(width=16),)),
        dict(h=h, preds=(pred(), pred(width=5))),                  # ... in a later predicate
        dict(h=h, preds=(pred(off=PAYLOAD - 3, width=4),)),        # ends one byte past the payload
        dict(h=h, preds=(pred(off=PAYLOAD, width=1),)),            # starts past it
        dict(h=h, preds=(pred(off=0xFFFFFFFF, width=8),)),         # off + width wraps in 32 bits
        dict(h=h, preds=(pred(), pred(), pred(), pred(off=PAYLOAD - 7, width=8))),
        dict(h=h, preds=(pred(is_signed=2),)),                     # is_signed / negate above 1
        dict(h=h, preds=(pred(negate=2),)),
        dict(h=h, preds=(pred(negate=255),)),
        dict(h=h, preds=(pred(pad=1),)),                           # pad != 0
        dict(h=h, begin=2, end=1),                                 # leaf_begin > leaf_end
        dict(h=h, begin=END, end=5),
    ]
    if call is aggregate:
        bad += [
            dict(h=h, agg=None),                                   # null d_agg
            dict(h=h, agg=None, preds=()),
            dict(h=h, agg_width=3),                                # the aggregate column
            dict(h=h, agg_width=16),
            dict(h=h, agg_off=PAYLOAD - 7, agg_width=8),           # ends one byte past the payload
            dict(h=h, agg_off=PAYLOAD - 7, agg_width=8, preds=()),
            dict(h=h, agg_off=PAYLOAD, agg_width=1),
            dict(h=h, agg_off=0xFFFFFFFF, agg_width=2),
            dict(h=h, agg_signed=2),
        ]
    else:
        bad += [
            dict(h=h, count=None),                                 # null d_count
            dict(h=h, count=None, max_records=0, recs=None),
            dict(h=h, recs=None),                                  # max_records != 0 with a null record buffer
            dict(h=h, recs=None, max_records=1 << 40),
        ]
    if call is where_window:
        bad += [
            dict(h=h, ln=0),                                       # empty window
            dict(h=h, off=PAYLOAD, ln=1),                          # starts past the payload
            dict(h=h, off=PAYLOAD - 99, ln=100),                   # ends one byte past it
            dict(h=h, off=0xFFFFFFFF, ln=2),                       # off + len wraps in 32 bits
            dict(h=h, ln=0, max_records=0, recs=None),
        ]
    for kw in bad:
        assert stage.lib().stage_set_probe_tuning(h, 3, 0) == E_ARG  # leaves another message behind
        before = last_error()
        assert call(read_id=read_id, **kw) == E_ARG, kw
        msg = last_error()
        assert len(msg) > 0 and msg != before and b"stage_sync" not in msg, (kw, msg)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("read_id", [None, 7])
def test_valid_call_reaches_the_state_error(unsynced, call, read_id):
    h = unsynced.h
    cases = [
        dict(),
        dict(begin=0, end=1),
        dict(begin=3, end=3),                                      # an empty range
        dict(begin=5, end=1 << 40),                                # the leaf count is checked after the state
        dict(preds=()),                                            # n_pred == 0
        dict(preds=(), null_preds=True),                           # ... with null preds
        dict(preds=(pred(lo=5, hi=-5, is_signed=1),)),             # lo > hi is legal
        dict(preds=(pred(lo=5, hi=1, negate=1),)),
        dict(preds=(pred(off=PAYLOAD - 8, width=8, lo=-1, hi=-1),)),  # the row's last bytes; uint64 bit patterns
        dict(preds=(pred(off=PAYLOAD - 1, width=1), pred(off=6, width=4), pred(off=118, width=4, is_signed=1),
                    pred(off=5, width=2, negate=1))),              # STAGE_PRED_MAX of them, any alignment
    ]
    if call is aggregate:
        cases += [dict(agg_width=0), dict(agg_width=0, agg_off=1 << 30),  # count only: no column to check
                  dict(agg_off=PAYLOAD - 8, agg_width=8, agg_signed=1), dict(agg_off=PAYLOAD - 1, agg_width=1),
                  dict(agg_off=5, agg_width=2)]
    else:
        cases += [
            dict(offsets=None, slot=None, meta=None, status=None),  # the optional outputs
            dict(max_records=0, recs=None),                         # count only
            dict(max_records=0, recs=None, offsets=None, slot=None, meta=None, status=None),
        ]
    if call is where_window:
        cases += [dict(off=0, ln=PAYLOAD), dict(off=PAYLOAD - 1, ln=1), dict(off=3, ln=5), dict(keys=None),
                  dict(max_records=0, recs=None, keys=None)]
    for kw in cases:
        assert call(h, read_id=read_id, **kw) == E_STATE, kw
        assert b"stage_sync" in last_error()


def test_python_wrappers_reach_the_c_entry_points(unsynced):
    P = stage.Pred
    ok = [P(0, 4, 0, 10)]
    # the device forms take raw pointers too: placeholders, as above
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_where_device(None, None, ok, 0, 16)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_where_device((0, 1), 5, ok, 10, 16, 16, 16, window=(0, 4), d_row_keys=16, d_row_slot=16,
                                         d_row_meta=16, d_row_status=16)
    with pytest.raises(stage.StageError, match="width"):
        unsynced.table_scan_where_device(None, None, [P(0, 3, 0, 1)], 0, 16)
    with pytest.raises(stage.StageError, match="payload_size"):
        unsynced.table_scan_where_device(None, None, [P(PAYLOAD - 1, 2, 0, 1)], 0, 16)
    with pytest.raises(stage.StageError, match="payload_size"):
        unsynced.table_scan_where_device(None, None, ok, 0, 16, window=(PAYLOAD, 1))
    with pytest.raises(stage.StageError, match="STAGE_PRED_MAX"):
        unsynced.table_scan_where_device(None, None, ok * 5, 0, 16)
    with pytest.raises(stage.StageError, match="leaf_begin"):
        unsynced.table_scan_where_device((4, 2), None, ok, 0, 16)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_where_device(None, 7, (), 0, 16)  # no predicate
    with pytest.raises(ValueError):
        unsynced.table_scan_where(preds=ok, row_keys=True)  # the rows carry their keys
    # (table_scan_where and table_scan_aggregate allocate their device buffers first: GPU tests)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_aggregate_device(None, None, ok, (0, 4, True), 16)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_aggregate_device(None, 3, (), None, 16)  # count only
    with pytest.raises(stage.StageError, match="aggregate column"):
        unsynced.table_scan_aggregate_device(None, None, (), (PAYLOAD - 3, 4, False), 16)
    with pytest.raises(stage.StageError, match="d_agg"):
        unsynced.table_scan_aggregate_device(None, None, ok, (0, 4, False), None)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_aggregate_device((0, 1), 9, ok, None, 16)
    # Pred: Python ints in the column's domain, an unsigned 8-byte bound as its bit pattern
    p = P(8, 8, 1 << 63, (1 << 64) - 1)
    assert p == (8, 8, 1 << 63, (1 << 64) - 1, False, False)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_where_device(None, None, [p, P(0, 1, -128, 127, signed=True, negate=True)], 0, 16)
    assert "slots" in stage.TableScanWhereResult._fields
    assert stage.TableScanWhereResult._fields[:6] == stage.TableScanResult._fields
