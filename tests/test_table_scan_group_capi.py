"""CPU: argument checks of the grouped aggregate (stage_table_scan_group_aggregate) on a created,
unsynced table -- the predicates, the group column, the aggregate column, the range and the result
buffer are validated before the "needs stage_sync" state, so both errors are visible without a
device and nothing is launched -- and the expectation helper the GPU tests rest on
(table_scan_group_expect.group_aggregate), checked against a hand-written table."""
import collections
import ctypes

import numpy as np
import pytest

import stage
from stage._lib import GROUP_LDS_MAX, GROUP_MAX, LIB_PATH, SIGNATURES, ScanGroup, ScanPred
from table_scan_group_expect import folded, group_aggregate, group_ids

E_ARG, E_STATE = -1, -4
PAYLOAD = 1000
KEY_PAD = 8
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


def grp(off=0, width=1, is_signed=0, in_key=0, pad=0, base=0, n_groups=4, pad2=0):
    return ScanGroup(off, width, is_signed, in_key, pad, base, n_groups, pad2)


ONE = (pred(),)


# placeholder device pointers (never dereferenced: every call here ends in an argument or state error)
def call(h, begin=0, end=END, read_id=None, preds=ONE, n_pred=None, null_preds=False, group=None, null_group=False,
         agg_off=0, agg_width=4, agg_signed=0, groups=16):
    arr = (ScanPred * max(len(preds), 1))(*preds)
    g = group if group is not None else grp()
    return stage.lib().stage_table_scan_group_aggregate(
        h, begin, end, rid(read_id), None if null_preds else arr, len(preds) if n_pred is None else n_pred,
        None if null_group else ctypes.byref(g), agg_off, agg_width, agg_signed, groups, None)


def last_error():
    return stage.lib().stage_last_error()


def test_symbol_is_exported_with_its_signature():
    L = ctypes.CDLL(LIB_PATH)
    assert hasattr(L, "stage_table_scan_group_aggregate")
    res, args = SIGNATURES["stage_table_scan_group_aggregate"]
    assert res is ctypes.c_int and len(args) == 12
    assert stage.lib().stage_table_scan_group_aggregate.argtypes == args


def test_struct_layout_and_constants():
    assert ctypes.sizeof(ScanGroup) == 24
    assert [f[0] for f in ScanGroup._fields_] == ["off", "width", "is_signed", "in_key", "pad", "base", "n_groups", "pad2"]
    assert [getattr(ScanGroup, f).offset for f in ("off", "width", "is_signed", "in_key", "pad", "base", "n_groups",
                                                   "pad2")] == [0, 4, 5, 6, 7, 8, 16, 20]
    assert GROUP_MAX == stage.GROUP_MAX == 1 << 24
    assert 1 <= GROUP_LDS_MAX == stage.GROUP_LDS_MAX < GROUP_MAX
    assert 32 * (GROUP_LDS_MAX + 1) <= 64 * 1024  # a workgroup's table fits its LDS allocation


@pytest.mark.parametrize("read_id", [None, 7])
def test_argument_errors_come_before_the_state_error(unsynced, read_id):
    h = unsynced.h
    bad = [
        dict(h=None),                                              # null table
        dict(h=h, preds=(pred(),) * 5),                            # the predicate errors
        dict(h=h, n_pred=0xFFFFFFFF),
        dict(h=h, null_preds=True),
        dict(h=h, preds=(pred(width=3),)),
        dict(h=h, preds=(pred(off=PAYLOAD - 3, width=4),)),
        dict(h=h, preds=(pred(is_signed=2),)),
        dict(h=h, preds=(pred(negate=2),)),
        dict(h=h, preds=(pred(pad=1),)),
        dict(h=h, null_group=True),                                # null group
        dict(h=h, null_group=True, preds=()),
        dict(h=h, group=grp(width=0)),                             # the group column: width
        dict(h=h, group=grp(width=3)),
        dict(h=h, group=grp(width=16)),
        dict(h=h, group=grp(is_signed=2)),                         # ... flags and pads
        dict(h=h, group=grp(in_key=2)),
        dict(h=h, group=grp(pad=1)),
        dict(h=h, group=grp(pad2=1)),
        dict(h=h, group=grp(off=PAYLOAD - 3, width=4)),            # ... ends one byte past the payload
        dict(h=h, group=grp(off=PAYLOAD, width=1)),
        dict(h=h, group=grp(off=0xFFFFFFFF, width=8)),             # off + width wraps in 32 bits
        dict(h=h, group=grp(off=KEY_PAD - 3, width=4, in_key=1)),  # ... ends one byte past the key field
        dict(h=h, group=grp(off=KEY_PAD, width=1, in_key=1)),
        dict(h=h, group=grp(off=1, width=8, in_key=1)),
        dict(h=h, group=grp(off=0xFFFFFFFF, width=2, in_key=1)),
        dict(h=h, group=grp(n_groups=0)),                          # n_groups
        dict(h=h, group=grp(n_groups=GROUP_MAX + 1)),
        dict(h=h, group=grp(n_groups=0xFFFFFFFF)),
        dict(h=h, agg_width=3),                                    # the aggregate column
        dict(h=h, agg_width=16),
        dict(h=h, agg_off=PAYLOAD - 7, agg_width=8),
        dict(h=h, agg_off=PAYLOAD, agg_width=1),
        dict(h=h, agg_off=0xFFFFFFFF, agg_width=2),
        dict(h=h, agg_signed=2),
        dict(h=h, begin=2, end=1),                                 # leaf_begin > leaf_end
        dict(h=h, begin=END, end=5),
        dict(h=h, groups=None),                                    # null d_groups
        dict(h=h, groups=None, preds=(), agg_width=0),
    ]
    for kw in bad:
        assert stage.lib().stage_set_probe_tuning(h, 3, 0) == E_ARG  # leaves another message behind
        before = last_error()
        assert call(read_id=read_id, **kw) == E_ARG, kw
        msg = last_error()
        assert len(msg) > 0 and msg != before and b"stage_sync" not in msg, (kw, msg)


def test_errors_arrive_in_the_documented_order(unsynced):
    """two errors at once: the earlier one of the contract's list is the one reported"""
    h = unsynced.h
    order = [
        (dict(preds=(pred(width=3),)), b"predicate"),
        (dict(null_group=True), b"null group"),
        (dict(group=grp(width=3)), b"group column"),
        (dict(group=grp(n_groups=0)), b"n_groups"),
        (dict(agg_width=3), b"aggregate column"),
        (dict(begin=2, end=1), b"leaf_begin"),
        (dict(groups=None), b"d_groups"),
    ]
    for i, (first, word) in enumerate(order):
        for later, _ in order[i + 1:]:
            kw = dict(later)
            kw.update(first)
            if "null_group" in kw:
                kw.pop("group", None)
            assert call(h, **kw) == E_ARG, kw
            assert word in last_error(), (kw, last_error())


@pytest.mark.parametrize("read_id", [None, 7])
def test_valid_call_reaches_the_state_error(unsynced, read_id):
    h = unsynced.h
    cases = [
        dict(),
        dict(begin=3, end=3),                                      # an empty range
        dict(begin=5, end=1 << 40),                                # the leaf count is checked after the state
        dict(preds=(), null_preds=True),
        dict(agg_width=0), dict(agg_width=0, agg_off=1 << 30),     # counts only: no column to check
        dict(agg_off=PAYLOAD - 8, agg_width=8, agg_signed=1),
        dict(group=grp(off=PAYLOAD - 1, width=1)),                 # the payload's last byte
        dict(group=grp(off=PAYLOAD - 8, width=8, is_signed=1, base=-(1 << 63))),
        dict(group=grp(off=5, width=2, base=-3, is_signed=1, n_groups=8)),
        dict(group=grp(off=0, width=8, base=-3, n_groups=3)),      # an unsigned base as its bit pattern: 2^64 - 3
        dict(group=grp(off=0, width=8, in_key=1)),                 # the whole key field
        dict(group=grp(off=KEY_PAD - 1, width=1, in_key=1)),
        dict(group=grp(n_groups=1)), dict(group=grp(n_groups=GROUP_LDS_MAX)), dict(group=grp(n_groups=GROUP_LDS_MAX + 1)),
        dict(group=grp(n_groups=GROUP_MAX)),
    ]
    for kw in cases:
        assert call(h, read_id=read_id, **kw) == E_STATE, kw
        assert b"stage_sync" in last_error()


def test_group_tuning_arguments(unsynced):
    L = stage.lib()
    assert L.stage_set_scan_group_tuning(None, -1, -1) == E_ARG
    for lds_max, combine in ((-2, -1), (GROUP_LDS_MAX + 1, -1), (-1, -2), (-1, 65)):
        assert L.stage_set_scan_group_tuning(unsynced.h, lds_max, combine) == E_ARG
    for lds_max, combine in ((0, 0), (GROUP_LDS_MAX, 64), (-1, -1)):
        assert L.stage_set_scan_group_tuning(unsynced.h, lds_max, combine) == 0


def test_python_wrapper_reaches_the_c_entry_point(unsynced):
    G, P = stage.Group, stage.Pred
    assert G(3, 2, -3, 8, signed=True) == (3, 2, -3, 8, True, False)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_group_aggregate_device(None, None, [P(0, 4, 0, 10)], G(0, 1, 0, 4), (0, 4, True), 16)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_group_aggregate_device((0, 1), 9, (), G(0, 8, (1 << 64) - 3, 3), None, 16)
    with pytest.raises(stage.StageError, match="stage_sync"):
        unsynced.table_scan_group_aggregate_device(None, None, (), G(4, 4, 0, 16, in_key=True), None, 16)
    with pytest.raises(stage.StageError, match="null group"):
        unsynced.table_scan_group_aggregate_device(None, None, (), None, None, 16)
    with pytest.raises(stage.StageError, match="padded key"):
        unsynced.table_scan_group_aggregate_device(None, None, (), G(7, 2, 0, 4, in_key=True), None, 16)
    with pytest.raises(stage.StageError, match="n_groups"):
        unsynced.table_scan_group_aggregate_device(None, None, (), G(0, 1, 0, 0), None, 16)
    with pytest.raises(stage.StageError, match="d_groups"):
        unsynced.table_scan_group_aggregate_device(None, None, (), G(0, 1, 0, 4), None, None)
    with pytest.raises(ValueError):
        unsynced.table_scan_group_aggregate()
    assert stage.GroupAggregates._fields == ("count", "sum", "min", "max")


# ------------------------------------------------------------------------------------------
# the expectation helper, on a hand-written table

Hand = collections.namedtuple("Hand", "rows status offsets leaves")

U64, I64MIN, I64MAX = (1 << 64) - 1, -(1 << 63), (1 << 63) - 1
# (key byte 0, u8 at payload 0, i16 at 1, u64 at 3, i64 at 11, u32 at 19, status)
RECORDS = [
    (1, 10, -3, U64 - 2, I64MIN, 7, 1),
    (1, 11, -2, U64 - 1, I64MIN + 1, 1, 1),
    (2, 12, 4, U64, I64MAX, 9, 1),
    (2, 13, 5, U64 - 3, I64MAX - 2, 4, 1),       # 13 = base + n_groups of (10, 3): rest; U64 - 3: below its base
    (2, 9, -4, 0, 0, 100, 1),                    # 9: below base 10: rest
    (3, 10, -3, U64 - 2, I64MIN, 0xFFFFFFFF, 1),
    (3, 10, 0, 5, -1, 50, 3),                    # a version's image (ST_OLD)
    (4, 11, 1, U64, I64MAX - 1, 2, 0),           # no tuple: never takes part
    (4, 12, 4, 1 << 63, I64MAX, 3, 1),
    (5, 250, 32767, (1 << 63) - 1, I64MIN + 2, 6, 1),
    (5, 255, -32768, U64 - 1, 5, 8, 1),
    (6, 10, 2, U64 - 2, I64MIN, 11, 1),
]


def hand():
    rows = np.zeros((len(RECORDS), KEY_PAD + 23), np.uint8)
    for r, (k, a, b, c, d, e, _) in zip(rows, RECORDS):
        r[0] = k
        r[KEY_PAD] = a
        r[KEY_PAD + 1:KEY_PAD + 3] = np.frombuffer(int(b).to_bytes(2, "little", signed=True), np.uint8)
        r[KEY_PAD + 3:KEY_PAD + 11] = np.frombuffer(int(c).to_bytes(8, "little"), np.uint8)
        r[KEY_PAD + 11:KEY_PAD + 19] = np.frombuffer(int(d).to_bytes(8, "little", signed=True), np.uint8)
        r[KEY_PAD + 19:KEY_PAD + 23] = np.frombuffer(int(e).to_bytes(4, "little"), np.uint8)
    status = np.array([x[-1] for x in RECORDS], np.uint8)
    return Hand(rows, status, np.array([0, 5, 9, 12], np.uint64), 3)


def as_lists(res):
    return [[int(v) for v in x] for x in res]


def test_group_ids_do_not_wrap():
    assert group_ids(np.array([U64 - 3, U64 - 2, U64, 0, 2], np.uint64), U64 - 2, 3).tolist() == [3, 0, 2, 3, 3]
    assert group_ids(np.array([U64, 0], np.uint64), U64, GROUP_MAX).tolist() == [0, GROUP_MAX]
    assert group_ids(np.array([I64MIN, I64MIN + 7, I64MAX, -1], np.int64), I64MIN, 8).tolist() == [0, 7, 8, 8]
    assert group_ids(np.array([I64MAX - 2, I64MAX, I64MIN], np.int64), I64MAX - 2, 16).tolist() == [0, 2, 16]
    assert group_ids(np.array([-3, 4, 5, -4], np.int64), -3, 8).tolist() == [0, 7, 8, 8]
    assert group_ids(np.zeros(0, np.uint64), 0, 4).size == 0


def test_expect_helper_on_a_hand_written_table():
    e, G, P = hand(), stage.Group, stage.Pred
    u32 = (19, 4, False)
    # u8 column, base 10, 3 groups: 10 -> {7, 0xFFFFFFFF, 50, 11}, 11 -> {1}, 12 -> {9, 3}; rest {4, 100, 6, 8}
    assert as_lists(group_aggregate(e, KEY_PAD, [], G(0, 1, 10, 3), u32)) == [
        [4, 1, 2, 4], [7 + 0xFFFFFFFF + 50 + 11, 1, 12, 118], [7, 1, 3, 4], [0xFFFFFFFF, 1, 9, 100]]
    # counts alone; and under a predicate that keeps the u32 values <= 9
    assert as_lists(group_aggregate(e, KEY_PAD, [], G(0, 1, 10, 3), None)) == [[4, 1, 2, 4], [0] * 4, [0] * 4, [0] * 4]
    assert as_lists(group_aggregate(e, KEY_PAD, [P(19, 4, 0, 9)], G(0, 1, 10, 3), u32)) == [
        [1, 1, 2, 3], [7, 1, 12, 18], [7, 1, 3, 4], [7, 1, 9, 8]]
    # base 250, 16 groups: 250 and 255 reachable, 256.. are not -- identities; nine records in rest
    c, s, mn, mx = as_lists(group_aggregate(e, KEY_PAD, [], G(0, 1, 250, 16), u32))
    assert c == [1, 0, 0, 0, 0, 1] + [0] * 10 + [9] and s[0] == 6 and s[5] == 8 and s[6:16] == [0] * 10
    assert mn[1] == 0xFFFFFFFF and mx[1] == 0 and mn[6:16] == [0xFFFFFFFF] * 10 and mx[6:16] == [0] * 10
    # unsigned 8-byte column, base 2^64 - 3: three reachable groups; 2^64 - 4 and small values in rest
    c, s, mn, mx = as_lists(group_aggregate(e, KEY_PAD, [], G(3, 8, U64 - 2, 3), (3, 8, False)))
    assert c == [3, 2, 1, 5]
    assert s[:3] == [(3 * (U64 - 2)) % (1 << 64), (2 * (U64 - 1)) % (1 << 64), U64]   # sums wrap, ids do not
    assert mn[:3] == mx[:3] == [U64 - 2, U64 - 1, U64] and (mn[3], mx[3]) == (0, U64 - 3)
    # the same base with more groups than are reachable: identities past group 2
    c, s, mn, mx = as_lists(group_aggregate(e, KEY_PAD, [], G(3, 8, U64 - 2, 5), u32))
    assert c == [3, 2, 1, 0, 0, 5] and mn[3:5] == [0xFFFFFFFF] * 2 and mx[3:5] == [0, 0]
    # signed 8-byte column: base INT64_MIN, and base INT64_MAX - 2 (8 groups, three reachable)
    c, s, mn, mx = as_lists(group_aggregate(e, KEY_PAD, [], G(11, 8, I64MIN, 3, signed=True), (11, 8, True)))
    assert c == [3, 1, 1, 6] and s[0] == (3 * I64MIN) % (1 << 64) - (1 << 64) and mn[0] == mx[0] == I64MIN
    assert (s[2], mn[2], mx[2]) == (I64MIN + 2,) * 3 and (mn[3], mx[3]) == (-1, I64MAX)
    c, s, mn, mx = as_lists(group_aggregate(e, KEY_PAD, [], G(11, 8, I64MAX - 2, 8, signed=True), (1, 2, True)))
    assert c == [1, 0, 2] + [0] * 5 + [8] and (s[0], s[2]) == (5, 8) and mn[1] == 32767 and mx[1] == -32768
    # signed 2-byte column, base -3, 8 groups: -3 .. 4; 5, -4, 32767 and -32768 in rest
    c, s, mn, mx = as_lists(group_aggregate(e, KEY_PAD, [], G(1, 2, -3, 8, signed=True), (1, 2, True)))
    assert c == [2, 1, 0, 1, 0, 1, 0, 2, 4] and s == [-6, -2, 0, 0, 0, 2, 0, 8, 5 - 4 + 32767 - 32768]
    assert (mn[8], mx[8]) == (-32768, 32767) and (mn[2], mx[2]) == (32767, -32768)
    # a key byte as the group column; leaves [1, 3) alone; an empty range
    assert as_lists(group_aggregate(e, KEY_PAD, [], G(0, 1, 1, 6, in_key=True), None))[0] == [2, 3, 2, 1, 2, 1, 0]
    assert as_lists(group_aggregate(e, KEY_PAD, [], G(0, 1, 1, 6, in_key=True), None, 1, 3))[0] == [0, 0, 2, 1, 2, 1, 0]
    c, s, mn, mx = as_lists(group_aggregate(e, KEY_PAD, [], G(0, 1, 1, 2, in_key=True), (1, 2, True), 2, 2))
    assert (c, s, mn, mx) == ([0] * 3, [0] * 3, [32767] * 3, [-32768] * 3)
    # dtypes, and the fold back to the ungrouped aggregate
    res = group_aggregate(e, KEY_PAD, [], G(0, 1, 10, 3), (11, 8, True))
    assert [x.dtype for x in res] == [np.uint64, np.int64, np.int64, np.int64]
    vals = [d for (_, _, _, _, d, _, st) in RECORDS if st]
    total = sum(vals) % (1 << 64)
    assert folded(res, (11, 8, True)) == (11, total - (1 << 64) if total >> 63 else total, I64MIN, I64MAX)
    res = group_aggregate(e, KEY_PAD, [], G(0, 1, 10, 3), u32)
    assert [x.dtype for x in res] == [np.uint64] * 4
    assert folded(res, u32) == (11, sum(x[5] for x in RECORDS if x[6]), 1, 0xFFFFFFFF)
    assert folded(group_aggregate(e, KEY_PAD, [], G(0, 1, 10, 3), None), None) == (11, 0, 0, 0)
