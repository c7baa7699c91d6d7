"""Expected results of the filtered whole-table scans (stage_table_scan_where, _where_window,
stage_table_scan_aggregate), from the oracle alone -- TEST INFRASTRUCTURE ONLY.

The unfiltered expectation is table_scan_expect's (raw_expect / snapshot_expects: the oracle's leaf
blocks and its index_scan); numpy does the rest.  A column's values are the row bytes
rows[:, key_pad + off : key_pad + off + width] viewed little-endian and sign- or zero-extended; a
record matches when it yields a tuple (status != 0) and every predicate holds; the aggregates are
Python integers, the sum reduced modulo 2^64.  Each record's (leaf, slot) comes from the oracle's
leaf blocks, parsed as table_scan_expect.parse_blocks parses them: the live slot indices in slot
order, the snapshot set being the visible subset."""
import numpy as np

import stage
from table_scan_expect import M_VISIBLE


def domain(width, signed):
    """-> (smallest, largest) value of the column's domain"""
    bits = 8 * width
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)


def column(rows, key_pad, off, width, signed):
    """-> the column's extended values, int64 (signed) or uint64 [N]"""
    raw = np.ascontiguousarray(rows[:, key_pad + off:key_pad + off + width])
    assert raw.shape[1] == width, (rows.shape, key_pad, off, width)
    v = raw.view(f"<{'i' if signed else 'u'}{width}").reshape(-1)
    return v.astype(np.int64 if signed else np.uint64)


def holds(values, pred):
    """one predicate on a column's values: lo <= x <= hi (Python-integer bounds in the column's
    64-bit domain), or not"""
    lo, hi = pred.lo, pred.hi
    dlo, dhi = domain(8, pred.signed)
    assert dlo <= lo <= dhi and dlo <= hi <= dhi, pred
    t = np.int64 if pred.signed else np.uint64
    m = (values >= t(lo)) & (values <= t(hi))
    return ~m if pred.negate else m


def match_mask(e, key_pad, preds):
    """the records of expectation e that match: a tuple, and every predicate"""
    m = e.status != stage.ST_NOT_FOUND
    for p in preds:
        m = m & holds(column(e.rows, key_pad, p.off, p.width, p.signed), p)
    return m


def raw_slots(orc, kwords=1):
    """(leaf << 16) | slot of raw mode's records: the slots below the record count whose meta word
    is non-zero, per leaf block in key order (the parse of table_scan_expect.parse_blocks)"""
    blocks, _, _ = orc.export_leaf_images(kwords=kwords)
    out = []
    for leaf, b in enumerate(blocks):
        status = int(b[32:40].view(np.uint64)[0])
        cnt = (status >> 44) & 0xFFFF
        words = b[40:40 + 24 * cnt].reshape(cnt, 24)[:, :8].copy().view(np.uint64).reshape(-1)
        out.append((np.uint64(leaf) << np.uint64(16)) | np.nonzero(words != 0)[0].astype(np.uint64))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def snapshot_slots(raw, slots, key_width):
    """the visible subset, the rule of table_scan_expect.snapshot_expects"""
    klen = ((raw.meta & np.uint64(0x2FFF << 48)) >> np.uint64(48)).astype(np.int64)
    vis = (raw.meta & np.uint64(M_VISIBLE)) != 0
    if key_width:
        vis &= klen == key_width
    return slots[vis]


class Filtered:
    """the matching records of one mode's expectation e, compacted: Expect's interface (counts =
    matches per leaf, offsets, meta, status, rows, range()) plus slots, and the mask over e's
    records; the records are gathered from e when asked for"""

    def __init__(self, e, slots, mask):
        leaf_of = np.repeat(np.arange(e.leaves), e.counts)
        self.e, self.all_slots, self.mask, self.idx = e, slots, mask, np.nonzero(mask)[0]
        self.counts = np.bincount(leaf_of[mask], minlength=e.leaves).astype(np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)
        assert int(self.offsets[-1]) == self.idx.size

    leaves = property(lambda self: self.counts.size)
    meta = property(lambda self: self.e.meta[self.idx])
    status = property(lambda self: self.e.status[self.idx])
    rows = property(lambda self: self.e.rows[self.idx])
    slots = property(lambda self: self.all_slots[self.idx])

    def range(self, a, b):
        """-> count, offsets [b - a + 1], meta, status, rows, slots of the matches in leaves [a, b)"""
        lo, hi = int(self.offsets[a]), int(self.offsets[b])
        i = self.idx[lo:hi]
        return (hi - lo, self.offsets[a:b + 1] - np.uint64(lo), self.e.meta[i], self.e.status[i], self.e.rows[i],
                self.all_slots[i])


def aggregate(e, key_pad, preds, agg, a=0, b=None):
    """-> (count, sum, min, max) over the matches in leaves [a, b) as Table.table_scan_aggregate
    returns them: Python ints in the column's domain, the sum modulo 2^64 (a signed column's as an
    int64), the identities when nothing matches; agg None: the count and zeros"""
    b = e.leaves if b is None else b
    lo, hi = int(e.offsets[a]), int(e.offsets[b])
    m = match_mask(e, key_pad, preds)[lo:hi]
    count = int(m.sum())
    if agg is None:
        return count, 0, 0, 0
    off, width, signed = agg
    vals = [int(v) for v in column(e.rows[lo:hi], key_pad, off, width, signed)[m]]
    total = sum(vals) % (1 << 64)
    if signed and total >= 1 << 63:
        total -= 1 << 64
    dlo, dhi = domain(width, signed)
    return count, total, min(vals, default=dhi), max(vals, default=dlo)
