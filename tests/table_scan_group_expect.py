"""Expected results of the grouped aggregate (stage_table_scan_group_aggregate), from the oracle
alone -- TEST INFRASTRUCTURE ONLY.

The record set and the columns are table_scan_where_expect's (match_mask / column over the
oracle's unfiltered expectation); an in_key group column is column(rows, 0, off, ...), the row's
own key bytes.  Group ids are Python integers, value - base, so nothing wraps: a record belongs to
group g iff its extended value equals base + g with 0 <= g < n_groups, else to the rest group
n_groups.  Sums are reduced modulo 2^64; an entry without a record holds the identities."""
import numpy as np

from table_scan_where_expect import column, domain, match_mask


def group_ids(values, base, n_groups):
    """-> the group index of each extended value (Python-integer arithmetic), rest = n_groups"""
    d = np.asarray(values).astype(object) - int(base)  # Python ints: no width, no wrap
    if d.size == 0:
        return np.zeros(0, np.int64)
    inside = np.asarray(d >= 0, bool) & np.asarray(d < n_groups, bool)
    return np.where(inside, d, n_groups).astype(np.int64)


def fold(values, signed_sum, dlo, dhi):
    """(count, sum modulo 2^64 -- as an int64 when signed_sum --, min, max) of Python ints"""
    total = sum(values) % (1 << 64)
    if signed_sum and total >= 1 << 63:
        total -= 1 << 64
    return len(values), total, min(values, default=dhi), max(values, default=dlo)


def group_aggregate(e, key_pad, preds, group, agg, a=0, b=None):
    """-> (count, sum, min, max): numpy arrays of group.n_groups + 1 entries as
    Table.table_scan_group_aggregate returns them over the matches in leaves [a, b) -- count
    uint64; sum, min, max int64 (a signed aggregate column) or uint64; agg None: counts and zeros"""
    b = e.leaves if b is None else b
    lo, hi = int(e.offsets[a]), int(e.offsets[b])
    m = match_mask(e, key_pad, preds)[lo:hi]
    rows = e.rows[lo:hi][m]
    n = group.n_groups + 1
    gcol = column(rows, 0 if group.in_key else key_pad, group.off, group.width, group.signed)
    ids = group_ids(gcol, group.base, group.n_groups)
    count = np.bincount(ids, minlength=n).astype(np.uint64)
    signed = agg is not None and bool(agg[2])
    t = np.int64 if signed else np.uint64
    if agg is None:
        z = np.zeros(n, np.uint64)
        return count, z, z.copy(), z.copy()
    off, width, _ = agg
    vals = [int(v) for v in column(rows, key_pad, off, width, signed)]
    dlo, dhi = domain(width, signed)
    per = [[] for _ in range(min(n, 1 + int(ids.max(initial=0))))]
    for g, v in zip(ids.tolist(), vals):
        per[g].append(v)
    s, mn, mx = np.zeros(n, t), np.full(n, dhi, t), np.full(n, dlo, t)
    for g, vs in enumerate(per):
        if vs:
            c, s[g], mn[g], mx[g] = fold(vs, signed, dlo, dhi)
            assert c == int(count[g])
    return count, s, mn, mx


def folded(res, agg):
    """the n_groups + 1 entries folded into stage_table_scan_aggregate's (count, sum, min, max)"""
    count, s, mn, mx = res
    if agg is None:
        return int(count.sum(dtype=np.uint64)), 0, 0, 0
    with np.errstate(over="ignore"):  # uint64 addition is addition modulo 2^64
        total = int(np.sum(np.asarray(s).astype(np.uint64), dtype=np.uint64))
    if agg[2] and total >= 1 << 63:
        total -= 1 << 64
    return int(count.sum(dtype=np.uint64)), total, int(mn.min()), int(mx.max())
