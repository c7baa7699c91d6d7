"""Expected results of the whole-table scans (stage_table_scan / stage_table_scan_window), from the
oracle alone -- TEST INFRASTRUCTURE ONLY.

Raw mode (ScanLeafNode): the oracle's reference-format leaf blocks in key order
(OracleTree.export_leaf_images) are parsed here -- the block layout of stage_hip.h's leaf-snapshot
comment, the StatusWord / RecordMetadata fields of the M_* and st_count macros at the top of
oracle/stage_oracle.c: record count = StatusWord bits 44-59 (the u64 at byte 32), slot i's meta
word = the u64 at byte 40 + 24 i, the record = [key padded to 8][payload] at the word's offset
(bits 32-47).  Every slot below the record count whose meta word is non-zero is one record.

Snapshot mode: the slots the range iterator considers are the visible ones (visible bit, and on a
fixed-width table the table's key length), in the same leaf and slot order; what each yields at a
read id is the oracle's index_scan from the smallest key, matched to the slots by key order."""
import functools

import numpy as np

import oracle_lib as O

M_VISIBLE = 1 << 62
LAST = 0xFFFFFFFE


def parse_blocks(blocks, row, payload):
    """-> records per leaf [L], meta words [N], rows [N, row] in leaf and slot order"""
    counts, metas, rows = [], [], []
    for b in blocks:
        status = int(b[32:40].view(np.uint64)[0])
        cnt = (status >> 44) & 0xFFFF
        words = b[40:40 + 24 * cnt].reshape(cnt, 24)[:, :8].copy().view(np.uint64).reshape(-1)
        live = np.nonzero(words != 0)[0]
        counts.append(live.size)
        for i in live:
            m = int(words[i])
            off = (m >> 32) & 0xFFFF
            klen = (m & (0x2FFF << 48)) >> 48
            assert (klen + 7) // 8 * 8 + payload == row, (klen, payload, row)
            metas.append(m)
            rows.append(b[off:off + row])
    rows = np.array(rows, np.uint8).reshape(len(metas), row)
    return np.array(counts, np.int64), np.array(metas, np.uint64), rows


class Expect:
    """one mode's records of the whole table: per-leaf counts, and per record meta, status, row"""

    def __init__(self, counts, meta, status, rows):
        self.counts, self.meta, self.status, self.rows = counts, meta, status, rows
        self.offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        assert int(self.offsets[-1]) == meta.size == status.size == rows.shape[0]

    @property
    def leaves(self):
        return self.counts.size

    def range(self, a, b):
        """-> count, offsets [b - a + 1], meta, status, rows of leaves [a, b)"""
        lo, hi = int(self.offsets[a]), int(self.offsets[b])
        return hi - lo, self.offsets[a:b + 1] - np.uint64(lo), self.meta[lo:hi], self.status[lo:hi], self.rows[lo:hi]


def key_of(row, meta, key_pad):
    klen = (int(meta) & (0x2FFF << 48)) >> 48
    return row[:klen].tobytes()


def raw_expect(orc, kwords=1):
    blocks, _, _ = orc.export_leaf_images(kwords=kwords)
    counts, meta, rows = parse_blocks(blocks, orc.row, orc.payload_size)
    return Expect(counts, meta, np.full(meta.size, 1, np.uint8), rows)  # every record ST_LATEST


def snapshot_expects(orc, raw, key_width, rids):
    """-> {rid: Expect}.  The considered slots are raw's visible ones; their order by key
    (KeyCompare) is the order of the oracle's index_scan, which gives each its status and row."""
    klen = ((raw.meta & np.uint64(0x2FFF << 48)) >> np.uint64(48)).astype(np.int64)
    vis = (raw.meta & np.uint64(M_VISIBLE)) != 0
    if key_width:
        vis &= klen == key_width
    leaf_of = np.repeat(np.arange(raw.leaves), raw.counts)
    counts = np.bincount(leaf_of[vis], minlength=raw.leaves).astype(np.int64)
    pos = np.nonzero(vis)[0]
    keys = [key_of(raw.rows[p], raw.meta[p], orc.key_pad) for p in pos]
    assert len(set(keys)) == len(keys), "a key is visible twice"
    order = sorted(range(len(keys)), key=functools.cmp_to_key(lambda i, j: O.key_compare(keys[i], keys[j])))
    out = {}
    for rid in rids:
        # One index_scan from the smallest key with scan_size above the record count -- unless the
        # reference's iterator ends early: after a leaf's last record it re-descends from that key
        # with le_child = false, and where the leaf's largest key was deleted that leads back into
        # the same leaf, whose first record is the key itself: item_vec.clear(), the scan is over
        # (scan_one_ex).  The scan is then restarted at the next key in key order, so every
        # considered slot still gets the oracle's own (status, row).
        ost, orows, done = [], [], 0
        while done < len(keys):
            first = keys[order[done]]
            c, r, s = orc.index_scan(first, len(first), len(keys) - done + 50, rid)
            assert 1 <= c <= len(keys) - done, (rid, done, c, len(keys))
            ost.append(s)
            orows.append(r)
            done += c
        assert len(ost) <= 1 + len(keys) // 100, "the oracle's scan restarts too often to be one scan"
        ost, orows = np.concatenate(ost), np.concatenate(orows)
        status = np.zeros(len(keys), np.uint8)
        rows = np.zeros((len(keys), orc.row), np.uint8)
        status[order], rows[order] = ost, orows
        produced = status != 0
        got = [rows[i, :len(keys[i])].tobytes() for i in np.nonzero(produced)[0]]
        assert got == [keys[i] for i in np.nonzero(produced)[0]], "the oracle's records are not in key order"
        assert not rows[~produced].any()
        out[rid] = Expect(counts, raw.meta[vis], status, rows)
    return out
