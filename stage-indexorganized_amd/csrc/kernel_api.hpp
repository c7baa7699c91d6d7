// kernel_api.hpp -- launchers of the gfx950 kernels (probe.hip, scan.hip, table_scan.hip,
// aux_kernels.hip), called by the host side.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "stage_core.hpp"

namespace stage {

// same bytes as stage_probe_out (include/stage_hip.h)
struct alignas(16) stage_probe_out_dev {
    uint32_t w[8];
};

// device copy of ImageDesc (host_table.hpp)
struct alignas(8) ImageDescDev {
    uint64_t key_le;
    uint64_t arg;
    uint32_t kind;
    uint32_t mode;
};

// the point probe's two forms for fixed-width keys of at most 8 bytes in 64- / 128-slot leaves:
// probe_kernel (a wave per probe) or probe_rows_kernel (front end a lane per probe, rows wave-wide;
// taken at group 8 and nontemporal stores only).  Mirrors of STAGE_PROBE_FORM_* (include/stage_hip.h).
constexpr int kProbeFormWave = 0, kProbeFormLane = 1;
struct ProbeTuning {
    int group = 8;         // probes per wave in flight (swept: 8 > 4 > 2 > 1 at 100M rows)
    int max_blocks = 0;    // 0 = default grid cap (16384 blocks of 256 threads)
    int store = 1;         // output stores: 0 temporal, 1 nontemporal, 2 write-through (sc1)
    int status_bytes = 32; // status record: 32 (stage_probe_out) or 16 (stage_probe_out16)
    int form = kProbeFormLane; // stage_set_probe_form (LANE measured faster at every shape)
};
constexpr int kProbeRows = 16;  // probe_rows_kernel's rows in flight per wave (swept: 16 > 8)

hipError_t launch_resolve(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t n, int le_child,
                          uint32_t *out, hipStream_t s);
// d_n (optional, the split-probe tables only -- wide keys or leaves above 128 slots): the batch's
// size lives on the device (written by an earlier kernel of the stream); n is its upper bound and
// sizes the grid, shape_n (0 = n) the expected size that picks the launch shape
hipError_t launch_probe(const DevTable &t, const uint64_t *keys, const uint16_t *lens, const uint32_t *rids,
                        const uint32_t *leaf_in, uint64_t n, stage_probe_out_dev *out, uint8_t *recs, hipStream_t s,
                        const ProbeTuning &tune, const uint64_t *d_n = nullptr, uint64_t shape_n = 0);
// launch_probe that delivers, instead of each probe's row, bytes [row_off, row_off + len) of it
// (row_off = key pad + payload offset; row_off + len within the heap row, else
// hipErrorInvalidValue): win holds n windows of (len + 15) & ~15 bytes, zero past len and zero
// for a probe that yields no tuple; the status records are launch_probe's.  probe_kernel's
// geometries run one fused launch (probe_window_kernel, tune.max_blocks and tune.status_bytes
// apply, tune.group and tune.store do not); the lane / split geometries run launch_probe without
// rows and then window_gather_kernel on the same stream (32-B records).
hipError_t launch_probe_window(const DevTable &t, const uint64_t *keys, const uint16_t *lens, const uint32_t *rids,
                               const uint32_t *leaf_in, uint64_t n, uint32_t row_off, uint32_t len,
                               stage_probe_out_dev *out, uint8_t *win, hipStream_t s, const ProbeTuning &tune);
// launch_probe with no read id (status records only) that also evaluates each hit at the read
// ids mrids[0..mnq) and sets missed[q] when a probe produces no tuple at read id q (the miss pass
// of launch_revisit_segments, folded in).  The lane-probe tables only (probe_missed_supported:
// wide fixed-width keys or 8-byte keys in leaves above 128 slots, leaves of at most 256 slots);
// otherwise hipErrorInvalidValue and nothing is launched.
bool probe_missed_supported(const DevTable &t);
hipError_t launch_probe_missed(const DevTable &t, const uint64_t *keys, uint64_t n, stage_probe_out_dev *out,
                               hipStream_t s, const ProbeTuning &tune, const uint64_t *d_n, uint64_t shape_n,
                               const uint32_t *mrids, uint32_t mnq, int32_t *missed);
// fan-out probe (sharded front-end, dist.hip): probe i's status record and row are stored at
// every caller position flist[k], k in [fan[i].lo, fan[i].hi) (flist null: k itself; fan null:
// the one position flist[i]).  Tables of the YCSB geometry only (fixed-width 8-byte keys, 64-slot
// leaves, rows <= 1024 B).
struct alignas(8) FanRange {
    uint32_t lo, hi;
};
// dest (device memory, optional): the probes fall in dest->nseg consecutive segments (segment g
// ends at probe dest->end[g], launch-relative), each with its own output buffers out[g] / recs[g]
// in place of out / recs -- one launch for the requests of several callers (STAGE_REPLY_DIRECT)
constexpr int kFanDests = 64;
struct FanDest {
    uint32_t nseg;
    uint32_t end[kFanDests];
    stage_probe_out_dev *out[kFanDests];
    uint8_t *recs[kFanDests];
};
bool probe_fanout_supported(const DevTable &t);
hipError_t launch_probe_fanout(const DevTable &t, const uint64_t *keys, const uint32_t *rids, uint64_t n,
                               const FanRange *fan, const uint32_t *flist, stage_probe_out_dev *out, uint8_t *recs,
                               hipStream_t s, const ProbeTuning &tune, const FanDest *dest = nullptr);
struct ScanTuning {
    int max_blocks = 0;  // 0 = default grid cap (16384 blocks of 256 threads)
};

// row_status != nullptr: IndexScanExecutor range semantics (per-record visibility for
// rids[i]); row_status[i*scan_size + j] = ST_LATEST / ST_OLD / ST_NOT_FOUND (row zeroed)
hipError_t launch_scan(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t n, uint32_t scan_size,
                       uint32_t *counts, uint8_t *recs, hipStream_t s, const ScanTuning &tune,
                       const uint32_t *rids = nullptr, uint8_t *row_status = nullptr);
// launch_scan that delivers, instead of each scanned record's row, bytes [row_off, row_off + len)
// of it (row_off = key pad + payload offset; row_off + len within the heap row, else
// hipErrorInvalidValue): win[(i*scan_size + j) * ((len + 15) & ~15)] is record j of scan i, zero
// past len and all zero where the row form zeroes the row; positions j >= counts[i] are not
// written.  row_keys (optional): the row's first key_pad bytes at (i*scan_size + j) * key_pad.
// counts and row_status are launch_scan's; the same geometries, grid rule and tuning.  Kernels of
// their own (scan_window_kernel, scan_window_kernel_compact): launch_scan's code is untouched.
hipError_t launch_scan_window(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t n,
                              uint32_t scan_size, uint32_t row_off, uint32_t len, uint32_t key_pad, uint32_t *counts,
                              uint8_t *win, uint8_t *row_keys, hipStream_t s, const ScanTuning &tune,
                              const uint32_t *rids = nullptr, uint8_t *row_status = nullptr);
// Whole-table scan: every record of leaves [leaf0, leaf0 + nl) in leaf and slot order, record k of
// the range at output position k.  snapshot false: ScanLeafNode -- the slots below the leaf's
// record count whose meta word is non-zero, the current image, status ST_LATEST.  snapshot true:
// the slots of the head's visible masks, each evaluated at read id `rid` like launch_scan's
// row_status form (ST_NOT_FOUND: row / window / key zero; the slot still takes a position).
// len == 0: rows of t.stride bytes to o.recs; len != 0: windows [row_off, row_off + len) of
// (len + 15) & ~15 bytes to o.win and, optionally, the rows' first key_pad bytes to o.row_keys
// (launch_scan_window's conventions).  o.count[0] = the records of the range; only positions
// < o.max_records are written (0: count only, no record buffer needed).  o.leaf_offsets
// (optional, nl + 1 words): the position of each leaf's first record, then the count.
// scratch: table_scan_scratch_bytes(nl) bytes, 8-B aligned, used until the launches end on s.
// Three launches, none of which waits for another workgroup; tune's grid cap applies to each.
struct TableScanOut {
    uint64_t max_records;
    uint64_t *count;
    uint64_t *leaf_offsets;
    uint8_t *recs;
    uint8_t *win;
    uint8_t *row_keys;
    uint64_t *row_meta;
    uint8_t *row_status;
};
uint64_t table_scan_scratch_bytes(uint64_t nl);
hipError_t launch_table_scan(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                             uint32_t row_off, uint32_t len, uint32_t key_pad, const TableScanOut &o, uint8_t *scratch,
                             hipStream_t s, const ScanTuning &tune);
// Filtered whole-table scans.  A record of launch_table_scan's set (same range, same mode) matches
// when it yields a tuple (status != ST_NOT_FOUND) and every predicate holds on its heap row: the
// column of `width` (1, 2, 4, 8) little-endian bytes at row byte `src` (key pad + payload offset),
// sign- or zero-extended, lies in [lo, hi] (negate: does not).  The predicates travel by value
// in the kernel arguments.
constexpr uint32_t kScanPredMax = 4;
constexpr bool scan_column_width(uint32_t w) { return w == 1 || w == 2 || w == 4 || w == 8; }
struct ScanPred {  // 24 B
    uint32_t src;
    uint8_t width, is_signed, negate, pad;
    int64_t lo, hi;  // the column's domain (unsigned column: the uint64 bit patterns)
};
struct ScanPreds {
    uint32_t n, pad;
    ScanPred p[kScanPredMax];
};
// launch_table_scan's outputs for the matching records alone, compacted in the same order (o's
// fields and every rule of launch_table_scan), row_slot (optional): (leaf << 16) | slot per
// record.  scratch: table_scan_where_scratch_bytes(nl, t.cap) bytes (tile offsets, one bit per
// slot, matches per leaf), 8-B aligned.  Four launches (match, tile sums, then launch_table_scan's
// offsets and emit kernels: one launcher body and one emit kernel serve both).
uint64_t table_scan_where_scratch_bytes(uint64_t nl, uint32_t cap);
hipError_t launch_table_scan_where(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                                   const ScanPreds &preds, uint32_t row_off, uint32_t len, uint32_t key_pad,
                                   const TableScanOut &o, uint64_t *row_slot, uint8_t *scratch, hipStream_t s,
                                   const ScanTuning &tune);
// agg[0..3] = {count, sum modulo 2^64, min, max} of the matching records' column (agg_src,
// agg_width, agg_signed), the words of stage_scan_agg; agg_width 0: the count alone (sum, min,
// max zero).  Integer and order-free, so the result does not depend on the grid.  scratch:
// table_scan_aggregate_scratch_bytes(nl, tune) bytes (one 32-B partial per block).
uint64_t table_scan_aggregate_scratch_bytes(uint64_t nl, const ScanTuning &tune);
hipError_t launch_table_scan_aggregate(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                                       const ScanPreds &preds, uint32_t agg_src, uint32_t agg_width, bool agg_signed,
                                       uint64_t *agg, uint8_t *scratch, hipStream_t s, const ScanTuning &tune);
// launch_table_scan_aggregate per group: groups[4 g .. 4 g + 3] = the words of stage_scan_agg over
// the matching records whose group column (grp.src, grp.width, grp.is_signed) holds grp.base + g,
// g < grp.n, in the integers (nothing wraps); entry grp.n = every other matching record.  An entry
// without a record holds count 0, sum 0 and the identities of launch_table_scan_aggregate.
// grp.n <= the LDS tier's bound: a table per workgroup in LDS (32 (grp.n + 1) bytes of dynamic
// shared memory), left in scratch and folded by a second launch; above: a fill, the scan with
// global atomics straight on groups[], a finish launch.  Stream order, one launch for an empty
// range.  scratch: table_scan_group_scratch_bytes(nl, grp.n, tune, gt) bytes (one table per
// workgroup of the LDS tier, at most 64 MiB; 0 in the global tier), 8-B aligned.  Integer and
// order-free: the same bytes from either tier and any grid.
constexpr uint32_t kGroupMax = 1u << 24;   // STAGE_GROUP_MAX
constexpr uint32_t kGroupLdsMax = 256;     // STAGE_GROUP_LDS_MAX
struct ScanGroupSpec {
    uint32_t src, width;  // the group column at row byte src (key bytes lie below the key pad)
    bool is_signed;
    uint64_t base;        // the column's domain (unsigned column: the uint64 bit pattern)
    uint32_t n;           // 1 .. kGroupMax
};
struct ScanGroupTuning {
    int lds_max = -1;  // groups the LDS tier takes: -1 = kGroupLdsMax, 0 = the global tier always
    int combine = -1;  // distinct groups of a wave's 64 records combined before the update: -1 =
                       // by tier (table_scan.hip), 0 = none, 64 = all
};
uint64_t table_scan_group_scratch_bytes(uint64_t nl, uint32_t n_groups, const ScanTuning &tune, const ScanGroupTuning &gt);
hipError_t launch_table_scan_group(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                                   const ScanPreds &preds, const ScanGroupSpec &grp, uint32_t agg_src, uint32_t agg_width,
                                   bool agg_signed, uint64_t *groups, uint8_t *scratch, hipStream_t s,
                                   const ScanTuning &tune, const ScanGroupTuning &gt);
// two single scans (no read id) of two tables in one launch, the same records as launch_scan of
// each (n = 1): 8-byte keys, leaves of the same size above 128 slots, 1..63 records each
// (scan_pair_supported; otherwise hipErrorInvalidValue and nothing is launched)
hipError_t launch_scan_pair(const DevTable &t0, const uint64_t *k0, uint32_t sz0, uint32_t *c0, uint8_t *r0,
                            const DevTable &t1, const uint64_t *k1, uint32_t sz1, uint32_t *c1, uint8_t *r1,
                            hipStream_t s);
bool scan_pair_supported(const DevTable &t0, uint32_t sz0, const DevTable &t1, uint32_t sz1);
// IndexScanExecutor range scan (fixed-width tables) kept only up to its first produced tuple
// whose key starts with the start key's first `words` order words: img_out[i] = its heap row
// (0xFFFFFFFF if none), st_out[i] = ST_LATEST / ST_OLD / ST_NOT_FOUND
hipError_t launch_scan_first(const DevTable &t, const uint64_t *keys, uint64_t n, uint32_t scan_size,
                             const uint32_t *rids, uint32_t words, uint32_t *img_out, uint8_t *st_out, hipStream_t s,
                             const ScanTuning &tune);
// request ring of the resident reader (all arrays in pinned, device-mapped host memory except
// pos, which is device memory of `waves` words initialised to 0)
// one request: {key bytes (LE), read id, tag}, tag = (ticket + 1) << 4 | key length, written by
// the caller last (release); 16-B aligned, so one device load sees the tag with its key
struct alignas(16) ReaderReq {
    uint64_t key;
    uint32_t rid;
    uint32_t tag;
};
struct ReaderRing {
    const ReaderReq *req;      // [slots]
    uint32_t *done;            // [slots] ticket + 1 once its results are in place (device)
    stage_probe_out_dev *out;  // [slots]
    uint8_t *rows;             // [slots * stride]
    const uint32_t *stop;      // non-zero: instances end at their next poll
    uint64_t *pos;             // [waves] next own ticket index k of each wave, kept across instances
    uint32_t slots;            // multiple of 64 * waves
    uint32_t waves;
    uint64_t life_ticks;       // lifetime of one instance in real-time counter ticks
    uint32_t *ident;           // [slots * 2] {location handle, next handle} of each read (stage_probe_ident)
};
hipError_t launch_resident_reader(const DevTable &t, const ReaderRing &g, hipStream_t s);
// the probes of one key set at several read ids: base[0..n) holds probe results (any read id) of
// n keys; out[q * n + i] = the result of key i at rids[q], q < nq -- the hit slot is the same for
// every read id (SearchRecordMeta does not depend on it), only the visibility walk is redone;
// perm (may be null): base[i] is key perm[i]'s result, written to out[q * n + perm[i]]
// d_n (optional): the key count on the device (n its upper bound); out is then [nq][*d_n]
hipError_t launch_revisit(const DevTable &t, const stage_probe_out_dev *base, uint64_t n, const uint32_t *rids,
                          uint32_t nq, const uint32_t *perm, stage_probe_out_dev *out, hipStream_t s,
                          const uint64_t *d_n = nullptr);
// launch_revisit folded, for n probes cut into segments (segment k = base[seg_off[k], + seg_cnt[k])):
// missed[q] |= 1 when any probe yields no record (LATEST / COPY / OLD) at rids[q], and
// last[q * nseg + k] = segment k's last probe at rids[q] (left as it is for an empty segment) --
// the n * nq results themselves are never stored
hipError_t launch_revisit_segments(const DevTable &t, const stage_probe_out_dev *base, uint64_t n,
                                   const uint64_t *seg_off, const uint32_t *seg_cnt, uint32_t nseg,
                                   const uint32_t *rids, uint32_t nq, stage_probe_out_dev *last, int32_t *missed,
                                   hipStream_t s, const uint64_t *d_n = nullptr, const uint64_t *d_nseg = nullptr);
// stage_probe_batch_ex: after launch_probe of the same batch, re-answer the probes with fu[i] != 0
// as BTree::Read(..., is_for_update = true) (status record and, if recs, the row); 32-B records
hipError_t launch_for_update(const DevTable &t, const uint8_t *fu, const uint32_t *rids, uint64_t n,
                             stage_probe_out_dev *out, uint8_t *recs, hipStream_t s);
// stage_probe_ident: {location handle, next handle} of each probe's hit slot (two u32 per probe)
hipError_t launch_ident(const DevTable &t, const stage_probe_out_dev *out, uint64_t n, uint32_t *ident, hipStream_t s);
hipError_t launch_murmur(const void *keys, uint32_t key_len, uint32_t key_stride, uint64_t seed, uint64_t n,
                         uint64_t *out, hipStream_t s);
hipError_t launch_fill(uint8_t *heap, uint32_t stride, uint32_t payload_size, uint32_t row_bytes,
                       const ImageDescDev *descs, const uint8_t *arena, uint64_t first, uint64_t count,
                       uint64_t ident_rowid0, uint32_t ident_key_width, int ident_mode, hipStream_t s);
hipError_t launch_patch(uint8_t *head, uint64_t *okey, SlotInfo *slot, uint32_t head_bytes, uint32_t cap, uint32_t kw,
                        const uint32_t *head_leaf, const void *head_src, uint64_t nhead, const uint64_t *slot_idx,
                        const SlotInfo *slot_src, const uint64_t *words, uint64_t nslot, hipStream_t s);

}  // namespace stage
