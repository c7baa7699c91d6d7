// table_scan.hip -- gfx950 kernels of the whole-table scan and of its filtered forms (a count or a
// match pass, the offsets, one emit pass for both), of the aggregate and of the grouped aggregate,
// and their launchers.
#include "kernel_api.hpp"
#include "launch_util.hpp"
#include "row_store.hpp"
#include "tree_search.hpp"

namespace stage {

// ----------------------------------------------------------------------------------------
// whole-table scan (stage_table_scan / stage_table_scan_window): every record of the leaves
// [leaf0, leaf0 + nl) in leaf and slot order -- TableScanExecutor with scan_sz == -1
// (executor.h:581-619, ScanLeafNode), or, with a read id, IndexScanExecutor's per-record rule
// (executor.h:465-534) over the slots the range iterator considers.  No tree descent, no key
// planes, no fingerprints: leaf heads, slot words and heap rows only, so the geometry (cap, key
// words) stays a run-time value and nothing here is instantiated per table shape.
//
// Output positions are the leaf and slot order, found by three stream-ordered steps in which no
// workgroup waits for another: records per leaf and their sums over tiles of 64 leaves
// (table_scan_count_kernel), an exclusive scan of the tile sums by one block
// (table_scan_offsets_kernel), and the emit pass, where a leaf's wave adds the counts of its
// tile's earlier leaves (one 256-B load) to the tile's offset.  The filtered forms (further down)
// replace the first step by a match pass and run the other two as they are.
constexpr uint32_t kTableScanMaxCap = 1024;  // slots per leaf the emit pass's LDS list holds

// what an emit launch carries (wave-uniform); the type also selects the emitting lanes at compile
// time: every slot of the scan here, the match pass's bits with TableScanMatchArgs
struct TableScanArgs {
    static constexpr bool matched = false;
    uint32_t leaf0, nl;      // the range: leaves leaf0 .. leaf0 + nl - 1
    const uint32_t *cnt;     // [nl] records per leaf
    const uint64_t *toff;    // [(nl + 63) / 64] position of each tile's first record
    uint64_t max_records;    // positions >= max_records are not written
    uint64_t *leaf_offsets;  // optional [nl]: position of each leaf's first record
    uint64_t *row_meta;      // optional: the slot's RecordMetadata word per record
    uint8_t *row_status;     // optional: ST_LATEST / ST_OLD / ST_NOT_FOUND per record
    uint8_t *recs;           // row form: rows of t.stride bytes
    ScanWindowArgs a;        // window form
    uint32_t rid;            // snapshot mode: the read id
};
struct TableScanMatchArgs : TableScanArgs {
    static constexpr bool matched = true;
    const uint64_t *mask;  // [nl * cap / 64] the match pass's bits
    uint64_t *row_slot;    // optional: (leaf << 16) | slot per record
};

// records per leaf of the range and their sums over tiles of 64 leaves, a wave per tile and a
// lane per leaf.  Snapshot mode (VIS): the popcount of the head's visible masks -- heads only.
// Raw mode counts the slots below the record count whose meta word is non-zero: a visible slot
// lies below the record count and its meta word is non-zero, so a leaf whose visible slots are
// as many as its records has exactly that many; only the other leaves (deleted or invisible
// slots) have their meta words read, by the whole wave, one such leaf after the other.
template <bool VIS>
__global__ __launch_bounds__(256) void table_scan_count_kernel(DevTable t, uint32_t leaf0, uint32_t nl,
                                                               uint32_t *__restrict__ cnt,
                                                               uint64_t *__restrict__ tsum) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t ntiles = ((uint64_t)nl + 63) >> 6;
    const uint32_t spl = t.cap >> 6;
    for (uint64_t k = wave; k < ntiles; k += nwaves) {
        const uint64_t i = k * 64 + lane;
        const uint32_t leaf = leaf0 + (uint32_t)i;
        uint32_t c = 0, rc = 0;
        if (i < nl) {
            for (uint32_t s = 0; s < spl; ++s) c += (uint32_t)__builtin_popcountll(head_vis(t, leaf, (int)s));
            if (!VIS) {
                rc = *reinterpret_cast<const uint32_t *>(t.head + (uint64_t)leaf * t.head_bytes +
                                                         head_info_offset(t.cap, t.key_words)) & 0xFFFFu;
                if (rc > t.cap) rc = t.cap;
            }
        }
        if (!VIS) {
            uint64_t todo = ballot(c != rc);
            while (todo) {
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1;
                const uint64_t base = (uint64_t)rl32(leaf, l) * t.cap;
                const uint32_t n = rl32(rc, l);
                uint32_t m = 0;
                for (uint32_t s0 = 0; s0 < n; s0 += 64u) {
                    const uint32_t sl = s0 + lane;
                    m += (uint32_t)__builtin_popcountll(ballot(sl < n && t.slot[base + sl].meta != 0));
                }
                if (lane == (uint32_t)l) c = m;
            }
        }
        if (i < nl) cnt[i] = c;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
        if (lane == 0) tsum[k] = c;
    }
}

// one block of 1024 threads: the tile sums become their exclusive prefix sums in place, the
// total goes to total[0] and, when given, to last[0] (the closing entry of the leaf offsets)
__global__ __launch_bounds__(1024) void table_scan_offsets_kernel(uint64_t *__restrict__ tsum, uint64_t ntiles,
                                                                  uint64_t *__restrict__ total,
                                                                  uint64_t *__restrict__ last) {
    __shared__ uint64_t s_wave[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint64_t carry = 0;
    for (uint64_t b = 0; b < ntiles; b += 1024) {
        const uint64_t i = b + tid;
        const uint64_t v = i < ntiles ? tsum[i] : 0ull;
        uint64_t y = v;  // inclusive prefix inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t z = (uint64_t)__shfl_up((unsigned long long)y, (unsigned)o, 64);
            if (lane >= (uint32_t)o) y += z;
        }
        if (lane == 63) s_wave[wv] = y;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint64_t w = s_wave[k];
            if (k < wv) before += w;
            all += w;
        }
        if (i < ntiles) tsum[i] = carry + before + y - v;
        carry += all;
        __syncthreads();  // s_wave is rewritten by the next round
    }
    if (tid == 0) {
        total[0] = carry;
        if (last) last[0] = carry;
    }
}

// The e rows at output positions pos0 .. pos0 + e - 1, their heap rows in rank order in the
// wave's LDS list rk (0xFFFFFFFF: the record yields no tuple, its row is zero).  The rows are
// consecutive in memory, e * (stride / 16) pieces: chunks of 64 ranks are stored wave-wide with
// coalesced 16-B nontemporal stores, piece q of a chunk belonging to rank q / chunks (its heap row
// comes from that lane, ds_bpermute) -- store_windows' shape with heap_chunk as the piece, the
// bytes copy_rows writes.  Called by every lane of the wave, after the list's writes are fenced.
template <int U = 4>
__device__ __forceinline__ void store_scan_rows(const DevTable &t, uint32_t lane, uint64_t pos0, uint32_t e,
                                                const uint32_t *rk, uint8_t *recs) {
    const uint32_t chunks = t.stride >> 4;
    for (uint32_t r0 = 0; r0 < e; r0 += 64u) {
        const uint32_t cnt = e - r0 < 64u ? e - r0 : 64u;
        const uint32_t image = lane < cnt ? rk[r0 + lane] : 0xFFFFFFFFu;
        const uint32_t total = cnt * chunks;
        u32x4 *out = reinterpret_cast<u32x4 *>(recs + (pos0 + r0) * (uint64_t)t.stride);
        for (uint32_t q0 = 0; q0 < total; q0 += 64u * U) {
            u32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t q = q0 + 64u * u + lane;
                const uint32_t p = q / chunks, c = q - p * chunks;
                const uint32_t img = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((p & 63u) << 2), (int)image);
                v[u] = u32x4{0, 0, 0, 0};
                if (q < total && img != 0xFFFFFFFFu) v[u] = heap_chunk(t, img, c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t q = q0 + 64u * u + lane;
                if (q < total) __builtin_nontemporal_store(v[u], out + q);
            }
        }
    }
}

// the emit pass of both families, a wave per leaf.
// Shared: the counts of the leaf's tile, the tile's offset and the first head or mask word are
// loaded together before any of them is used, then the slot words of the lanes they name (two
// round trips to the heap-row loads instead of four dependent ones); the leaf's first position;
// each 64-slot group's emitting lanes rank themselves, put their heap rows into the wave's LDS
// list by rank and write meta / status at their positions; the leaf's records then leave as
// consecutive rows (store_scan_rows) or windows (store_scan_windows), cut at max_records.
// Different, chosen at compile time by Args::matched (SEL below) -- where the emitting lanes come
// from:
//   every slot (TableScanArgs): the lanes the head names (snapshot) or the lanes below the record
//     count whose meta word is non-zero (raw); the emitting lanes are a ballot over them.
//   the match pass's bits (TableScanMatchArgs): the stored word is the ballot; a leaf without a
//     match is skipped after its offset is written, a group without one costs its mask word; the
//     matched lanes resolve image and status again (the same image: the passes are stream-ordered
//     on one published image); row_slot is written.
template <bool VIS, bool WIN, class Args>
__global__ __launch_bounds__(256) void table_scan_emit_kernel(DevTable t, Args g) {
    constexpr bool SEL = Args::matched;
    __shared__ uint32_t s_img[4][kTableScanMaxCap];
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    uint32_t *rk = s_img[wv];
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t spl = t.cap >> 6;
    for (uint64_t i = wave; i < g.nl; i += nwaves) {
        const uint32_t leaf = g.leaf0 + (uint32_t)i;
        const uint64_t base = (uint64_t)leaf * t.cap;
        const uint64_t tile = i >> 6;
        const uint32_t self = (uint32_t)(i & 63u);
        // the counts of the tile's earlier leaves; SEL: one lane more, the leaf's own count
        uint32_t v = lane < (SEL ? self + 1u : self) ? g.cnt[tile * 64 + lane] : 0u;
        const uint64_t tile0 = g.toff[tile];
        uint32_t rc = t.cap;  // raw unfiltered scan: the head's record count; otherwise every group is visited
        uint32_t own = 1;     // SEL: the leaf's matches, 0 skips the leaf; the unfiltered scan never skips one here
        uint64_t vm = 0;      // the group's head word (VIS) or mask word (SEL); unused in the raw unfiltered scan
        if constexpr (SEL) {
            vm = uni64(g.mask[i * spl]);
            own = rl32(v, (int)self);
            v = lane < self ? v : 0u;
        } else {
            if (!VIS)
                rc = *reinterpret_cast<const uint32_t *>(t.head + (uint64_t)leaf * t.head_bytes +
                                                         head_info_offset(t.cap, t.key_words)) & 0xFFFFu;
            if (VIS) vm = head_vis(t, leaf, 0);
        }
        // the leaf's first position: its tile's offset and the tile's earlier leaves
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
        const uint64_t pos0 = tile0 + uni32(v);
        if (g.leaf_offsets && lane == 0) g.leaf_offsets[i] = pos0;
        if (own == 0 || pos0 >= g.max_records) continue;
        if constexpr (!SEL) {
            rc = uni32(rc);
            if (rc > t.cap) rc = t.cap;
        }
        uint32_t produced = 0;
        for (uint32_t s = 0; s < spl && (SEL || s * 64u < rc); ++s) {
            if constexpr (SEL) {
                if (s) vm = uni64(g.mask[i * spl + s]);
                if (vm == 0) continue;
            } else if (VIS && s) {
                vm = head_vis(t, leaf, (int)s);
            }
            bool on = VIS || SEL ? ((vm >> lane) & 1) != 0 : s * 64u + lane < rc;
            uint64_t meta = 0;
            uint32_t img = 0xFFFFFFFFu;
            uint8_t st = ST_LATEST;
            if (on) {
                const SlotInfo si = t.slot[base + s * 64u + lane];
                meta = si.meta;
                if (VIS) {
                    img = scan_visible(t, si, g.rid, st);
                } else {
                    img = si.image;
                    if (!SEL) on = meta != 0;  // 0: a deleted slot
                }
            }
            const uint64_t em = SEL ? vm : ballot(on);
            if (on) {
                const uint32_t r = produced + count_below(em);  // < cap
                rk[r] = img;
                const uint64_t k = pos0 + r;
                if (k < g.max_records) {
                    if (g.row_meta) g.row_meta[k] = meta;
                    if (g.row_status) g.row_status[k] = st;
                    if constexpr (SEL)
                        if (g.row_slot) g.row_slot[k] = ((uint64_t)leaf << 16) | (s * 64u + lane);
                }
            }
            produced += (uint32_t)__builtin_popcountll(em);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint64_t room = g.max_records - pos0;
        const uint32_t e = produced < room ? produced : (uint32_t)room;
        if (WIN) store_scan_windows(t, lane, pos0, e, rk, g.a);
        else store_scan_rows(t, lane, pos0, e, rk, g.recs);
        __builtin_amdgcn_wave_barrier();  // the list is rewritten on the next leaf
    }
}

// ----------------------------------------------------------------------------------------
// filtered whole-table scans (stage_table_scan_where / _where_window / _aggregate): the records
// of the unfiltered scan that yield a tuple and on whose row bytes every predicate holds --
// the per-tuple predicate of TableScanExecutor / IndexScanExecutor (executor.h:346-361, 465-534,
// 573-642) evaluated on the device.  A match pass stores one bit per slot and the matches per
// leaf; the offsets and the emit pass above do the rest (TableScanMatchArgs).  The aggregate runs
// the match pass's loop alone and keeps count / sum / min / max in registers.  Integer arithmetic
// only, no atomics, no workgroup waits for another.

// column `width` bytes at row byte src of heap row img, little-endian at any alignment, zero-
// extended: out of the one or two aligned 8-B words that hold it.  The second word is read only
// when the column's last byte lies in it, and that byte is below src + width <= key pad +
// payload <= hstride (a multiple of 16), so no load leaves the row's own hstride bytes.
__device__ __forceinline__ uint64_t column_bits(const DevTable &t, uint32_t img, uint32_t src, uint32_t width) {
    const uint64_t *row = reinterpret_cast<const uint64_t *>(t.heap + (uint64_t)img * t.hstride);
    const uint32_t w = src >> 3, sh = uni32(src & 7u);
    uint64_t x = row[w] >> (8u * sh);
    if (sh + width > 8u) x |= row[w + 1u] << (8u * (8u - sh));  // sh >= 1 here
    return width >= 8u ? x : x & ((1ull << (8u * width)) - 1ull);
}

// the column's value in a domain where unsigned order is the column's order: the sign-extended
// value with its top bit flipped (signed), the zero-extended value (unsigned)
__device__ __forceinline__ uint64_t column_key(uint64_t bits, uint32_t width, bool is_signed) {
    if (!is_signed) return bits;
    const uint32_t up = 64u - 8u * width;
    return (uint64_t)((int64_t)(bits << up) >> up) ^ (1ull << 63);
}

// every predicate on heap row img (wave-uniform predicates, kernel arguments)
__device__ __forceinline__ bool preds_hold(const DevTable &t, uint32_t img, const ScanPreds &p) {
    bool ok = true;
#pragma unroll
    for (uint32_t k = 0; k < kScanPredMax; ++k)
        if (k < p.n) {
            const ScanPred &q = p.p[k];
            const uint64_t x = column_key(column_bits(t, img, q.src, q.width), q.width, q.is_signed != 0);
            // lo / hi arrive in the same order domain (order_domain flips a signed column's)
            const bool in = x >= (uint64_t)q.lo && x <= (uint64_t)q.hi;
            ok &= in != (q.negate != 0);
        }
    return ok;
}

// one 64-slot group of a leaf: the lanes the head names (snapshot) or the lanes below the record
// count (raw) read their slot word and resolve the image; -> the lane's heap row, 0xFFFFFFFF
// when the lane's slot is not part of the scan or yields no tuple
template <bool VIS>
__device__ __forceinline__ uint32_t scan_group_image(const DevTable &t, uint32_t leaf, uint32_t s, uint32_t lane,
                                                     uint32_t rc, uint32_t rid) {
    const bool on = VIS ? ((head_vis(t, leaf, (int)s) >> lane) & 1) != 0 : s * 64u + lane < rc;
    uint32_t img = 0xFFFFFFFFu;
    if (on) {
        const SlotInfo si = t.slot[(uint64_t)leaf * t.cap + s * 64u + lane];
        uint8_t st;
        if (VIS) img = scan_visible(t, si, rid, st);
        else if (si.meta != 0) img = si.image;
    }
    return img;
}

template <bool VIS>
__device__ __forceinline__ uint32_t scan_record_count(const DevTable &t, uint32_t leaf) {
    if (VIS) return t.cap;
    const uint32_t rc = uni32(*reinterpret_cast<const uint32_t *>(t.head + (uint64_t)leaf * t.head_bytes +
                                                                  head_info_offset(t.cap, t.key_words)) & 0xFFFFu);
    return rc > t.cap ? t.cap : rc;
}

// the match pass, a wave per leaf: mask[i * (cap / 64) + s] = the matching lanes of leaf i's
// slot group s, cnt[i] = their number
template <bool VIS>
__global__ __launch_bounds__(256) void table_scan_match_kernel(DevTable t, uint32_t leaf0, uint32_t nl, uint32_t rid,
                                                               ScanPreds p, uint64_t *__restrict__ mask,
                                                               uint32_t *__restrict__ cnt) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t spl = t.cap >> 6;
    for (uint64_t i = wave; i < nl; i += nwaves) {
        const uint32_t leaf = leaf0 + (uint32_t)i;
        const uint32_t rc = scan_record_count<VIS>(t, leaf);
        uint32_t total = 0;
        for (uint32_t s = 0; s < spl; ++s) {
            uint64_t m = 0;
            if (s * 64u < rc) {
                const uint32_t img = scan_group_image<VIS>(t, leaf, s, lane, rc, rid);
                m = ballot(img != 0xFFFFFFFFu && preds_hold(t, img, p));
            }
            if (lane == 0) mask[i * spl + s] = m;
            total += (uint32_t)__builtin_popcountll(m);
        }
        if (lane == 0) cnt[i] = total;
    }
}

// the sums of cnt over tiles of 64 leaves, a wave per tile and a lane per leaf
__global__ __launch_bounds__(256) void table_scan_tile_sums_kernel(const uint32_t *__restrict__ cnt, uint32_t nl,
                                                                   uint64_t *__restrict__ tsum) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t ntiles = ((uint64_t)nl + 63) >> 6;
    for (uint64_t k = wave; k < ntiles; k += nwaves) {
        const uint64_t i = k * 64 + lane;
        uint32_t c = i < nl ? cnt[i] : 0u;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
        if (lane == 0) tsum[k] = c;
    }
}

// count / sum / min / max of one block's (or the fold's) lanes: over the wave by shuffles, over
// the block's waves through LDS; thread 0 holds the result.  min / max travel in the unsigned
// order domain of column_key.
struct AggAcc {
    uint64_t count, sum, min, max;
};
__device__ __forceinline__ void agg_add(AggAcc &a, const AggAcc &b) {
    a.count += b.count;
    a.sum += b.sum;
    a.min = b.min < a.min ? b.min : a.min;
    a.max = b.max > a.max ? b.max : a.max;
}
__device__ __forceinline__ void agg_block_reduce(AggAcc &a, AggAcc *s_part) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        AggAcc b;
        b.count = (uint64_t)__shfl_xor((unsigned long long)a.count, o, 64);
        b.sum = (uint64_t)__shfl_xor((unsigned long long)a.sum, o, 64);
        b.min = (uint64_t)__shfl_xor((unsigned long long)a.min, o, 64);
        b.max = (uint64_t)__shfl_xor((unsigned long long)a.max, o, 64);
        agg_add(a, b);
    }
    const uint32_t wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63u) == 0) s_part[wv] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t k = 1; k < nw; ++k) agg_add(a, s_part[k]);
}

// the aggregate column of a launch (wave-uniform); width 0: count only
struct ScanAggCol {
    uint32_t src, width, is_signed;
};

// the match pass's loop with the aggregate column read beside the predicate columns; each block
// leaves one partial (order-domain min / max) in part[blockIdx.x]
template <bool VIS>
__global__ __launch_bounds__(256) void table_scan_aggregate_kernel(DevTable t, uint32_t leaf0, uint32_t nl,
                                                                   uint32_t rid, ScanPreds p, ScanAggCol col,
                                                                   AggAcc *__restrict__ part) {
    __shared__ AggAcc s_part[4];
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t spl = t.cap >> 6;
    AggAcc acc{0, 0, ~0ull, 0};
    for (uint64_t i = wave; i < nl; i += nwaves) {
        const uint32_t leaf = leaf0 + (uint32_t)i;
        const uint32_t rc = scan_record_count<VIS>(t, leaf);
        for (uint32_t s = 0; s < spl && s * 64u < rc; ++s) {
            const uint32_t img = scan_group_image<VIS>(t, leaf, s, lane, rc, rid);
            if (img != 0xFFFFFFFFu && preds_hold(t, img, p)) {
                acc.count += 1;
                if (col.width) {
                    const uint64_t x = column_key(column_bits(t, img, col.src, col.width), col.width, col.is_signed != 0);
                    acc.sum += col.is_signed ? x ^ (1ull << 63) : x;  // the extended value, modulo 2^64
                    acc.min = x < acc.min ? x : acc.min;
                    acc.max = x > acc.max ? x : acc.max;
                }
            }
        }
    }
    agg_block_reduce(acc, s_part);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// one block folds the partials into agg[0] = {count, sum, min, max} in the column's domain;
// no match (or no partial at all): min = the domain's largest value, max = its smallest
__global__ __launch_bounds__(256) void table_scan_aggregate_fold_kernel(const AggAcc *__restrict__ part, uint32_t nparts,
                                                                        ScanAggCol col, uint64_t *__restrict__ agg) {
    __shared__ AggAcc s_part[4];
    AggAcc acc{0, 0, ~0ull, 0};
    for (uint32_t k = threadIdx.x; k < nparts; k += blockDim.x) agg_add(acc, part[k]);
    agg_block_reduce(acc, s_part);
    if (threadIdx.x != 0) return;
    uint64_t mn = 0, mx = 0;
    if (col.width) {
        const uint64_t flip = col.is_signed ? 1ull << 63 : 0ull;
        if (acc.count) {
            mn = acc.min ^ flip;
            mx = acc.max ^ flip;
        } else {
            const uint64_t ones = col.width >= 8u ? ~0ull : (1ull << (8u * col.width)) - 1ull;
            mn = col.is_signed ? ones >> 1 : ones;   // 2^(8w-1) - 1, or 2^(8w) - 1
            mx = col.is_signed ? ~(ones >> 1) : 0ull;  // -2^(8w-1), or 0
        }
    }
    agg[0] = acc.count;
    agg[1] = acc.sum;
    agg[2] = mn;
    agg[3] = mx;
}

// a signed column's bounds enter the order domain of column_key once, on the host
static ScanPreds order_domain(ScanPreds p) {
    for (uint32_t k = 0; k < p.n; ++k)
        if (p.p[k].is_signed) {
            p.p[k].lo = (int64_t)((uint64_t)p.p[k].lo ^ (1ull << 63));
            p.p[k].hi = (int64_t)((uint64_t)p.p[k].hi ^ (1ull << 63));
        }
    return p;
}

// an integer column of a heap row: column_bits' loads rest on it
static bool column_fits(uint32_t width, uint32_t src, uint32_t hstride) {
    return scan_column_width(width) && (uint64_t)src + width <= hstride;
}

static bool preds_fit(const DevTable &t, const ScanPreds &p) {
    if (p.n > kScanPredMax) return false;
    for (uint32_t k = 0; k < p.n; ++k)
        if (!column_fits(p.p[k].width, p.p[k].src, t.hstride)) return false;
    return true;
}

template <class Args>
static void launch_table_scan_emit(const DevTable &t, const Args &g, bool snapshot, bool win, int blocks, hipStream_t s) {
    if (snapshot) {
        if (win) table_scan_emit_kernel<true, true><<<blocks, 256, 0, s>>>(t, g);
        else table_scan_emit_kernel<true, false><<<blocks, 256, 0, s>>>(t, g);
    } else {
        if (win) table_scan_emit_kernel<false, true><<<blocks, 256, 0, s>>>(t, g);
        else table_scan_emit_kernel<false, false><<<blocks, 256, 0, s>>>(t, g);
    }
}

// both scan launchers; preds null: the unfiltered scan.  scratch: the tile offsets, with preds one
// mask word per 64 slots, the records per leaf.
static hipError_t table_scan_launches(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                                      const ScanPreds *preds, uint32_t row_off, uint32_t len, uint32_t key_pad,
                                      const TableScanOut &o, uint64_t *row_slot, uint8_t *scratch, hipStream_t s,
                                      const ScanTuning &tune) {
    const bool win = len != 0;
    // the leaves exist, a leaf's records fit the emit pass's list, and the window, the key and
    // every predicate column lie inside a heap row (window_piece's, the key writer's and
    // column_bits' loads rest on it)
    if ((uint64_t)leaf0 + nl > t.nleaves || t.cap > kTableScanMaxCap || !o.count || (preds && !preds_fit(t, *preds)))
        return hipErrorInvalidValue;
    if (win && ((uint64_t)row_off + len > t.hstride || key_pad > t.hstride || (key_pad & 7u))) return hipErrorInvalidValue;
    if (o.max_records && !(win ? o.win : o.recs)) return hipErrorInvalidValue;
    if (nl == 0) {
        hipError_t e = hipMemsetAsync(o.count, 0, sizeof(uint64_t), s);
        if (e == hipSuccess && o.leaf_offsets) e = hipMemsetAsync(o.leaf_offsets, 0, sizeof(uint64_t), s);
        return e;
    }
    if (!scratch) return hipErrorInvalidValue;
    const uint64_t ntiles = ((uint64_t)nl + 63) / 64;
    uint64_t *toff = reinterpret_cast<uint64_t *>(scratch);
    uint64_t *mask = toff + ntiles;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(preds ? mask + (uint64_t)nl * (t.cap / 64) : mask);
    const int mb = max_blocks(tune);
    const int blocks = grid_for(nl, 4, mb), tile_blocks = grid_for(ntiles, 4, mb);
    // records per leaf and per tile: from the heads alone, or the match pass and its tile sums
    if (preds) {
        const ScanPreds p = order_domain(*preds);
        if (snapshot) table_scan_match_kernel<true><<<blocks, 256, 0, s>>>(t, leaf0, nl, rid, p, mask, cnt);
        else table_scan_match_kernel<false><<<blocks, 256, 0, s>>>(t, leaf0, nl, rid, p, mask, cnt);
        table_scan_tile_sums_kernel<<<tile_blocks, 256, 0, s>>>(cnt, nl, toff);
    } else if (snapshot) {
        table_scan_count_kernel<true><<<tile_blocks, 256, 0, s>>>(t, leaf0, nl, cnt, toff);
    } else {
        table_scan_count_kernel<false><<<tile_blocks, 256, 0, s>>>(t, leaf0, nl, cnt, toff);
    }
    table_scan_offsets_kernel<<<1, 1024, 0, s>>>(toff, ntiles, o.count, o.leaf_offsets ? o.leaf_offsets + nl : nullptr);
    if (o.max_records || o.leaf_offsets) {
        const TableScanArgs g{leaf0, nl, cnt, toff, o.max_records, o.leaf_offsets, o.row_meta, o.row_status, o.recs,
                              ScanWindowArgs{WindowArgs{row_off, len, (len + 15u) >> 4, o.win}, o.row_keys, key_pad}, rid};
        if (preds) launch_table_scan_emit(t, TableScanMatchArgs{g, mask, row_slot}, snapshot, win, blocks, s);
        else launch_table_scan_emit(t, g, snapshot, win, blocks, s);
    }
    return hipGetLastError();
}

uint64_t table_scan_scratch_bytes(uint64_t nl) { return ((nl + 63) / 64) * 8 + nl * 4; }

uint64_t table_scan_where_scratch_bytes(uint64_t nl, uint32_t cap) {
    return table_scan_scratch_bytes(nl) + nl * (cap / 64) * 8;
}

hipError_t launch_table_scan(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                             uint32_t row_off, uint32_t len, uint32_t key_pad, const TableScanOut &o, uint8_t *scratch,
                             hipStream_t s, const ScanTuning &tune) {
    return table_scan_launches(t, leaf0, nl, snapshot, rid, nullptr, row_off, len, key_pad, o, nullptr, scratch, s, tune);
}

hipError_t launch_table_scan_where(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                                   const ScanPreds &preds, uint32_t row_off, uint32_t len, uint32_t key_pad,
                                   const TableScanOut &o, uint64_t *row_slot, uint8_t *scratch, hipStream_t s,
                                   const ScanTuning &tune) {
    return table_scan_launches(t, leaf0, nl, snapshot, rid, &preds, row_off, len, key_pad, o, row_slot, scratch, s, tune);
}

// the match pass's grid: a partial per block is 32 B of scratch, and a grid of a few blocks per
// CU (2048, measured at 100M rows) left a tail of blocks that no longer fit beside the first wave
static int aggregate_blocks(uint32_t nl, const ScanTuning &tune) { return grid_for(nl, 4, max_blocks(tune)); }

uint64_t table_scan_aggregate_scratch_bytes(uint64_t nl, const ScanTuning &tune) {
    return nl ? (uint64_t)aggregate_blocks((uint32_t)nl, tune) * sizeof(AggAcc) : 0;
}

hipError_t launch_table_scan_aggregate(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                                       const ScanPreds &preds, uint32_t agg_src, uint32_t agg_width, bool agg_signed,
                                       uint64_t *agg, uint8_t *scratch, hipStream_t s, const ScanTuning &tune) {
    if ((uint64_t)leaf0 + nl > t.nleaves || !agg || !preds_fit(t, preds)) return hipErrorInvalidValue;
    if (agg_width && !column_fits(agg_width, agg_src, t.hstride)) return hipErrorInvalidValue;
    if (nl && !scratch) return hipErrorInvalidValue;
    const ScanAggCol col{agg_src, agg_width, agg_signed ? 1u : 0u};
    AggAcc *part = reinterpret_cast<AggAcc *>(scratch);
    const int blocks = nl ? aggregate_blocks(nl, tune) : 0;
    if (nl) {
        const ScanPreds p = order_domain(preds);
        if (snapshot) table_scan_aggregate_kernel<true><<<blocks, 256, 0, s>>>(t, leaf0, nl, rid, p, col, part);
        else table_scan_aggregate_kernel<false><<<blocks, 256, 0, s>>>(t, leaf0, nl, rid, p, col, part);
    }
    table_scan_aggregate_fold_kernel<<<1, 256, 0, s>>>(part, (uint32_t)blocks, col, agg);
    return hipGetLastError();
}


// ----------------------------------------------------------------------------------------
// grouped aggregate (stage_table_scan_group_aggregate): the aggregate's record set and loop, each
// matching record added to the entry of its group -- count / sum / min / max per value of one
// integer column, GROUP BY on the device (the per-group MIN of RunQuery2's SQL,
// tpcc_new_order.cpp:621-630; executor.h:346-361, 465-534, 573-642 for the record set).  The
// entries are AggAcc records (order-domain min / max) updated with 64-bit integer atomics.
//   LDS tier (at most kGroupLdsMax groups): a table per workgroup in LDS, every lane updates its
//     entry; the workgroup leaves its table in scratch and a fold launch, a workgroup per entry,
//     reduces the tables and writes the records in the column's domain -- the aggregate's two
//     steps with a table in place of one partial.
//   global tier: a fill launch writes the order-domain identities into groups[], the scan launch
//     updates groups[] itself, a finish launch turns min / max into the column's domain.  Updates
//     of one entry serialise in the L2 (about 11 ns each, measured), so the lanes of a wave that
//     share the first lane's group are reduced by shuffles, a wave keeps that result in registers
//     while the next 64 records give the same group, and a workgroup's waves merge what they
//     still hold at the end: a group that takes most records (the rest group, typically) costs
//     one update per workgroup, not one per record.
// Integer atomics are order-free, so both tiers and every grid give the same bytes; no workgroup
// waits for another.

// the group column of a launch (wave-uniform)
struct ScanGroupCol {
    uint32_t src, width, is_signed;
    uint32_t n;     // groups; entry n is the rest group
    uint64_t base;  // group 0's value in the order domain of column_key
    uint32_t kmax;  // distinct groups of a wave's 64 records that are combined before the update
};

// one entry takes cnt records with sum, min and max (col false: the count alone).  No value
// returns, so these are ds_add / ds_min / ds_max _u64 and global_atomic_ add / umin / umax _x2.
template <bool LDS>
__device__ __forceinline__ void group_entry_add(AggAcc *e, const AggAcc &v, bool col) {
    constexpr int scope = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    __hip_atomic_fetch_add(&e->count, v.count, __ATOMIC_RELAXED, scope);
    if (col) {
        __hip_atomic_fetch_add(&e->sum, v.sum, __ATOMIC_RELAXED, scope);
        __hip_atomic_fetch_min(&e->min, v.min, __ATOMIC_RELAXED, scope);
        __hip_atomic_fetch_max(&e->max, v.max, __ATOMIC_RELAXED, scope);
    }
}

// what a wave of the global tier still holds for one group (wave-uniform); g == kNoGroup: nothing
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;
struct GroupPending {
    uint32_t g;
    AggAcc a;
};

// the wave's 64 records (on: the lane has one, of group g with order-domain value x and summand
// sv) enter the table.  Up to kmax times the first remaining lane's group is taken out when two
// or more lanes hold it: they are reduced by shuffles into one update -- of the entry (LDS), or
// of what the wave holds (global tier: merged when it is the same group, else what was held goes
// to its entry first).  The lanes that remain update their entries themselves.  Called by every
// lane of the wave.
template <bool LDS>
__device__ __forceinline__ void group_wave_add(AggAcc *tab, GroupPending &pend, bool on, uint32_t g, uint64_t x,
                                               uint64_t sv, bool col, uint32_t kmax, uint32_t lane) {
    uint64_t todo = ballot(on);
    for (uint32_t it = 0; todo != 0 && it < kmax; ++it) {
        const int l = __builtin_ctzll(todo);
        const uint32_t g0 = rl32(g, l);
        const bool peer = on && g == g0;
        const uint64_t peers = ballot(peer);
        todo &= ~peers;
        const uint32_t np = (uint32_t)__builtin_popcountll(peers);
        if (np < 2) continue;
        AggAcc v{np, peer ? sv : 0ull, peer ? x : ~0ull, peer ? x : 0ull};
        if (col) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                v.sum += (uint64_t)__shfl_xor((unsigned long long)v.sum, o, 64);
                const uint64_t a = (uint64_t)__shfl_xor((unsigned long long)v.min, o, 64);
                const uint64_t b = (uint64_t)__shfl_xor((unsigned long long)v.max, o, 64);
                v.min = a < v.min ? a : v.min;
                v.max = b > v.max ? b : v.max;
            }
        }
        if (LDS) {
            if (lane == (uint32_t)l) group_entry_add<true>(tab + g0, v, col);
        } else if (pend.g == g0) {
            agg_add(pend.a, v);
        } else {
            if (pend.g != kNoGroup && lane == 0) group_entry_add<false>(tab + pend.g, pend.a, col);
            pend.g = g0;
            pend.a = v;
        }
        on = on && !peer;
    }
    if (on) group_entry_add<LDS>(tab + g, AggAcc{1, sv, x, x}, col);
}

// the aggregate's loop.  LDS: out = the scratch tables, gc.n + 1 entries per workgroup; the
// workgroup's table is dynamic shared memory, initialised to the identities and copied out at
// the end.  Global tier: out = groups[].
template <bool VIS, bool LDS>
__global__ __launch_bounds__(256) void table_scan_group_kernel(DevTable t, uint32_t leaf0, uint32_t nl, uint32_t rid,
                                                               ScanPreds p, ScanGroupCol gc, ScanAggCol col,
                                                               AggAcc *__restrict__ out) {
    extern __shared__ AggAcc s_groups[];
    AggAcc *tab = LDS ? s_groups : out;
    if (LDS) {
        for (uint32_t k = threadIdx.x; k <= gc.n; k += blockDim.x) s_groups[k] = AggAcc{0, 0, ~0ull, 0};
        __syncthreads();
    }
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t spl = t.cap >> 6;
    const bool agg = col.width != 0;
    GroupPending pend{kNoGroup, AggAcc{0, 0, ~0ull, 0}};
    for (uint64_t i = wave; i < nl; i += nwaves) {
        const uint32_t leaf = leaf0 + (uint32_t)i;
        const uint32_t rc = scan_record_count<VIS>(t, leaf);
        for (uint32_t s = 0; s < spl && s * 64u < rc; ++s) {
            const uint32_t img = scan_group_image<VIS>(t, leaf, s, lane, rc, rid);
            const bool on = img != 0xFFFFFFFFu && preds_hold(t, img, p);
            uint32_t g = gc.n;
            uint64_t x = 0;
            if (on) {
                // x - base in the integers: both are in the order domain, where nothing wraps
                const uint64_t k = column_key(column_bits(t, img, gc.src, gc.width), gc.width, gc.is_signed != 0);
                if (k >= gc.base && k - gc.base < gc.n) g = (uint32_t)(k - gc.base);
                if (agg) x = column_key(column_bits(t, img, col.src, col.width), col.width, col.is_signed != 0);
            }
            if (ballot(on) == 0) continue;
            group_wave_add<LDS>(tab, pend, on, g, x, col.is_signed ? x ^ (1ull << 63) : x, agg, gc.kmax, lane);
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        AggAcc *mine = out + (uint64_t)blockIdx.x * ((uint64_t)gc.n + 1);
        for (uint32_t k = threadIdx.x; k <= gc.n; k += blockDim.x) mine[k] = s_groups[k];
    } else {
        // what the waves still hold: equal groups merged, one update each
        __shared__ GroupPending s_pend[4];
        if (lane == 0) s_pend[wv] = pend;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t nw = blockDim.x >> 6;
            for (uint32_t k = 0; k < nw; ++k) {
                GroupPending a = s_pend[k];
                if (a.g == kNoGroup) continue;
                for (uint32_t j = k + 1; j < nw; ++j)
                    if (s_pend[j].g == a.g) {
                        agg_add(a.a, s_pend[j].a);
                        s_pend[j].g = kNoGroup;
                    }
                group_entry_add<false>(out + a.g, a.a, agg);
            }
        }
    }
}

// an entry's record in the column's domain; no record: the identities of
// table_scan_aggregate_fold_kernel (min = the domain's largest value, max = its smallest)
__device__ __forceinline__ AggAcc group_record(AggAcc a, const ScanAggCol &col) {
    if (!col.width) {
        a.sum = a.min = a.max = 0;
    } else if (a.count) {
        const uint64_t flip = col.is_signed ? 1ull << 63 : 0ull;
        a.min ^= flip;
        a.max ^= flip;
    } else {
        const uint64_t ones = col.width >= 8u ? ~0ull : (1ull << (8u * col.width)) - 1ull;
        a.sum = 0;
        a.min = col.is_signed ? ones >> 1 : ones;
        a.max = col.is_signed ? ~(ones >> 1) : 0ull;
    }
    return a;
}

// LDS tier: workgroup e folds entry e of the nparts scratch tables (n entries each) into groups[e]
__global__ __launch_bounds__(256) void table_scan_group_fold_kernel(const AggAcc *__restrict__ part, uint32_t nparts,
                                                                    uint32_t n, ScanAggCol col,
                                                                    AggAcc *__restrict__ groups) {
    __shared__ AggAcc s_part[4];
    const uint32_t e = blockIdx.x;
    AggAcc acc{0, 0, ~0ull, 0};
    for (uint32_t b = threadIdx.x; b < nparts; b += blockDim.x) agg_add(acc, part[(uint64_t)b * n + e]);
    agg_block_reduce(acc, s_part);
    if (threadIdx.x == 0) groups[e] = group_record(acc, col);
}

// global tier, n entries of groups[]: fill -- the order-domain identities the scan launch starts
// from; finish -- its entries in the column's domain (fresh: the record of an entry without a
// record for every entry, nothing is read -- the empty leaf range of either tier)
__global__ __launch_bounds__(256) void table_scan_group_fill_kernel(AggAcc *__restrict__ groups, uint64_t n) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        groups[k] = AggAcc{0, 0, ~0ull, 0};
}
__global__ __launch_bounds__(256) void table_scan_group_finish_kernel(AggAcc *__restrict__ groups, uint64_t n,
                                                                      ScanAggCol col, bool fresh) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        groups[k] = group_record(fresh ? AggAcc{0, 0, ~0ull, 0} : groups[k], col);
}

// the LDS tier's grid: the aggregate's (a wave per leaf up to the grid cap -- a grid of a few
// workgroups per CU measured slower here as it did there), bounded so that the scratch tables
// stay within kGroupScratchMax: 16384 workgroups up to 127 groups, 8160 at 256
constexpr uint64_t kGroupScratchMax = 64ull << 20;
static bool group_lds_tier(uint32_t n_groups, const ScanGroupTuning &gt) {
    return n_groups <= (gt.lds_max < 0 || (uint32_t)gt.lds_max > kGroupLdsMax ? kGroupLdsMax : (uint32_t)gt.lds_max);
}
static int group_lds_blocks(uint32_t nl, uint32_t n_groups, const ScanTuning &tune) {
    const uint64_t bound = kGroupScratchMax / (((uint64_t)n_groups + 1) * sizeof(AggAcc));
    const int mb = max_blocks(tune);
    return grid_for(nl, 4, bound < (uint64_t)mb ? (int)bound : mb);
}

uint64_t table_scan_group_scratch_bytes(uint64_t nl, uint32_t n_groups, const ScanTuning &tune, const ScanGroupTuning &gt) {
    if (!nl || !group_lds_tier(n_groups, gt)) return 0;
    return (uint64_t)group_lds_blocks((uint32_t)nl, n_groups, tune) * ((uint64_t)n_groups + 1) * sizeof(AggAcc);
}

hipError_t launch_table_scan_group(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                                   const ScanPreds &preds, const ScanGroupSpec &grp, uint32_t agg_src, uint32_t agg_width,
                                   bool agg_signed, uint64_t *groups, uint8_t *scratch, hipStream_t s,
                                   const ScanTuning &tune, const ScanGroupTuning &gt) {
    if ((uint64_t)leaf0 + nl > t.nleaves || !groups || !preds_fit(t, preds)) return hipErrorInvalidValue;
    if (!column_fits(grp.width, grp.src, t.hstride) || grp.n == 0 || grp.n > kGroupMax) return hipErrorInvalidValue;
    if (agg_width && !column_fits(agg_width, agg_src, t.hstride)) return hipErrorInvalidValue;
    const ScanAggCol col{agg_src, agg_width, agg_signed ? 1u : 0u};
    AggAcc *out = reinterpret_cast<AggAcc *>(groups);
    const uint32_t n = grp.n + 1;
    const int fill_blocks = grid_for(((uint64_t)n + 255) / 256, 1, 2048);
    if (nl == 0) {
        table_scan_group_finish_kernel<<<fill_blocks, 256, 0, s>>>(out, n, col, true);
        return hipGetLastError();
    }
    const bool lds = group_lds_tier(grp.n, gt);
    if (lds && !scratch) return hipErrorInvalidValue;
    // combined by default: nothing in the LDS tier (64 lanes on one LDS entry measured no slower
    // than the shuffles that would spare them), the first lane's group in the global tier
    const uint32_t kmax = gt.combine >= 0 ? (uint32_t)gt.combine : lds ? 0u : 1u;
    const ScanGroupCol gc{grp.src, grp.width, grp.is_signed ? 1u : 0u, grp.n,
                          grp.is_signed ? grp.base ^ (1ull << 63) : grp.base, kmax};
    const ScanPreds p = order_domain(preds);
    if (lds) {
        const int blocks = group_lds_blocks(nl, grp.n, tune);
        const size_t shm = (size_t)n * sizeof(AggAcc);
        AggAcc *part = reinterpret_cast<AggAcc *>(scratch);
        if (snapshot) table_scan_group_kernel<true, true><<<blocks, 256, shm, s>>>(t, leaf0, nl, rid, p, gc, col, part);
        else table_scan_group_kernel<false, true><<<blocks, 256, shm, s>>>(t, leaf0, nl, rid, p, gc, col, part);
        table_scan_group_fold_kernel<<<n, 256, 0, s>>>(part, (uint32_t)blocks, n, col, out);
    } else {
        const int blocks = grid_for(nl, 4, max_blocks(tune));
        table_scan_group_fill_kernel<<<fill_blocks, 256, 0, s>>>(out, n);
        if (snapshot) table_scan_group_kernel<true, false><<<blocks, 256, 0, s>>>(t, leaf0, nl, rid, p, gc, col, out);
        else table_scan_group_kernel<false, false><<<blocks, 256, 0, s>>>(t, leaf0, nl, rid, p, gc, col, out);
        table_scan_group_finish_kernel<<<fill_blocks, 256, 0, s>>>(out, n, col, false);
    }
    return hipGetLastError();
}

}  // namespace stage
