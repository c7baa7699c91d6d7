// table_scan.hip -- gfx950 kernels of the whole-table scan (count, offsets, emit) and their launcher.
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
// tile's earlier leaves (one 256-B load) to the tile's offset.
constexpr uint32_t kTableScanMaxCap = 1024;  // slots per leaf the emit pass's LDS list holds

// what an emit launch carries (wave-uniform)
struct TableScanArgs {
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

// the emit pass, a wave per leaf: each 64-slot group's emitting lanes rank themselves by ballot,
// put their heap rows into the wave's LDS list by rank and write meta / status at their
// positions; the leaf's records then leave as consecutive rows (store_scan_rows) or windows
// (store_scan_windows), cut at max_records.  The counts of the leaf's tile, the tile's offset and
// the head words are loaded together before any of them is used, then the slot words of the
// lanes the head names: two round trips to the heap-row loads instead of four dependent ones.
template <bool VIS, bool WIN>
__global__ __launch_bounds__(256) void table_scan_emit_kernel(DevTable t, TableScanArgs g) {
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
        uint32_t v = lane < (uint32_t)(i & 63u) ? g.cnt[tile * 64 + lane] : 0u;
        const uint64_t tile0 = g.toff[tile];
        uint32_t rc = t.cap;
        if (!VIS)
            rc = *reinterpret_cast<const uint32_t *>(t.head + (uint64_t)leaf * t.head_bytes +
                                                     head_info_offset(t.cap, t.key_words)) & 0xFFFFu;
        uint64_t vm = VIS ? head_vis(t, leaf, 0) : 0ull;
        // the leaf's first position: its tile's offset and the tile's earlier leaves
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
        const uint64_t pos0 = tile0 + uni32(v);
        if (g.leaf_offsets && lane == 0) g.leaf_offsets[i] = pos0;
        if (pos0 >= g.max_records) continue;
        rc = uni32(rc);
        if (rc > t.cap) rc = t.cap;
        uint32_t produced = 0;
        for (uint32_t s = 0; s < spl && s * 64u < rc; ++s) {
            if (VIS && s) vm = head_vis(t, leaf, (int)s);
            bool on = VIS ? ((vm >> lane) & 1) != 0 : s * 64u + lane < rc;
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
                    on = meta != 0;  // 0: a deleted slot
                }
            }
            const uint64_t em = ballot(on);
            if (on) {
                const uint32_t r = produced + count_below(em);  // < cap
                rk[r] = img;
                const uint64_t k = pos0 + r;
                if (k < g.max_records) {
                    if (g.row_meta) g.row_meta[k] = meta;
                    if (g.row_status) g.row_status[k] = st;
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

uint64_t table_scan_scratch_bytes(uint64_t nl) { return ((nl + 63) / 64) * 8 + nl * 4; }

hipError_t launch_table_scan(const DevTable &t, uint32_t leaf0, uint32_t nl, bool snapshot, uint32_t rid,
                             uint32_t row_off, uint32_t len, uint32_t key_pad, const TableScanOut &o, uint8_t *scratch,
                             hipStream_t s, const ScanTuning &tune) {
    const bool win = len != 0;
    // the leaves exist, a leaf's records fit the emit pass's list, and the window and the key lie
    // inside a heap row (window_piece's and the key writer's loads rest on it)
    if ((uint64_t)leaf0 + nl > t.nleaves || t.cap > kTableScanMaxCap || !o.count) return hipErrorInvalidValue;
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
    uint32_t *cnt = reinterpret_cast<uint32_t *>(scratch + ntiles * 8);
    const int mb = max_blocks(tune);
    if (snapshot) table_scan_count_kernel<true><<<grid_for(ntiles, 4, mb), 256, 0, s>>>(t, leaf0, nl, cnt, toff);
    else table_scan_count_kernel<false><<<grid_for(ntiles, 4, mb), 256, 0, s>>>(t, leaf0, nl, cnt, toff);
    table_scan_offsets_kernel<<<1, 1024, 0, s>>>(toff, ntiles, o.count, o.leaf_offsets ? o.leaf_offsets + nl : nullptr);
    if (o.max_records || o.leaf_offsets) {
        const TableScanArgs g{leaf0, nl, cnt, toff, o.max_records, o.leaf_offsets, o.row_meta, o.row_status, o.recs,
                              ScanWindowArgs{WindowArgs{row_off, len, (len + 15u) >> 4, o.win}, o.row_keys, key_pad}, rid};
        const int blocks = grid_for(nl, 4, mb);
        if (snapshot) {
            if (win) table_scan_emit_kernel<true, true><<<blocks, 256, 0, s>>>(t, g);
            else table_scan_emit_kernel<true, false><<<blocks, 256, 0, s>>>(t, g);
        } else {
            if (win) table_scan_emit_kernel<false, true><<<blocks, 256, 0, s>>>(t, g);
            else table_scan_emit_kernel<false, false><<<blocks, 256, 0, s>>>(t, g);
        }
    }
    return hipGetLastError();
}

}  // namespace stage
