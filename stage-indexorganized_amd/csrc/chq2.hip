// chq2.hip -- CH-benCHmark Q2 (RunQuery2, benchmark/tpcc/tpcc_new_order.cpp:608-982) through the
// index-organized read path.
//
// Reference transaction at one read id:
//   1. REGION TableScan of 6 from key 0, NATION TableScan of 65 from key 0 (:650-761);
//   2. for the region named regions[target] (tpcc_record.h:931) and each of its nations, the
//      SUPPLIER table scan (scan_sz -1: every record, :779-797) filtered on SU_NATIONKEY;
//   3. per supplier: the STOCK point lookups {w, i} of its supp_stock_map entries
//      (tpcc_workload.cpp:398-404) -- a FAILURE read or a lookup with no tuple aborts; the
//      "minimum" keeps the LAST stock read because min_qty is never updated (:812-859);
//   4. the ITEM point lookup of that stock's S_I_ID (:862-887); I_DATA containing 'b' skips
//      the supplier (:890-892); otherwise S_QUANTITY < 10 updates S_QUANTITY..S_REMOTE_CNT to
//      (q + 50, ytd, order_cnt, remote_cnt) (:893-950), committed with the transaction.
//
// Here REGION / NATION run as device scans; four short kernels (q2_sel_*) read the SUPPLIER leaves
// slot by slot and select -- the region named regions[target], its nations, their suppliers in
// visiting order -- and lay out each visited supplier's supp_stock_map segment; the
// hot part -- every visited supplier's stock lookups (W * I / 10^4 each, ~2600 suppliers for
// EUROPE) and the item lookups -- is one gather kernel, one probe launch over all stock keys,
// their visibility folded at every read id of the batch (aborts and each supplier's last
// stock), one item probe launch and one finishing kernel that writes the records straight into
// the caller's page-locked `out`.  The counts stay on the device (the kernels read them there),
// so a batch has ONE host synchronisation, at its end (round 5; before, the host filtered the
// scans between two synchronisations).  Updates go through the device write path when a commit
// id is given.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "handle.hpp"
#include "tuple_read.hpp"
#include "visibility.hpp"
#include "wave.hpp"

using namespace stage_capi;

namespace stage {
namespace {

constexpr int kRegionScan = 6, kNationScan = 65;  // scan_sz of :653 and :734
constexpr uint32_t kIDataOff = 4 + 32 + 8;         // I_DATA in Item's payload (I_IM_ID, I_NAME, I_PRICE)
static const char *const kRegions[] = {"AFRICA", "AMERICA", "ASIA", "EUROPE", "MIDDLE EAST"};

// blocks copy the visited suppliers' map entries (2 words each) to their segments; counts[0] =
// the number of visited suppliers (q2_sel_start); nothing is written past m_cap keys (the host
// rejects counts above it after the batch)
__global__ void q2_gather(const uint64_t *__restrict__ map_keys, const uint64_t *__restrict__ src,
                          const uint64_t *__restrict__ dst, const uint32_t *__restrict__ cnt,
                          const uint64_t *__restrict__ counts, uint64_t m_cap, uint64_t *__restrict__ keys) {
    const uint64_t n = counts[0];
    for (uint64_t s = blockIdx.x; s < n; s += gridDim.x)
        for (uint32_t e = threadIdx.x; e < cnt[s] && dst[s] + e < m_cap; e += blockDim.x) {
            keys[2 * (dst[s] + e)] = map_keys[2 * (src[s] + e)];
            keys[2 * (dst[s] + e) + 1] = map_keys[2 * (src[s] + e) + 1];
        }
}

// RunQuery2's selection (tpcc_new_order.cpp:650-797) on the device, from the REGION / NATION scan
// rows and the SUPPLIER leaves (TableScanExecutor::ScanLeafNode with scan_sz -1, executor.h:
// 580-612: every slot of every leaf in leaf order, slots in slot order, raw records):
//   visits   = for each REGION row named the target (scan order), each NATION row of that region
//              (scan order); a nation is visited at most once (one region key per nation, region
//              keys unique), so at most kNationScan visits;
//   sel      = every SUPPLIER record of each visited nation, visit by visit, in slot order: a
//              stable counting sort by visit over 64-slot chunks --
//                q2_sel_count  (a wave per chunk) the visits, each slot's visit, its rank and its
//                              map entries' offset among its chunk's slots of that visit, the
//                              chunk's supplier and entry counts per visit (stored
//                              visit-major: a visit's chunks side by side);
//                q2_sel_start  (one block) each (visit, chunk)'s supplier and entry starts:
//                              visit, then chunk order;
//                q2_sel_place  (a lane per slot) sel[start + rank], the supplier's map segment
//                              (src, cnt) and its first STOCK key (dst = entry start + offset);
//   counts   = {suppliers, stock keys}.
// Every block derives the visits itself from the (L2-resident) scan rows, so no launch is spent
// on them; no loop waits on one global load per iteration.
constexpr int kVisits = kNationScan;
constexpr uint32_t kDirect = 1024;  // nation keys below this: a direct LDS map, the rest searched

struct VisitMap {  // nation key -> visit (LDS)
    int8_t dir[kDirect];
    int64_t big_key[kVisits];
    int32_t big_val[kVisits];
    uint32_t nbig, nv;
};

// the visit map of the target region, built by every block (blockDim.x >= 64)
__device__ void build_visits(VisitMap &vm, const uint8_t *regs, uint32_t rs, const uint8_t *nats, uint32_t ns,
                             uint64_t name0, uint64_t name1, uint64_t mask0, uint64_t mask1, uint8_t *s_rmatch,
                             uint8_t *s_flag) {
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t nreg = min(*reinterpret_cast<const uint32_t *>(regs - 8), (uint32_t)kRegionScan);
    const uint32_t nnat = min(*reinterpret_cast<const uint32_t *>(nats - 8), (uint32_t)kNationScan);
    for (uint32_t i = tid; i < kDirect; i += blockDim.x) vm.dir[i] = -1;
    if (tid == 0) vm.nbig = 0;
    // R_NAME == regions[target]: the bytes up to and including the target's NUL (< 16)
    if (tid < nreg) {
        const uint64_t *nm = reinterpret_cast<const uint64_t *>(regs + (uint64_t)tid * rs + 8);
        s_rmatch[tid] = ((nm[0] ^ name0) & mask0) == 0 && ((nm[1] ^ name1) & mask1) == 0;
    }
    __syncthreads();
    const uint32_t nf = nreg * nnat;  // flag f = (region row f / nnat, nation row f % nnat), visit order
    for (uint32_t f = tid; f < nf; f += blockDim.x) {
        const uint32_t r = f / nnat, a = f % nnat;
        s_flag[f] = s_rmatch[r] && *reinterpret_cast<const int64_t *>(nats + (uint64_t)a * ns + 8) ==
                                       *reinterpret_cast<const int64_t *>(regs + (uint64_t)r * rs);
    }
    __syncthreads();
    if (tid < 64) {  // wave 0 numbers the flagged (region, nation) pairs in order
        uint32_t base = 0;
        for (uint32_t f0 = 0; f0 < nf; f0 += 64) {
            const uint32_t f = f0 + lane;
            const bool fl = f < nf && s_flag[f];
            const uint64_t b = ballot(fl);
            if (fl) {
                const uint32_t idx = base + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1));
                const int64_t nk = *reinterpret_cast<const int64_t *>(nats + (uint64_t)(f % nnat) * ns);
                if (idx < (uint32_t)kVisits) {
                    if (nk >= 0 && nk < (int64_t)kDirect) {
                        vm.dir[nk] = (int8_t)idx;
                    } else {
                        const uint32_t k = atomicAdd(&vm.nbig, 1u);
                        vm.big_key[k] = nk;
                        vm.big_val[k] = (int32_t)idx;
                    }
                }
            }
            base += (uint32_t)__builtin_popcountll(b);
        }
        if (lane == 0) vm.nv = min(base, (uint32_t)kVisits);
    }
    __syncthreads();
}

__device__ __forceinline__ int visit_of(const VisitMap &vm, uint64_t nat) {
    if ((int64_t)nat >= 0 && (int64_t)nat < (int64_t)kDirect) return vm.dir[nat];
    for (uint32_t k = 0; k < vm.nbig; ++k)
        if (vm.big_key[k] == (int64_t)nat) return vm.big_val[k];
    return -1;
}

// a wave per 64-slot chunk of the SUPPLIER leaves (blocks of 4 waves)
__global__ __launch_bounds__(256) void q2_sel_count(const uint8_t *__restrict__ regs, uint32_t rs,
                                                    const uint8_t *__restrict__ nats, uint32_t ns, uint64_t name0,
                                                    uint64_t name1, uint64_t mask0, uint64_t mask1, DevTable t,
                                                    uint32_t kpad, uint64_t nchunks, const uint32_t *__restrict__ map_off,
                                                    int8_t *__restrict__ g_vis, uint8_t *__restrict__ g_rank,
                                                    uint32_t *__restrict__ g_koff, uint64_t *__restrict__ g_key,
                                                    uint32_t *__restrict__ ccnt, uint32_t *__restrict__ kcnt,
                                                    uint32_t *__restrict__ g_nv) {
    __shared__ VisitMap vm;
    __shared__ uint8_t s_rmatch[kRegionScan];
    __shared__ uint8_t s_flag[kRegionScan * kNationScan];
    __shared__ uint32_t s_cnt[4][kVisits], s_kcnt[4][kVisits];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t c = (uint64_t)blockIdx.x * 4 + wv;
    // the slot's record first -- slot word, key, nation key, map segment: none of it depends on
    // the visits, so these dependent loads overlap build_visits' own (the scan rows)
    const uint64_t i = c * 64 + lane;
    uint64_t key = ~0ull, nat = 0;
    uint32_t ma = 0, mb = 0;
    if (c < nchunks) {
        const SlotInfo si = t.slot[i];
        if (si.meta != 0) {
            const uint8_t *row = t.heap + (uint64_t)si.image * t.hstride;
            key = *reinterpret_cast<const uint64_t *>(row);
            nat = *reinterpret_cast<const uint64_t *>(row + kpad);
        }
        if (key < 10000) ma = map_off[key], mb = map_off[key + 1];
    }
    build_visits(vm, regs, rs, nats, ns, name0, name1, mask0, mask1, s_rmatch, s_flag);
    if (blockIdx.x == 0 && threadIdx.x == 0) *g_nv = vm.nv;
    if (c >= nchunks) return;
    for (uint32_t v = lane; v < (uint32_t)kVisits; v += 64) s_cnt[wv][v] = 0, s_kcnt[wv][v] = 0;
    const int v = key == ~0ull ? -1 : visit_of(vm, nat);
    // the supplier's supp_stock_map entries (keys below 10000)
    const uint32_t mc = v >= 0 && key < 10000 && mb > ma ? mb - ma : 0;
    // per visit present in the chunk: each slot's rank and its entries' offset among the
    // chunk's slots of that visit, the visit's supplier and entry counts
    uint32_t rank = 0, koff = 0;
    uint64_t todo = ballot(v >= 0);
    while (todo) {
        const int vl = (int)rl32((uint32_t)v, (int)__builtin_ctzll(todo));
        const bool in = v == vl;
        const uint64_t mm = ballot(in);
        const uint32_t x = in ? mc : 0u;
        uint32_t y = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t z = __shfl_up(y, o, 64);
            if (lane >= (uint32_t)o) y += z;
        }
        if (in) {
            rank = (uint32_t)__builtin_popcountll(mm & ((1ull << lane) - 1));
            koff = y - x;
        }
        const uint32_t ktot = rl32(y, 63);
        if (lane == 0) {
            s_cnt[wv][vl] = (uint32_t)__builtin_popcountll(mm);
            s_kcnt[wv][vl] = ktot;
        }
        todo &= ~mm;
    }
    g_vis[i] = (int8_t)v;
    g_rank[i] = (uint8_t)rank;
    g_koff[i] = koff;
    g_key[i] = key;
    for (uint32_t w = lane; w < vm.nv; w += 64) {  // visit-major: q2_sel_start reads a visit's chunks coalesced
        ccnt[(uint64_t)w * nchunks + c] = s_cnt[wv][w];
        kcnt[(uint64_t)w * nchunks + c] = s_kcnt[wv][w];
    }
}

// one block, after q2_sel_count: the (visit, chunk) supplier counts ccnt and entry counts kcnt
// (visit-major) -> their starts, in place (visit, then chunk order); counts = {suppliers, stock
// keys}.  A wave per visit; lane l takes chunks l, l + 64, ... so each load and store of the
// wave is 64 consecutive words; 16 chunks per lane in flight at once.  (Round 6: a lane per
// contiguous run of chunks in the chunk-major layout made every load touch 64 lines -- ~10 K
// line requests through the block's one CU, ~13 µs of the chain.)
constexpr uint32_t kSelBatch = 16;
__device__ __forceinline__ void load_batch(const uint32_t *__restrict__ ccnt, const uint32_t *__restrict__ kcnt,
                                           uint64_t row, uint64_t nchunks, uint64_t c0, uint32_t lane,
                                           uint32_t (&x0)[kSelBatch], uint32_t (&x1)[kSelBatch]) {
#pragma unroll
    for (uint32_t k = 0; k < kSelBatch; ++k) {  // unconditional loads (an index past the end re-reads chunk 0)
        const uint64_t c = c0 + k * 64 + lane;
        const uint64_t at = row + (c < nchunks ? c : 0);
        x0[k] = ccnt[at];
        x1[k] = kcnt[at];
    }
#pragma unroll
    for (uint32_t k = 0; k < kSelBatch; ++k) {
        const bool in = c0 + k * 64 + lane < nchunks;
        x0[k] = in ? x0[k] : 0u;
        x1[k] = in ? x1[k] : 0u;
    }
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t y, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t z = __shfl_up(y, o, 64);
        if (lane >= (uint32_t)o) y += z;
    }
    return y;
}

__global__ __launch_bounds__(1024) void q2_sel_start(uint32_t *__restrict__ ccnt, uint32_t *__restrict__ kcnt,
                                                     uint64_t nchunks, const uint32_t *__restrict__ g_nv,
                                                     uint64_t *__restrict__ counts) {
    __shared__ uint32_t s_tot[2][kVisits];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const uint32_t nv = *g_nv;
    for (uint32_t v = wv; v < nv; v += nw) {  // the visit's totals
        uint32_t t0 = 0, t1 = 0;
        for (uint64_t c0 = 0; c0 < nchunks; c0 += 64 * kSelBatch) {
            uint32_t x0[kSelBatch], x1[kSelBatch];
            load_batch(ccnt, kcnt, (uint64_t)v * nchunks, nchunks, c0, lane, x0, x1);
#pragma unroll
            for (uint32_t k = 0; k < kSelBatch; ++k) t0 += x0[k], t1 += x1[k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t0 += __shfl_xor(t0, o, 64), t1 += __shfl_xor(t1, o, 64);
        if (lane == 0) s_tot[0][v] = t0, s_tot[1][v] = t1;
    }
    __syncthreads();
    if (tid < 2) {
        uint32_t pos = 0;
        for (uint32_t v = 0; v < nv; ++v) {
            const uint32_t t = s_tot[tid][v];
            s_tot[tid][v] = pos;
            pos += t;
        }
        counts[tid] = pos;
    }
    __syncthreads();
    for (uint32_t v = wv; v < nv; v += nw) {  // exclusive scan over the chunks, in place
        uint32_t p0 = s_tot[0][v], p1 = s_tot[1][v];  // the start of the next 64 chunks
        const uint64_t row = (uint64_t)v * nchunks;
        for (uint64_t c0 = 0; c0 < nchunks; c0 += 64 * kSelBatch) {
            uint32_t x0[kSelBatch], x1[kSelBatch];
            load_batch(ccnt, kcnt, row, nchunks, c0, lane, x0, x1);
#pragma unroll
            for (uint32_t k = 0; k < kSelBatch; ++k) {
                const uint64_t c = c0 + k * 64 + lane;
                const uint32_t y0 = wave_incl_scan(x0[k], lane), y1 = wave_incl_scan(x1[k], lane);
                if (c < nchunks) ccnt[row + c] = p0 + y0 - x0[k], kcnt[row + c] = p1 + y1 - x1[k];
                p0 += rl32(y0, 63);
                p1 += rl32(y1, 63);
            }
        }
    }
}

// a lane per slot: each selected supplier at its place, with its supp_stock_map segment (src,
// cnt) and the segment's offset among all looked-up STOCK keys (dst)
__global__ void q2_sel_place(const uint32_t *__restrict__ ccnt, const uint32_t *__restrict__ kcnt, uint64_t nslots,
                             const int8_t *__restrict__ g_vis, const uint8_t *__restrict__ g_rank,
                             const uint32_t *__restrict__ g_koff, const uint64_t *__restrict__ g_key,
                             const uint32_t *__restrict__ map_off, uint64_t *__restrict__ sel,
                             uint64_t *__restrict__ src, uint32_t *__restrict__ cnt, uint64_t *__restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nslots) return;
    const int v = g_vis[i];
    if (v < 0) return;
    const uint64_t g = (uint64_t)v * (nslots >> 6) + (i >> 6);  // visit-major (q2_sel_start)
    const uint32_t pos = ccnt[g] + g_rank[i];
    const uint64_t sk = g_key[i];
    uint64_t s0 = 0, c = 0;
    if (sk < 10000) {
        const uint32_t a = map_off[sk], b = map_off[sk + 1];
        s0 = a;
        c = b > a ? b - a : 0;
    }
    sel[pos] = sk;
    src[pos] = s0;
    cnt[pos] = (uint32_t)c;
    dst[pos] = (uint64_t)kcnt[g] + g_koff[i];
}

// q2_sel_start + q2_sel_place + q2_gather in one launch, for SUPPLIER tables of at most
// kPlaceChunks 64-slot chunks.  A block of 16 waves per 4 chunks (sel_count's chunks of a block):
//   1. per visit, a wave sums the (visit, chunk) counts of every chunk and of the chunks before
//      the block's first (coalesced loads, L2-resident: ~26 KB per block at 256 chunks and 13
//      visits) -- one load round when the visits fit the 16 waves -- and keeps the block's own
//      chunks' counts in LDS; the visit totals are scanned in LDS (block 0 writes counts);
//   2. a thread per slot of the 4 chunks places its supplier as q2_sel_place and lists it;
//   3. the block's listed suppliers' map segments are copied as q2_gather, a wave per supplier,
//      each segment's loads issued together (up to 256 entries of 16 B per round).
// Removes two launches and the one-block scan from the chain (round 6).
constexpr uint64_t kPlaceChunks = 1024;
__global__ __launch_bounds__(1024) void q2_place(const uint32_t *__restrict__ ccnt, const uint32_t *__restrict__ kcnt,
                                                 uint64_t nchunks, const uint32_t *__restrict__ g_nv,
                                                 const int8_t *__restrict__ g_vis, const uint8_t *__restrict__ g_rank,
                                                 const uint32_t *__restrict__ g_koff, const uint64_t *__restrict__ g_key,
                                                 const uint32_t *__restrict__ map_off, const uint64_t *__restrict__ map_keys,
                                                 uint64_t m_cap, uint64_t *__restrict__ sel, uint64_t *__restrict__ src,
                                                 uint32_t *__restrict__ cnt, uint64_t *__restrict__ dst,
                                                 uint64_t *__restrict__ counts, uint64_t *__restrict__ keys) {
    __shared__ uint32_t s_base[2][kVisits];  // visit start + the counts of chunks before the block's first
    __shared__ uint32_t s_tot[2][kVisits];
    __shared__ uint32_t s_loc[2][4][kVisits];  // the block's own chunks' counts
    __shared__ uint64_t s_a[256], s_d[256];    // listed suppliers: map segment start, first STOCK key
    __shared__ uint32_t s_m[256], s_n;         // ... entry count; list length
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const uint64_t c_first = (uint64_t)blockIdx.x * 4;
    // the slot's selection (threads 0..255: the block's 4 chunks) first, its map segment next:
    // independent of the counts, so these loads overlap the count pass below
    const bool slot_thread = tid < 256 && c_first + (tid >> 6) < nchunks;
    const uint64_t i = (c_first + (tid >> 6)) * 64 + lane;
    int v_i = -1;
    uint32_t rank_i = 0, koff_i = 0, lo_i = 0, hi_i = 0;
    uint64_t key_i = ~0ull;
    if (slot_thread) {
        v_i = g_vis[i];
        rank_i = g_rank[i];
        koff_i = g_koff[i];
        key_i = g_key[i];
        if (key_i < 10000) lo_i = map_off[key_i], hi_i = map_off[key_i + 1];
    }
    const uint32_t nv = *g_nv;
    if (tid == 0) s_n = 0;
    for (uint32_t j = tid; j < 2 * 4 * kVisits; j += blockDim.x)  // chunks past the table's end
        if (c_first + (j / kVisits) % 4 >= nchunks) (&s_loc[0][0][0])[j] = 0;
    for (uint32_t v = wv; v < nv; v += nw) {
        uint32_t t0 = 0, t1 = 0, p0 = 0, p1 = 0;
        for (uint64_t c0 = 0; c0 < nchunks; c0 += 64 * kSelBatch) {
            uint32_t x0[kSelBatch], x1[kSelBatch];
            load_batch(ccnt, kcnt, (uint64_t)v * nchunks, nchunks, c0, lane, x0, x1);
#pragma unroll
            for (uint32_t k = 0; k < kSelBatch; ++k) {
                const uint64_t c = c0 + k * 64 + lane;
                t0 += x0[k], t1 += x1[k];
                if (c < c_first) p0 += x0[k], p1 += x1[k];
                if (c >= c_first && c < c_first + 4 && c < nchunks)
                    s_loc[0][c - c_first][v] = x0[k], s_loc[1][c - c_first][v] = x1[k];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            t0 += __shfl_xor(t0, o, 64), t1 += __shfl_xor(t1, o, 64);
            p0 += __shfl_xor(p0, o, 64), p1 += __shfl_xor(p1, o, 64);
        }
        if (lane == 0) s_tot[0][v] = t0, s_tot[1][v] = t1, s_base[0][v] = p0, s_base[1][v] = p1;
    }
    __syncthreads();
    if (tid < 2) {
        uint32_t pos = 0;
        for (uint32_t v = 0; v < nv; ++v) {
            s_base[tid][v] += pos;
            pos += s_tot[tid][v];
        }
        if (blockIdx.x == 0) counts[tid] = pos;
    }
    __syncthreads();
    if (slot_thread && v_i >= 0) {
        const uint32_t j = tid >> 6, v = (uint32_t)v_i;  // the block's chunk, the slot's visit
        uint32_t pos = s_base[0][v] + rank_i, kpos = s_base[1][v] + koff_i;
        for (uint32_t jj = 0; jj < j; ++jj) pos += s_loc[0][jj][v], kpos += s_loc[1][jj][v];
        const uint32_t m = key_i < 10000 && hi_i > lo_i ? hi_i - lo_i : 0;
        sel[pos] = key_i;
        src[pos] = lo_i;
        cnt[pos] = m;
        dst[pos] = kpos;
        if (m) {
            const uint32_t k = atomicAdd(&s_n, 1u);
            s_a[k] = lo_i;
            s_d[k] = kpos;
            s_m[k] = m;
        }
    }
    __syncthreads();
    const uint32_t nl = s_n;
    for (uint32_t k = wv; k < nl; k += nw) {  // a wave per listed supplier
        const uint64_t a = s_a[k], d = s_d[k];
        const uint32_t m = s_m[k];
        for (uint32_t e0 = 0; e0 < m; e0 += 256) {
            u32x4 x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t e = e0 + r * 64 + lane;
                if (e < m && d + e < m_cap) x[r] = reinterpret_cast<const u32x4 *>(map_keys)[a + e];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t e = e0 + r * 64 + lane;
                if (e < m && d + e < m_cap) reinterpret_cast<u32x4 *>(keys)[d + e] = x[r];
            }
        }
    }
}

// thread per (query q, supplier s): the abort for a stock lookup that produced no tuple is already
// in abort_flag (launch_revisit_segments); the last entry's stock probe, its hit re-evaluated at
// q's read id here (revisit_one), gives (w, i, quantity, ytd, order_cnt, remote_cnt) and the item key
__global__ void q2_reduce(DevTable st, const stage_probe_out_dev *__restrict__ sbase, const uint32_t *__restrict__ rids,
                          const uint64_t *__restrict__ skeys, const uint64_t *__restrict__ dst,
                          const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ supp, uint32_t skpad,
                          const uint64_t *__restrict__ counts, uint32_t nq, stage_q2_rec *__restrict__ out,
                          uint64_t *__restrict__ ikeys) {
    const uint32_t n = (uint32_t)counts[0];
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;  // q * n + s
    if (g >= n * nq) return;
    const uint32_t s = g % n, q = g / n;
    const uint64_t kb = dst[s];
    const uint32_t c = cnt[s];
    stage_q2_rec r;
    memset(&r, 0, sizeof(r));
    r.supp_key = (int64_t)supp[s];
    if (c) {  // stock_0 / stock_1 of the last lookup (a supplier without stocks keeps zeros)
        const uint64_t klast = kb + c - 1;
        r.s_w_id = (int64_t)skeys[2 * klast];
        r.s_i_id = (int64_t)skeys[2 * klast + 1];
        const u32x4 *bp = reinterpret_cast<const u32x4 *>(sbase + klast);
        u32x4 a = bp[0], b = bp[1];
        revisit_one(st, rids[q], a, b);
        if (produced_tuple(a.x & 0xFF)) {
            const uint8_t *row = st.heap + (uint64_t)b.z * st.hstride + skpad;
            r.s_quantity = ld_i32(row);
            r.s_ytd = ld_i32(row + 4);
            r.s_order_cnt = ld_i32(row + 8);
            r.s_remote_cnt = ld_i32(row + 12);
        }
    }
    out[g] = r;
    ikeys[g] = (uint64_t)r.s_i_id;
}

// item outcome: no tuple aborts; I_DATA up to its first NUL containing 'b' skips; else a
// quantity below 10 marks the update
// ... and each record into the caller's page-locked records (host_out, row pitch max_out; null:
// the records stay in `out` on the device).  The host writes cross PCIe: a block's 256 records
// (48 B each) are staged in LDS and leave as 16-B chunks, consecutive lanes on consecutive
// chunks (a wave's store is 1 KB of one run of records), not as 48-B-strided lane stores.
// slot_out (split emit, host_out null): the records into the batch slot's own device buffer, row
// pitch slot_pitch (query q's supplier k at q * slot_pitch + k), for the side stream's copy to
// the caller.
static_assert(sizeof(stage_q2_rec) == 48, "three 16-B chunks per record");
__global__ __launch_bounds__(256) void q2_finish(DevTable it, const stage_probe_out_dev *__restrict__ ibase,
                                                 const uint32_t *__restrict__ rids, uint32_t ikpad,
                                                 const uint64_t *__restrict__ counts,
                                                 uint32_t nq, stage_q2_rec *__restrict__ out, int32_t *__restrict__ abort_flag,
                                                 stage_q2_rec *__restrict__ host_out, uint64_t max_out,
                                                 stage_q2_rec *__restrict__ slot_out, uint64_t slot_pitch) {
    __shared__ u32x4 s_rec[256 * 3];
    const uint32_t n = (uint32_t)counts[0];
    const uint64_t total = (uint64_t)n * nq;
    const uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x;
    const uint64_t s = g0 + threadIdx.x;  // q * n + supplier
    if (g0 >= total) return;  // block-uniform
    if (s < total) {
        // the supplier's item probe, its hit re-evaluated at the query's read id (revisit_one)
        const u32x4 *bp = reinterpret_cast<const u32x4 *>(ibase + s % n);
        u32x4 ia = bp[0], ib = bp[1];
        revisit_one(it, rids[s / n], ia, ib);
        const uint32_t st = ia.x & 0xFF;
        stage_q2_rec r = out[s];
        if (!produced_tuple(st)) {
            atomicOr(abort_flag + s / n, 1);
        } else {
            // I_DATA's 64 bytes in 16 word loads issued together (4-B aligned), scanned in registers
            const uint32_t *d =
                reinterpret_cast<const uint32_t *>(it.heap + (uint64_t)ib.z * it.hstride + ikpad + kIDataOff);
            uint32_t w[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k] = d[k];
            uint8_t has_b = 0;
            bool end = false;
#pragma unroll
            for (int c = 0; c < 64; ++c) {
                const uint8_t ch = (uint8_t)(w[c >> 2] >> (8 * (c & 3)));
                end |= ch == 0;
                has_b |= !end && ch == 'b';
            }
            r.item_has_b = has_b;
            r.update = !has_b && r.s_quantity < 10;
            out[s] = r;
        }
        u32x4 rv[3];
        memcpy(rv, &r, sizeof(r));
#pragma unroll
        for (int k = 0; k < 3; ++k) s_rec[threadIdx.x * 3 + k] = rv[k];
        if (slot_out) {
            u32x4 *so = reinterpret_cast<u32x4 *>(slot_out + (s / n) * slot_pitch + s % n);
#pragma unroll
            for (int k = 0; k < 3; ++k) so[k] = rv[k];
        }
    }
    if (!host_out) return;  // uniform
    __syncthreads();
    const uint64_t nrec = total - g0 < 256 ? total - g0 : 256;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t c = k * 256 + threadIdx.x;  // chunk c: record c / 3, part c % 3
        const uint64_t rec = g0 + c / 3;
        if (c / 3 < nrec && rec % n < max_out)
            reinterpret_cast<u32x4 *>(host_out + (rec / n) * max_out + rec % n)[c % 3] = s_rec[c];
    }
}

// ---- the host driver: q2_run = check, plan, bind, order, replay or enqueue, collect ----

// a running offset rounded up to 256 bytes: the staging and scratch layouts
struct Carve {
    uint64_t off = 0;
    uint64_t take(uint64_t bytes) {
        const uint64_t o = off;
        off += (bytes + 255) & ~255ull;
        return o;
    }
};

constexpr uint32_t kMapKeys = 10000;  // supp_stock_map's keys (map_off: one more entry)

// One call's sizes and layouts (q2_plan), then its buffers (q2_stage, q2_bind)
struct Q2Plan {
    // upper bounds (buffer sizes, grids): every SUPPLIER slot visited, every map entry looked up;
    // launch shapes from the previous call's counts (the visited set depends on the data only)
    uint64_t nslots, nchunks, n_max, m_max, n_hint, m_hint;
    uint32_t nat_scan;  // NATION's scan size
    bool fused_place;   // q2_place instead of q2_sel_start, q2_sel_place and q2_gather
    // pinned call staging mirrored at the head of the device scratch: [map_off][read ids]
    // [aborted] go down in one copy; [counts][aborted] come back in one copy; q_zero: the
    // REGION / NATION scans' start key, 0 (:653, :734)
    uint64_t q_map, q_rq, q_cn, q_ab, q_zero, q_end;
    // the SUPPLIER table's scratch (REGION's and NATION's hold their scan rows)
    uint64_t o_mir, o_pairs, o_sel, o_src, o_cnt, o_dst, o_keys, o_sbase, o_ik, o_ibase, o_rec, o_vis, o_rank, o_koff,
        o_ccnt, o_kcnt, o_nv, scratch, reg_rows, nat_rows;
    uint8_t *pq, *buf, *mir;  // the staging, the scratch, the staging's mirror in it
    const uint32_t *d_map, *d_rq;
    const uint64_t *d_zero;
    uint64_t *d_counts, *d_sel, *d_src, *d_dst, *d_keys, *d_ik, *g_key;
    int32_t *d_ab;
    uint32_t *d_cnt, *ccnt, *kcnt, *g_koff, *g_nv;
    stage_probe_out_dev *d_sbase, *d_ibase;
    stage_q2_rec *d_rec;
    int8_t *g_vis;
    uint8_t *g_rank, *regs, *nats;  // regs / nats: the scans' first rows, each count (u32) 8 bytes before
};

// Everything q2_enqueue reads.  The struct is zeroed before it is filled (q2_run) and its bytes
// are the graph key (q2_key): an argument cannot reach a launch without entering the key.
struct Q2Launch {
    Q2Plan p;
    DevTable rv, nv, pv, iv, sv;  // REGION, NATION, SUPPLIER, ITEM, STOCK
    ProbeTuning stock_tune, item_tune;
    ScanTuning region_scan, nation_scan;
    uint32_t supplier_kpad, item_kpad, stock_kpad;
    const uint64_t *d_map_keys;
    uint64_t name0, name1, mask0, mask1;  // regions[target] and its NUL as two masked words
    uint32_t nq;
    uint64_t max_out;
    stage_q2_rec *host_out, *slot_out;  // the caller's page-locked records / the slot's device buffer
    bool split;
    hipStream_t s;
};

// the key of a call's captured graph: the launch arguments, and what the call depends on beyond
// them -- the tables' own streams and scratch buffers
std::string q2_key(const Q2Launch &L, std::initializer_list<const stage_table *> tables) {
    std::string key;
    key.reserve(sizeof L + tables.size() * (sizeof(hipStream_t) + sizeof(void *)));
    key.append((const char *)&L, sizeof L);
    for (const stage_table *t : tables) {
        key.append((const char *)&t->dev.stream, sizeof t->dev.stream);
        key.append((const char *)&t->dev.scratch.p, sizeof t->dev.scratch.p);
    }
    return key;
}

// everything up to the batch's one synchronisation, enqueued on L.s
void q2_enqueue(const Q2Launch &L) {
    const Q2Plan &p = L.p;
    hipStream_t s = L.s;
    hip_check(hipMemcpyAsync(p.mir, p.pq, p.q_end, hipMemcpyHostToDevice, s), "h2d");
    // 1. the REGION / NATION scans (TableScanExecutor rows from key 0): one launch when
    // launch_scan_pair takes them, else one each
    auto cnt = [](uint8_t *rows) { return (uint32_t *)(rows - 8); };
    if (scan_pair_supported(L.rv, kRegionScan, L.nv, p.nat_scan)) {
        hip_check(launch_scan_pair(L.rv, p.d_zero, kRegionScan, cnt(p.regs), p.regs, L.nv, p.d_zero, p.nat_scan,
                                   cnt(p.nats), p.nats, s),
                  "scan pair");
    } else {
        hip_check(launch_scan(L.rv, p.d_zero, nullptr, 1, kRegionScan, cnt(p.regs), p.regs, s, L.region_scan), "scan");
        hip_check(launch_scan(L.nv, p.d_zero, nullptr, 1, p.nat_scan, cnt(p.nats), p.nats, s, L.nation_scan), "scan");
    }
    // 2. the selection and the map segments, on the device (four kernels, no host wait)
    if (p.nchunks) {
        q2_sel_count<<<(unsigned)((p.nchunks + 3) / 4), 256, 0, s>>>(
            p.regs, L.rv.stride, p.nats, L.nv.stride, L.name0, L.name1, L.mask0, L.mask1, L.pv, L.supplier_kpad,
            p.nchunks, p.d_map, p.g_vis, p.g_rank, p.g_koff, p.g_key, p.ccnt, p.kcnt, p.g_nv);
        if (p.fused_place) {  // starts, places and the STOCK keys in one launch
            q2_place<<<(unsigned)((p.nchunks + 3) / 4), 1024, 0, s>>>(
                p.ccnt, p.kcnt, p.nchunks, p.g_nv, p.g_vis, p.g_rank, p.g_koff, p.g_key, p.d_map, L.d_map_keys, p.m_max,
                p.d_sel, p.d_src, p.d_cnt, p.d_dst, p.d_counts, p.d_keys);
        } else {
            q2_sel_start<<<1, 1024, 0, s>>>(p.ccnt, p.kcnt, p.nchunks, p.g_nv, p.d_counts);
            q2_sel_place<<<(unsigned)((p.nslots + 255) / 256), 256, 0, s>>>(p.ccnt, p.kcnt, p.nslots, p.g_vis, p.g_rank,
                                                                             p.g_koff, p.g_key, p.d_map, p.d_sel,
                                                                             p.d_src, p.d_cnt, p.d_dst);
        }
    }
    hip_check(hipGetLastError(), "select");
    // 3. every visited supplier's STOCK keys, one probe of them all (the counts on the device)
    if (!p.fused_place)
        q2_gather<<<(unsigned)std::max<uint64_t>(std::min<uint64_t>(p.n_hint, 4096), 1), 256, 0, s>>>(
            L.d_map_keys, p.d_src, p.d_dst, p.d_cnt, p.d_counts, p.m_max, p.d_keys);
    // every query of the batch looks up the same STOCK keys (the visited suppliers and their
    // supp_stock_map do not depend on the read id): each key is probed once, with no read id
    // (the hit slot does not depend on it), and its visibility evaluated at every query's read
    // id inside the per-supplier fold (launch_revisit_segments: the aborts and each
    // supplier's last stock, per query)
    // (the misses at every read id folded into the probe where its kernel takes them;
    // q2_reduce re-evaluates each supplier's last lookup)
    if (p.m_max && probe_missed_supported(L.sv)) {
        hip_check(launch_probe_missed(L.sv, p.d_keys, p.m_max, p.d_sbase, s, L.stock_tune, p.d_counts + 1, p.m_hint,
                                      p.d_rq, L.nq, p.d_ab),
                  "stock probe");
    } else if (p.m_max) {
        hip_check(launch_probe(L.sv, p.d_keys, nullptr, nullptr, nullptr, p.m_max, p.d_sbase, nullptr, s, L.stock_tune,
                               p.d_counts + 1, p.m_hint),
                  "stock probe");
        hip_check(launch_revisit_segments(L.sv, p.d_sbase, p.m_max, nullptr, nullptr, 0, p.d_rq, L.nq, nullptr, p.d_ab,
                                          s, p.d_counts + 1, nullptr),
                  "stock read ids");
    }
    q2_reduce<<<(unsigned)((p.n_max * L.nq + 255) / 256), 256, 0, s>>>(L.sv, p.d_sbase, p.d_rq, p.d_keys, p.d_dst,
                                                                       p.d_cnt, p.d_sel, L.stock_kpad, p.d_counts, L.nq,
                                                                       p.d_rec, p.d_ik);
    // 4. item lookups of the last stocks (the same keys in every query: probed once, as above),
    // the I_DATA filter, the records into `out`
    hip_check(launch_probe(L.iv, p.d_ik, nullptr, nullptr, nullptr, p.n_max, p.d_ibase, nullptr, s, L.item_tune,
                           p.d_counts, p.n_hint),
              "item probe");
    q2_finish<<<(unsigned)((p.n_max * L.nq + 255) / 256), 256, 0, s>>>(L.iv, p.d_ibase, p.d_rq, L.item_kpad, p.d_counts,
                                                                       L.nq, p.d_rec, p.d_ab,
                                                                       L.split ? nullptr : L.host_out, L.max_out,
                                                                       L.slot_out, p.n_max);
    hip_check(hipGetLastError(), "q2 kernels");
    hip_check(hipMemcpyAsync(p.pq + p.q_cn, p.d_counts, 16 + L.nq * 4ull, hipMemcpyDeviceToHost, s), "d2h");
}

// STAGE_Q2_TRACE=1: host wall time of each phase on stderr
struct Q2Trace {
    static bool on() {
        static const bool t = std::getenv("STAGE_Q2_TRACE") != nullptr;
        return t;
    }
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char *what) const {
        if (on())
            std::fprintf(stderr, "[q2] %s %.1f us\n", what,
                         std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
};

// A hipGraph of an enqueue on one stream: captured on the second call in a row with the same key,
// replayed while the key stays the same -- one launch instead of ~20 (STAGE_Q2_GRAPH=0: always
// enqueue).  A capture or instantiation that fails is not tried again.  Returns what it did.
template <class F>
const char *replay_or_enqueue(Q2Graph &G, const std::string &key, hipStream_t s, F enqueue) {
    static const bool graphs = [] {
        const char *e = std::getenv("STAGE_Q2_GRAPH");
        return !(e && std::strcmp(e, "0") == 0);
    }();
    const char *how = "enqueued";
    bool launched = false;
    if (graphs && !G.failed) {
        if (G.exec && G.key == key) {
            hip_check(hipGraphLaunch(G.exec, s), "q2 graph launch");
            how = "replayed", launched = true;
        } else if (G.last_key == key) {  // the same call twice: capture it
            if (G.exec) (void)hipGraphExecDestroy(G.exec);
            G.exec = nullptr;
            G.key.clear();
            hipGraph_t g = nullptr;
            hip_check(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed), "q2 capture");
            try {
                enqueue();
            } catch (...) {
                (void)hipStreamEndCapture(s, &g);
                if (g) (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                throw;
            }
            hipError_t e = hipStreamEndCapture(s, &g);
            if (!e) e = hipGraphInstantiate(&G.exec, g, nullptr, nullptr, 0);
            if (g) (void)hipGraphDestroy(g);
            if (e) {  // no graph for this call shape: enqueue as before from now on
                (void)hipGetLastError();
                G.exec = nullptr;
                G.failed = true;
                if (Q2Trace::on()) std::fprintf(stderr, "[q2] graph capture failed: %s\n", hipGetErrorString(e));
            } else {
                G.key = key;
                hip_check(hipGraphLaunch(G.exec, s), "q2 graph launch");
                how = "captured", launched = true;
            }
        }
        G.last_key = key;
    }
    if (!launched) enqueue();
    return how;
}

}  // namespace
}  // namespace stage

using namespace stage;

// CH-Q2's users of the tables' per-call scratch, by table role (check_scratch_uses)
enum { kRoleRegion, kRoleNation, kRoleSupplier, kRoleItem, kRoleStock };
static const ScratchUse kQ2Scratch[] = {{kRoleSupplier, "the CH-Q2 batch buffers"},
                                        {kRoleRegion, "the REGION scan rows"},
                                        {kRoleNation, "the NATION scan rows"},
                                        {kRoleItem, "the stock-update staging"}};
constexpr int kQ2ScratchUses = (int)(sizeof(kQ2Scratch) / sizeof(kQ2Scratch[0]));

// nq transactions at read ids rq[0..nq): out[q * max_out + k], aborted[q]; commit only for nq == 1
struct Q2Call {
    stage_table *region, *nation, *supplier, *item, *stock;
    const uint32_t *map_off;
    const uint64_t *d_map_keys;
    int32_t target_region;
    const uint32_t *rq;
    uint32_t nq, commit_id;
    stage_q2_rec *out;
    uint64_t max_out, *n_out;
    int32_t *aborted;
    void *stream;
    int slot;
    bool async;
};

// the argument and state checks, in the order the CPU tests pin
static int q2_check(const Q2Call &c) {
    for (stage_table *t : {c.region, c.nation, c.supplier, c.item, c.stock})
        if (!t) return fail(STAGE_E_ARG, "null table");
    {
        const void *roles[] = {c.region, c.nation, c.supplier, c.item, c.stock};
        int rc = guarded([&] {
            check_scratch_uses(kQ2Scratch, kQ2ScratchUses, roles);
            return STAGE_OK;
        });
        if (rc) return rc;
    }
    for (stage_table *t : {c.region, c.nation, c.supplier, c.item, c.stock}) {
        int rc = need_synced(t);
        if (rc) return rc;
    }
    if (!c.map_off || !c.d_map_keys || (!c.async && (!c.n_out || !c.aborted)) || (c.max_out && !c.out))
        return fail(STAGE_E_ARG, "null argument");
    if (c.slot < 0 || c.slot > 1) return fail(STAGE_E_ARG, "slot must be 0 or 1");
    if (c.stock->q2p[c.slot].active)
        return fail(STAGE_E_STATE, "CH-Q2 slot still in flight: stage_ch_query2_wait first");
    if (c.target_region < 0 || c.target_region > 4) return fail(STAGE_E_ARG, "target_region must be 0..4");
    for (stage_table *t : {c.region, c.nation, c.supplier, c.item})
        if (facts(t).params().key_width != 8) return fail(STAGE_E_ARG, "REGION/NATION/SUPPLIER/ITEM keys are 8 bytes");
    if (facts(c.stock).params().key_width != 16) return fail(STAGE_E_ARG, "STOCK keys are {w, i}: 16 bytes");
    if (facts(c.region).params().payload_size < 55 || facts(c.nation).params().payload_size < 8 ||
        facts(c.supplier).params().payload_size < 8 || facts(c.item).params().payload_size < kIDataOff + 64 ||
        facts(c.stock).params().payload_size < 16)
        return fail(STAGE_E_ARG, "payloads too short for the Q2 columns");
    for (stage_table *t : {c.region, c.nation, c.supplier, c.item})
        if (t->dev.device != c.stock->dev.device) return fail(STAGE_E_ARG, "tables on different devices");
    return STAGE_OK;
}

// the call's sizes and the byte layouts of its staging and scratch
static void q2_plan(Q2Plan &p, const Q2Call &c) {
    const DevTable &pv = c.supplier->dev.view;
    p.nslots = (uint64_t)pv.nleaves * pv.cap;
    p.nchunks = p.nslots / 64;
    p.m_max = 0;
    for (uint32_t k = 0; k < kMapKeys; ++k)
        p.m_max += c.map_off[k + 1] > c.map_off[k] ? c.map_off[k + 1] - c.map_off[k] : 0;
    p.n_max = std::max<uint64_t>(p.nslots, 1);
    const uint64_t m1 = std::max<uint64_t>(p.m_max, 1), c1 = std::max<uint64_t>(p.nchunks, 1), *hint = c.stock->q2_hint;
    p.n_hint = hint[0] ? std::min(hint[0], p.n_max) : p.n_max;
    p.m_hint = hint[1] ? std::min(hint[1], m1) : p.m_max;
    // q2_place up to kPlaceChunks SUPPLIER chunks (STAGE_Q2_PLACE_CHUNKS: another limit, for
    // the tests of the three-kernel form larger tables take)
    const char *pe = std::getenv("STAGE_Q2_PLACE_CHUNKS");
    p.fused_place = p.nchunks <= (pe ? std::strtoull(pe, nullptr, 10) : kPlaceChunks);
    Carve q;
    p.q_map = q.take((kMapKeys + 1) * 4ull), p.q_rq = q.take(c.nq * 4ull);
    p.q_cn = q.off, q.off += 16;  // the 16 bytes of counts, the flags right behind them
    p.q_ab = q.take(c.nq * 4ull), p.q_zero = q.off, p.q_end = p.q_zero + 16;
    Carve o;
    p.o_mir = o.take(p.q_end), p.o_pairs = o.take(p.n_max * 16), p.o_sel = o.take(p.n_max * 8);
    p.o_src = o.take(p.n_max * 8), p.o_cnt = o.take(p.n_max * 4), p.o_dst = o.take(p.n_max * 8);
    p.o_keys = o.take(m1 * 16), p.o_sbase = o.take(m1 * 32), p.o_ik = o.take(p.n_max * 8 * c.nq);
    p.o_ibase = o.take(p.n_max * 32), p.o_rec = o.take(p.n_max * c.nq * sizeof(stage_q2_rec));
    p.o_vis = o.take(p.n_max), p.o_rank = o.take(p.n_max), p.o_koff = o.take(p.n_max * 4);
    p.o_ccnt = o.take(c1 * kVisits * 4), p.o_kcnt = o.take(c1 * kVisits * 4), p.o_nv = o.take(4);
    p.scratch = o.off;
    // NATION's scan (scan_sz 65) is past the compact scan kernel's 63 records; a table of fewer
    // slots than that returns the same records for every scan size of at least its slot count
    // (the scan ends at the table's end), so such a table is scanned with that size instead
    p.nat_scan = kNationScan;
    if (c.nation->dev.view.nleaves <= 4) {
        uint64_t slots = 0;
        for (const auto &L : host(c.nation).leaves_)
            if (L.live) slots += L.count;
        if (slots < (uint64_t)kNationScan) p.nat_scan = (uint32_t)std::max<uint64_t>(slots, 1);
    }
    p.reg_rows = 64 + (uint64_t)kRegionScan * c.region->dev.view.stride;
    p.nat_rows = 64 + (uint64_t)kNationScan * c.nation->dev.view.stride;
}

// the slot's pinned staging, filled
static void q2_stage(Q2Plan &p, const Q2Call &c) {
    p.pq = pinned_bytes(c.stock->dev, p.q_end, kQ2Pinned + c.slot);
    std::memcpy(p.pq + p.q_map, c.map_off, (kMapKeys + 1) * 4ull);
    std::memcpy(p.pq + p.q_rq, c.rq, c.nq * 4ull);
    std::memset(p.pq + p.q_cn, 0, 16 + c.nq * 4ull);
    std::memset(p.pq + p.q_zero, 0, 16);
}

// the device buffers: the batch buffers in SUPPLIER's scratch, the scan rows in REGION's and
// NATION's -- all sized here, before any capture
static void q2_bind(Q2Plan &p, const Q2Call &c) {
    // a batch still in flight uses these scratch buffers: growing one (a reallocation) waits
    // for it first
    if ((c.stock->q2p[0].active || c.stock->q2p[1].active) &&
        (c.supplier->dev.scratch.cap < p.scratch || c.region->dev.scratch.cap < p.reg_rows ||
         c.nation->dev.scratch.cap < p.nat_rows))
        hip_check(hipDeviceSynchronize(), "q2 drain");
    uint8_t *buf = p.buf = scratch_bytes(c.supplier->dev, p.scratch), *mir = p.mir = buf + p.o_mir;
    p.d_map = (const uint32_t *)(mir + p.q_map), p.d_rq = (const uint32_t *)(mir + p.q_rq);
    p.d_counts = (uint64_t *)(mir + p.q_cn), p.d_ab = (int32_t *)(mir + p.q_ab);
    p.d_zero = (const uint64_t *)(mir + p.q_zero);
    p.g_key = (uint64_t *)(buf + p.o_pairs), p.d_sel = (uint64_t *)(buf + p.o_sel);
    p.d_src = (uint64_t *)(buf + p.o_src), p.d_cnt = (uint32_t *)(buf + p.o_cnt), p.d_dst = (uint64_t *)(buf + p.o_dst);
    p.d_keys = (uint64_t *)(buf + p.o_keys), p.d_sbase = (stage_probe_out_dev *)(buf + p.o_sbase);
    p.d_ik = (uint64_t *)(buf + p.o_ik), p.d_ibase = (stage_probe_out_dev *)(buf + p.o_ibase);
    p.d_rec = (stage_q2_rec *)(buf + p.o_rec);
    p.g_vis = (int8_t *)(buf + p.o_vis), p.g_rank = buf + p.o_rank, p.g_koff = (uint32_t *)(buf + p.o_koff);
    p.ccnt = (uint32_t *)(buf + p.o_ccnt), p.kcnt = (uint32_t *)(buf + p.o_kcnt), p.g_nv = (uint32_t *)(buf + p.o_nv);
    p.regs = scratch_bytes(c.region->dev, p.reg_rows) + 64;
    p.nats = scratch_bytes(c.nation->dev, p.nat_rows) + 64;
}

// `out` in page-locked memory (stage_host_alloc, stage.pinned_empty) has a device view: the
// finishing kernel writes the records into it directly.  Pageable memory has none (null): the
// records are copied once the count is known.
static stage_q2_rec *q2_device_view(stage_q2_rec *out, uint64_t max_out) {
    void *dp = nullptr;
    if (!out || !max_out) return nullptr;
    if (hipHostGetDevicePointer(&dp, out, 0) != hipSuccess) dp = nullptr;
    (void)hipGetLastError();  // a pageable pointer is not an error here
    return (stage_q2_rec *)dp;
}

// an async batch's records leave from the side stream (Q2Pending::split): finished into the
// slot's own device buffer of `need` bytes, row pitch n_max
static stage_q2_rec *q2_slot_buffer(stage_table *stock, Q2Pending &P, uint64_t need) {
    if (P.dcap < need) {  // the slot is idle (q2_check): its old buffer is unused
        if (P.dbuf) hip_check(hipFree(P.dbuf), "q2 slot buffer");
        P.dbuf = nullptr;
        P.dcap = 0;
        hip_check(hipMalloc(&P.dbuf, need), "q2 slot buffer");
        P.dcap = need;
    }
    if (!stock->q2_side) hip_check(hipStreamCreateWithFlags(&stock->q2_side, hipStreamNonBlocking), "q2 side stream");
    if (!P.fin) hip_check(hipEventCreateWithFlags(&P.fin, hipEventDisableTiming), "q2 event");
    return (stage_q2_rec *)P.dbuf;
}

// the launch arguments beyond the plan
static void q2_arguments(Q2Launch &L, const Q2Call &c, stage_q2_rec *host_out, stage_q2_rec *slot_out, hipStream_t s) {
    L.rv = c.region->dev.view, L.nv = c.nation->dev.view, L.pv = c.supplier->dev.view;
    L.iv = c.item->dev.view, L.sv = c.stock->dev.view;
    L.stock_tune = c.stock->tune, L.item_tune = c.item->tune;
    L.region_scan = c.region->scan_tune, L.nation_scan = c.nation->scan_tune;
    L.supplier_kpad = facts(c.supplier).key_pad(), L.item_kpad = facts(c.item).key_pad();
    L.stock_kpad = facts(c.stock).key_pad();
    L.d_map_keys = c.d_map_keys;
    char tname[16] = {0};
    std::strncpy(tname, kRegions[c.target_region], 15);
    std::memcpy(&L.name0, tname, 8);
    std::memcpy(&L.name1, tname + 8, 8);
    for (size_t b = 0; b <= std::strlen(tname); ++b)  // the name and its NUL
        (b < 8 ? L.mask0 : L.mask1) |= 0xFFull << (8 * (b % 8));
    L.nq = c.nq, L.max_out = c.max_out, L.host_out = host_out, L.slot_out = slot_out;
    L.split = slot_out != nullptr;
    L.s = s;
}

// what must be over before the batch starts on s
static void q2_order(const Q2Call &c, hipStream_t s) {
    // work a caller left on the REGION / NATION tables' own streams (a call without a stream
    // runs there) is finished first: the whole batch then goes on s.  (Round 5 forked the two
    // scans onto those streams and joined them back: the cross-stream waits cost ~20 µs of
    // the ~35 µs the scans took, against ~10 µs for the two scans back to back on s.)
    for (stage_table *d : {c.region, c.nation})
        if (d->dev.stream && d->dev.stream != s) hip_check(hipStreamSynchronize(d->dev.stream), "dimension stream");
    // both slots share the SUPPLIER scratch and the REGION / NATION scan rows: a batch still in
    // flight on another stream is waited for on the device before this one is enqueued (on its
    // own stream, stream order already keeps them apart)
    for (const Q2Pending &o : c.stock->q2p)  // (a split batch's kernels: its copy reads only its slot buffer)
        if (o.active && o.stream != s) hip_check(hipStreamWaitEvent(s, o.split ? o.fin : o.ev, 0), "q2 other slot");
}

// where the enqueued batch's results will be (q2_collect); an async batch's events and, when
// split, its records' copy on the side stream
static void q2_park(const Q2Call &c, const Q2Launch &L, Q2Pending &P) {
    const Q2Plan &p = L.p;
    P.pq = p.pq, P.q_cn = p.q_cn, P.q_ab = p.q_ab, P.nq = c.nq, P.n_max = p.n_max, P.m_max = p.m_max;
    P.stream = L.s, P.split = L.split, P.out = c.out, P.max_out = c.max_out, P.slot_out = L.slot_out, P.cols = 0;
    if (!c.async) return;
    if (!P.ev) hip_check(hipEventCreateWithFlags(&P.ev, hipEventDisableTiming), "q2 event");
    if (P.split) {  // the records cross PCIe from the side stream while s goes on
        hip_check(hipEventRecord(P.fin, L.s), "q2 event");
        hip_check(hipStreamWaitEvent(c.stock->q2_side, P.fin, 0), "q2 side wait");
        // a 2-D copy (the DMA engine) of the expected count's columns -- the last call's
        // count; q2_collect copies any more.  (A kernel writing the records over PCIe from the
        // side stream slowed the next batch's kernels beside it ~4x, 0.153 ms a batch
        // against 0.127 with the copy, r06q2emit.)
        P.cols = std::min(p.n_hint, c.max_out);
        if (P.cols)
            hip_check(hipMemcpy2DAsync(c.out, c.max_out * sizeof(stage_q2_rec), L.slot_out,
                                       p.n_max * sizeof(stage_q2_rec), P.cols * sizeof(stage_q2_rec), c.nq,
                                       hipMemcpyDeviceToHost, c.stock->q2_side),
                      "q2 records copy");
        hip_check(hipEventRecord(P.ev, c.stock->q2_side), "q2 event");
    } else {
        hip_check(hipEventRecord(P.ev, L.s), "q2 event");
    }
    P.active = true;
}

// A finished batch's results (after the stream or event synchronisation): the counts and aborted
// flags out of its staging, the rest of a split emit; returns the number of visited suppliers
static uint64_t q2_collect(stage_table *stock, const Q2Pending &P, uint64_t *n_out, int32_t *aborted) {
    uint64_t cn[2];
    std::memcpy(cn, P.pq + P.q_cn, 16);
    std::memcpy(aborted, P.pq + P.q_ab, 4ull * P.nq);
    if (cn[0] > P.n_max || cn[1] > P.m_max) throw std::runtime_error("q2: device counts out of range");
    const uint64_t want = std::min<uint64_t>(cn[0], P.max_out);
    if (P.split && want > P.cols)  // more records than the copy expected
        hip_check(hipMemcpy2D(P.out + P.cols, P.max_out * sizeof(stage_q2_rec), P.slot_out + P.cols,
                              P.n_max * sizeof(stage_q2_rec), (want - P.cols) * sizeof(stage_q2_rec), P.nq,
                              hipMemcpyDeviceToHost),
                  "q2 records rest");
    stock->q2_hint[0] = cn[0];
    stock->q2_hint[1] = cn[1];
    *n_out = cn[0];
    if (cn[0] == 0)
        for (uint32_t q = 0; q < P.nq; ++q) aborted[q] = 0;
    return cn[0];
}

// 5. the transaction's stock updates (the marked ones of recs[0..n)), through the device write
// path; each one's code into its record
static int q2_apply_updates(const Q2Call &c, hipStream_t s, stage_q2_rec *recs, uint64_t n) {
    std::vector<uint64_t> uk;
    std::vector<int32_t> ud;
    std::vector<uint32_t> ui;
    for (uint32_t k = 0; k < n; ++k)
        if (recs[k].update) {
            uk.push_back((uint64_t)recs[k].s_w_id);
            uk.push_back((uint64_t)recs[k].s_i_id);
            ud.insert(ud.end(), {recs[k].s_quantity + 50, recs[k].s_ytd, recs[k].s_order_cnt, recs[k].s_remote_cnt});
            ui.push_back(k);
        }
    const uint64_t nu = ui.size();
    if (!nu) return STAGE_OK;
    Carve u;
    const uint64_t u_k = u.take(nu * 16), u_d = u.take(nu * 16), u_w = u.take(nu * 4), u_c = u.take(nu * 4),
                   u_rc = u.take(nu);
    uint8_t *ub = scratch_bytes(c.item->dev, u.off);
    std::vector<uint32_t> wid(nu, c.rq[0]), cid(nu, c.commit_id);
    hip_check(hipMemcpyAsync(ub + u_k, uk.data(), nu * 16, hipMemcpyHostToDevice, s), "h2d");
    hip_check(hipMemcpyAsync(ub + u_d, ud.data(), nu * 16, hipMemcpyHostToDevice, s), "h2d");
    hip_check(hipMemcpyAsync(ub + u_w, wid.data(), nu * 4, hipMemcpyHostToDevice, s), "h2d");
    hip_check(hipMemcpyAsync(ub + u_c, cid.data(), nu * 4, hipMemcpyHostToDevice, s), "h2d");
    uint64_t ok = 0;
    const int rc = stage_update_batch_device(c.stock, (const uint64_t *)(ub + u_k), nullptr, nu, 0, ub + u_d, 16,
                                             (const uint32_t *)(ub + u_w), (const uint32_t *)(ub + u_c), nullptr,
                                             ub + u_rc, &ok, s);
    if (rc) return rc;
    std::vector<uint8_t> rcs(nu);
    hip_check(hipMemcpyAsync(rcs.data(), ub + u_rc, nu, hipMemcpyDeviceToHost, s), "d2h");
    hip_check(hipStreamSynchronize(s), "update sync");
    for (uint64_t j = 0; j < nu; ++j) recs[ui[j]].update_rc = rcs[j];
    return STAGE_OK;
}

static int q2_run(const Q2Call &c) {
    if (int rc = q2_check(c)) return rc;
    return guarded([&] {
        hip_check(hipSetDevice(c.stock->dev.device), "hipSetDevice");
        hipStream_t s = pick(c.stock, c.stream);
        const Q2Trace trace;
        if (!c.async) {
            *c.n_out = 0;
            for (uint32_t q = 0; q < c.nq; ++q) c.aborted[q] = 0;
        }
        if (c.supplier->dev.view.cap % 64) return fail(STAGE_E_UNSUPPORTED, "SUPPLIER leaves of a multiple of 64 slots");
        Q2Launch L;  // zeroed, its padding too: its bytes are the graph's key
        std::memset((void *)&L, 0, sizeof L);
        Q2Plan &p = L.p;
        q2_plan(p, c);
        q2_stage(p, c);
        trace.lap("staged");
        q2_bind(p, c);
        stage_q2_rec *host_out = q2_device_view(c.out, c.max_out);
        if (Q2Trace::on())
            std::fprintf(stderr, "[q2] out %s\n", host_out ? "page-locked: written by q2_finish" : "pageable: copied");
        if (c.async && c.out && c.max_out && !host_out)
            return fail(STAGE_E_ARG, "stage_ch_query2_batch_async needs a page-locked out (stage_host_alloc)");
        Q2Pending &P = c.stock->q2p[c.slot];
        stage_q2_rec *slot_out =
            c.async && host_out ? q2_slot_buffer(c.stock, P, p.n_max * c.nq * sizeof(stage_q2_rec)) : nullptr;
        trace.lap("buffers");
        q2_order(c, s);
        q2_arguments(L, c, host_out, slot_out, s);
        const std::string key = q2_key(L, {c.region, c.nation, c.supplier, c.item, c.stock});
        trace.lap("key");
        const char *how = replay_or_enqueue(c.stock->q2g[c.slot], key, s, [&L] { q2_enqueue(L); });
        if (Q2Trace::on()) std::fprintf(stderr, "[q2] batch %s\n", how);
        trace.lap("enqueued");
        q2_park(c, L, P);
        if (c.async) return STAGE_OK;  // the results are read by stage_ch_query2_wait
        hip_check(hipStreamSynchronize(s), "q2 sync");  // the batch's one synchronisation
        trace.lap("results back");
        const uint64_t n = q2_collect(c.stock, P, c.n_out, c.aborted);
        if (n == 0) return STAGE_OK;
        std::vector<stage_q2_rec> recs_buf;
        if (!host_out) {  // a pageable (or no) `out`: the records come back now
            recs_buf.resize(n * c.nq);
            hip_check(hipMemcpy(recs_buf.data(), p.d_rec, n * c.nq * sizeof(stage_q2_rec), hipMemcpyDeviceToHost), "d2h");
        }
        if (c.nq == 1 && c.commit_id && !*c.aborted) {
            const int rc = host_out ? q2_apply_updates(c, s, c.out, std::min(n, c.max_out))
                                    : q2_apply_updates(c, s, recs_buf.data(), n);
            if (rc) return rc;
        }
        if (!host_out && c.out)
            for (uint32_t q = 0; q < c.nq; ++q)
                std::memcpy(c.out + (uint64_t)q * c.max_out, recs_buf.data() + (uint64_t)q * n,
                            std::min<uint64_t>(n, c.max_out) * sizeof(stage_q2_rec));
        trace.lap("out copied");
        return STAGE_OK;
    });
}

extern "C" int stage_ch_query2(stage_table *region, stage_table *nation, stage_table *supplier, stage_table *item,
                               stage_table *stock, const uint32_t *map_off, const uint64_t *d_map_keys,
                               int32_t target_region, uint32_t read_id, uint32_t commit_id, stage_q2_rec *out,
                               uint64_t max_out, uint64_t *n_out, int32_t *aborted, void *stream) {
    return q2_run({region, nation, supplier, item, stock, map_off, d_map_keys, target_region, &read_id, 1, commit_id,
                   out, max_out, n_out, aborted, stream, 0, false});
}

extern "C" int stage_ch_query2_batch_async(stage_table *region, stage_table *nation, stage_table *supplier,
                                           stage_table *item, stage_table *stock, const uint32_t *map_off,
                                           const uint64_t *d_map_keys, int32_t target_region, const uint32_t *read_ids,
                                           uint32_t nq, stage_q2_rec *out, uint64_t max_per_query, int slot,
                                           void *stream) {
    if (nq == 0 || !read_ids || nq > 4096) return fail(STAGE_E_ARG, "read_ids: 1..4096 queries");
    if (!out || !max_per_query) return fail(STAGE_E_ARG, "an out array is required");
    return q2_run({region, nation, supplier, item, stock, map_off, d_map_keys, target_region, read_ids, nq, 0, out,
                   max_per_query, nullptr, nullptr, stream, slot, true});
}

extern "C" int stage_ch_query2_wait(stage_table *stock, int slot, uint64_t *n_out, int32_t *aborted) {
    if (!stock || slot < 0 || slot > 1 || !n_out || !aborted) return fail(STAGE_E_ARG, "bad arguments");
    Q2Pending &P = stock->q2p[slot];
    if (!P.active) return fail(STAGE_E_STATE, "no CH-Q2 batch in flight in this slot");
    return guarded([&] {
        // the slot stays busy until its event and its records' rest have come back: while either
        // fails, a copy out of its buffer may still be queued (~stage_table waits for a busy slot)
        hip_check(hipEventSynchronize(P.ev), "q2 wait");
        q2_collect(stock, P, n_out, aborted);
        P.active = false;
        return STAGE_OK;
    });
}

extern "C" int stage_ch_query2_batch(stage_table *region, stage_table *nation, stage_table *supplier,
                                     stage_table *item, stage_table *stock, const uint32_t *map_off,
                                     const uint64_t *d_map_keys, int32_t target_region, const uint32_t *read_ids,
                                     uint32_t nq, stage_q2_rec *out, uint64_t max_per_query, uint64_t *n_out,
                                     int32_t *aborted, void *stream) {
    if (nq == 0) return STAGE_OK;
    if (!read_ids || nq > 4096) return fail(STAGE_E_ARG, "read_ids: 1..4096 queries");
    return q2_run({region, nation, supplier, item, stock, map_off, d_map_keys, target_region, read_ids, nq, 0, out,
                   max_per_query, n_out, aborted, stream, 0, false});
}

// the multi-table operations' scratch plans (stage_hip.h)
static const stage::ScratchUse kStockLevelScratch[] = {{0, "the stock-level batch buffers (DISTRICT)"}};

extern "C" int stage_scratch_plan_check(int op, const int32_t *roles, int n) {
    const stage::ScratchUse *plan;
    int np;
    if (op == 0) plan = kQ2Scratch, np = kQ2ScratchUses;
    else if (op == 1) plan = kStockLevelScratch, np = 1;
    else return fail(STAGE_E_ARG, "op: 0 = CH-Q2, 1 = stock-level");
    if (roles && n != np) return fail(STAGE_E_ARG, "roles: one per scratch user of the plan");
    return guarded([&] {
        std::vector<stage::ScratchUse> u(plan, plan + np);
        if (roles)
            for (int i = 0; i < np; ++i) u[i].role = roles[i];
        stage::check_scratch_uses(u.data(), np);
        return STAGE_OK;
    });
}
