// scan.hip -- gfx950 (CDNA4, wave64) range-scan kernels of the index-organized read path: the
// row scans, the column-window scans, the first-tuple scans and their launchers.  Mapping:
//   * range scan: ballot + mbcnt prefix counts give RangeScanBySize's slot-order truncation
//     (b_tree.cpp:1276-1302), an in-wave rank sort replaces std::sort, continuation as
//     Iterator::GetNext (b_tree.h:899-941).
// scan_one and scan_one_compact are plain __device__ templates: callers stay here.
#include "kernel_api.hpp"
#include "launch_util.hpp"
#include "row_store.hpp"
#include "tree_search.hpp"

namespace stage {

// ----------------------------------------------------------------------------------------
// range scan (TableScanExecutor over Iterator), one wave per scan

// one scan's start: its key length, order-key words and start leaf (wave-uniform)
template <bool VARLEN, int KW>
__device__ __forceinline__ uint32_t scan_start(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t i,
                                               uint32_t lane, uint64_t *ok, uint32_t &len) {
    len = t.key_width ? t.key_width : (lens ? (uint32_t)lens[i] : 8u);
    load_okey<KW>(keys, i, true, len, ok);
    return uni32(resolve_leaf_uniform<VARLEN, KW>(t, ok, len, true, lane));
}

// the heap row of a kept slot; for VIS the row reader rid sees, its status to row_status[pos].
// The window forms' snippet: scan_one's row branch and RowSink spell the same lines out, since
// calling this there (or one helper for their whole row emission) moved the code of the measured
// scan_kernel instances.
template <bool VIS>
__device__ __forceinline__ uint32_t kept_row(const DevTable &t, const SlotInfo &si, uint32_t rid, uint8_t *row_status,
                                             uint32_t pos) {
    if (!VIS) return si.image;
    uint8_t st;
    const uint32_t img = scan_visible(t, si, rid, st);
    row_status[pos] = st;
    return img;
}

// What a leaf visit does with its e smallest kept records is scan_one's trailing policy: NoWindow
// copies their rows to recs; ScanWindow (the column-window scan, below) writes their heap rows by
// rank into the wave's LDS list rk (SPL * 64 words) and hands it to store_scan_windows.  A
// compile-time policy passed by value: the row instances compile as they did without it.
struct NoWindow {
    static constexpr bool on = false;
};
struct ScanWindow {
    static constexpr bool on = true;
    uint64_t pos0;  // first output position of the scan: i * scan_size
    uint32_t *rk;
    const ScanWindowArgs *a;
};

template <bool VARLEN, int SPL, int R, int KW, bool VIS = false, class Win = NoWindow>
__device__ void scan_one(const DevTable &t, const uint64_t *x0, uint32_t xl, uint32_t leaf, uint32_t scan_size,
                         uint8_t *recs, uint32_t *count_out, uint32_t lane, uint32_t rid = 0,
                         uint8_t *row_status = nullptr, Win win = {}) {
    uint32_t remaining = scan_size, produced = 0;
    bool cont = false;
    uint64_t x[KW];
#pragma unroll
    for (int w = 0; w < KW; ++w) x[w] = x0[w];
    for (uint32_t guard = 0; guard < scan_size + 2 && remaining > 0; ++guard) {
        const uint64_t base = (uint64_t)leaf * t.cap;
        // the leaf's monotone slot prefix (info word), loaded beside the key columns
        const uint32_t mp =
            *reinterpret_cast<const uint32_t *>(t.head + (uint64_t)leaf * t.head_bytes + head_info_offset(t.cap, KW)) >> 16;
        uint64_t col[SPL][KW];
        uint32_t kl[SPL];
        uint64_t q[SPL];
#pragma unroll
        for (int s = 0; s < SPL; ++s)
#pragma unroll
            for (int w = 0; w < KW; ++w) col[s][w] = t.okey[((uint64_t)leaf * KW + w) * t.cap + s * 64 + lane];
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
            const uint64_t vm = head_vis(t, leaf, s);
            const bool vis = (vm >> lane) & 1;
            kl[s] = t.key_width;
            if (VARLEN) kl[s] = vis ? meta_keylen(t.slot[base + s * 64 + lane].meta) : 0u;
            // RangeScanBySize keeps visible records with KeyCompare(start, key) <= 0
            q[s] = ballot(vis && !key_less<VARLEN, KW>(col[s], kl[s], x, xl));
        }
        // slot-order truncation: records are collected until more than to_scan are held
        const uint32_t to_scan = remaining;
        uint32_t before = 0, m = 0;
        bool keep[SPL];
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
            const uint32_t rank = before + count_below(q[s]);
            keep[s] = ((q[s] >> lane) & 1) && rank <= to_scan;
            before += (uint32_t)__builtin_popcountll(q[s]);
        }
        uint64_t km[SPL];
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
            km[s] = ballot(keep[s]);
            m += (uint32_t)__builtin_popcountll(km[s]);
        }
        if (m == 0) break;
        // key rank among the kept records (std::sort by KeyCompare; keys are unique).  When
        // every kept record lies in the leaf's monotone slot prefix [0, mp) (info word), keys
        // increase with the slot, so a record's rank is its slot-order position: no compare loop
        uint32_t kr[SPL];
        uint32_t top = 0;  // one past the highest kept slot
#pragma unroll
        for (int s = 0; s < SPL; ++s)
            if (km[s]) top = (uint32_t)s * 64u + 64u - (uint32_t)__builtin_clzll(km[s]);
        const bool mono = top <= mp;
        {
            uint32_t pre = 0;
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                kr[s] = mono ? pre + count_below(km[s]) : 0u;
                pre += (uint32_t)__builtin_popcountll(km[s]);
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < SPL; ++s2) {
            uint64_t mm = mono ? 0ull : km[s2];
            while (mm) {
                const int b = __builtin_ctzll(mm);
                mm &= mm - 1;
                uint64_t ko[KW];
#pragma unroll
                for (int w = 0; w < KW; ++w) ko[w] = rl64(col[s2][w], b);
                const uint32_t kll = rl32(kl[s2], b);
#pragma unroll
                for (int s = 0; s < SPL; ++s) kr[s] += key_less<VARLEN, KW>(ko, kll, col[s], kl[s]) ? 1u : 0u;
            }
        }
        // continuation: if the new batch starts with the last key, the iterator stops
        if (cont) {
            bool dup = false;
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                bool eq = kl[s] == xl;
#pragma unroll
                for (int w = 0; w < KW; ++w) eq = eq && col[s][w] == x[w];
                dup |= keep[s] && kr[s] == 0 && eq;
            }
            if (ballot(dup)) break;
        }
        const uint32_t e = m < remaining ? m : remaining;
        if constexpr (Win::on) {
            // the e smallest kept records: heap rows into the list by rank (kr < e <= SPL * 64)
#pragma unroll
            for (int s = 0; s < SPL; ++s)
                if (keep[s] && kr[s] < e)
                    win.rk[kr[s]] = kept_row<VIS>(t, t.slot[base + s * 64 + lane], rid, row_status, produced + kr[s]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            store_scan_windows(t, lane, win.pos0 + produced, e, win.rk, *win.a);
            __builtin_amdgcn_wave_barrier();  // the list is rewritten on the next leaf
        } else {
            // emit the e smallest kept records at produced + rank, R rows in flight
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                const bool emit = keep[s] && kr[s] < e;
                uint32_t img = 0;
                if (emit) {
                    if (VIS) {
                        uint8_t st;
                        img = scan_visible(t, t.slot[base + s * 64 + lane], rid, st);
                        row_status[produced + kr[s]] = st;
                    } else {
                        img = t.slot[base + s * 64 + lane].image;
                    }
                }
                uint64_t em = ballot(emit);
                if (em && t.stride <= 512) {  // small rows: several per load instruction
                    copy_rows_flat<4>(t, em, img, produced + kr[s], recs, lane);
                    em = 0;
                }
                while (em) {
                    uint32_t imr[R], dr[R];
                    int nk = 0;
                    for (; nk < R && em; ++nk) {
                        const int b = __builtin_ctzll(em);
                        em &= em - 1;
                        imr[nk] = rl32(img, b);
                        dr[nk] = produced + rl32(kr[s], b);
                    }
                    copy_rows<R>(t, imr, dr, nk, recs, lane);
                }
            }
        }
        produced += e;
        remaining -= e;
        if (e < m) break;
        // last record popped: continue from its key with le_child = false (next_leaf_after)
        uint32_t lastl = 0;
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
            const uint64_t lm = ballot(keep[s] && kr[s] == m - 1);
            if (lm) {
                const int b = __builtin_ctzll(lm);
#pragma unroll
                for (int w = 0; w < KW; ++w) x[w] = rl64(col[s][w], b);
                lastl = rl32(kl[s], b);
            }
        }
        xl = lastl;
        leaf = uni32(next_leaf_after<VARLEN, KW>(t, leaf, x, xl));
        cont = true;
    }
    if (lane == 0) *count_out = produced;
}

// Range scan for leaves of many slot groups (wide-key tables, up to 1024 slots) and scans of
// at most 63 records: RangeScanBySize's collection (first to_scan+1 qualifying records in slot
// order) walks only the slot groups whose max key (leaf head) reaches the start key and stops
// as soon as to_scan+1 records are held; the kept records (<= 64) go to a per-wave LDS list,
// one lane per record ranks them (std::sort) and they are handed to the sink in key order.
//
// Sinks: emit() sees, per lane, whether the lane emits a record on this leaf visit (`on`), its
// slot, its rank `kr` among this visit's records (`produced` records came before) and its key
// words; it returns true to end the scan early.
template <bool VIS>
struct RowSink {  // rows (and, for VIS, per-record statuses) as scan_one writes them
    uint8_t *recs;
    uint8_t *row_status;
    uint32_t rid;
    template <int KW>
    __device__ __forceinline__ bool emit(const DevTable &t, uint64_t base, bool on, uint32_t mslot, uint32_t kr,
                                         uint32_t produced, const uint64_t *, uint32_t lane) {
        uint32_t img = 0;
        if (on) {
            if (VIS) {
                uint8_t st;
                img = scan_visible(t, t.slot[base + mslot], rid, st);
                row_status[produced + kr] = st;
            } else {
                img = t.slot[base + mslot].image;
            }
        }
        uint64_t em = ballot(on);
        if (em && t.stride <= 512) {  // small rows: several per load instruction
            copy_rows_flat<4>(t, em, img, produced + kr, recs, lane);
            em = 0;
        }
        while (em) {
            uint32_t imr[4], dr[4];
            int nk = 0;
            for (; nk < 4 && em; ++nk) {
                const int b = __builtin_ctzll(em);
                em &= em - 1;
                imr[nk] = rl32(img, b);
                dr[nk] = produced + rl32(kr, b);
            }
            copy_rows<4>(t, imr, dr, nk, recs, lane);
        }
        return false;
    }
};

// IndexScanExecutor range branch consumed up to its first produced tuple (LATEST or OLD) whose
// key begins with the start key's first `words` order words -- a predicate over the scan that
// keeps only that tuple (TPC-C stock-level, tpcc_stock_level.cpp:104-135, takes ol_i_ids[0]).
// Result (wave-uniform): the tuple's heap row and status, or 0xFFFFFFFF / NOT_FOUND.
template <int KW>
struct FirstPrefixSink {
    uint64_t pre[KW];
    uint32_t words;
    uint32_t rid;
    uint32_t img;
    uint32_t st;
    template <int KW2>
    __device__ __forceinline__ bool emit(const DevTable &t, uint64_t base, bool on, uint32_t mslot, uint32_t kr,
                                         uint32_t, const uint64_t *mk, uint32_t) {
        uint8_t s = ST_NOT_FOUND;
        uint32_t im = 0xFFFFFFFFu;
        bool pass = false;
        if (on) {
            im = scan_visible(t, t.slot[base + mslot], rid, s);
            pass = s == ST_LATEST || s == ST_OLD;
#pragma unroll
            for (int w = 0; w < KW; ++w)
                if ((uint32_t)w < words) pass = pass && mk[w] == pre[w];
        }
        uint64_t pm = ballot(pass);
        if (!pm) return false;
        uint32_t best = 0xFFFFFFFFu;
        int bl = 0;
        while (pm) {  // the passing record of lowest rank
            const int b = __builtin_ctzll(pm);
            pm &= pm - 1;
            const uint32_t k = rl32(kr, b);
            if (k < best) {
                best = k;
                bl = b;
            }
        }
        img = rl32(im, bl);
        st = rl32((uint32_t)s, bl);
        return true;
    }
};

template <bool VARLEN, int SPL, int KW, class Sink>
__device__ uint32_t scan_one_compact(const DevTable &t, const uint64_t *x0, uint32_t xl, uint32_t leaf,
                                     uint32_t scan_size, uint32_t lane, Sink &sink, uint64_t *lk, uint32_t *ll,
                                     uint32_t *ls) {
    uint32_t remaining = scan_size, produced = 0;
    bool cont = false;
    uint64_t x[KW];
#pragma unroll
    for (int w = 0; w < KW; ++w) x[w] = x0[w];
    for (uint32_t guard = 0; guard < scan_size + 2 && remaining > 0; ++guard) {
        const uint64_t base = (uint64_t)leaf * t.cap;
        const uint8_t *hd = t.head + (uint64_t)leaf * t.head_bytes;
        const uint32_t mp = *reinterpret_cast<const uint32_t *>(hd + head_info_offset(t.cap, KW)) >> 16;  // info word
        // slot groups that can hold a key >= x (lane g tests group g's max key)
        bool act = false;
        if (lane < (uint32_t)SPL) {
            const uint64_t *gm = reinterpret_cast<const uint64_t *>(hd + head_gmax_offset(t.cap)) + lane * KW;
            uint64_t g[KW];
#pragma unroll
            for (int w = 0; w < KW; ++w) g[w] = gm[w];
            act = !kw_lt<KW>(g, x);
        }
        uint64_t active = ballot(act);
        const uint32_t to_scan = remaining;
        uint32_t kept = 0;
        while (active) {
            const int s = __builtin_ctzll(active);
            active &= active - 1;
            const uint64_t vm = head_vis(t, leaf, s);
            if (!vm) continue;
            const bool vis = (vm >> lane) & 1;
            uint64_t col[KW];
#pragma unroll
            for (int w = 0; w < KW; ++w) col[w] = t.okey[((uint64_t)leaf * KW + w) * t.cap + s * 64 + lane];
            uint32_t kl = t.key_width;
            if (VARLEN) kl = vis ? meta_keylen(t.slot[base + s * 64 + lane].meta) : 0u;
            const uint64_t q = ballot(vis && !key_less<VARLEN, KW>(col, kl, x, xl));
            if (!q) continue;
            const uint32_t rank = kept + count_below(q);
            const bool take = ((q >> lane) & 1) && rank <= to_scan;
            if (take) {
#pragma unroll
                for (int w = 0; w < KW; ++w) lk[rank * KW + w] = col[w];
                ll[rank] = kl;
                ls[rank] = (uint32_t)(s * 64) + lane;
            }
            kept += (uint32_t)__builtin_popcountll(ballot(take));
            if (kept > to_scan) break;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t m = kept;
        if (m == 0) break;
        // lane k < m holds kept record k; its rank among the kept records = position after sort
        const bool mine = lane < m;
        uint64_t mk[KW];
        uint32_t ml = 0, mslot = 0;
#pragma unroll
        for (int w = 0; w < KW; ++w) mk[w] = mine ? lk[lane * KW + w] : 0ull;
        if (mine) {
            ml = ll[lane];
            mslot = ls[lane];
        }
        // the list is in slot order; when its last (highest) slot lies in the leaf's monotone slot
        // prefix [0, mp) (info word), keys increase with the slot and the list order is the rank
        const bool mono = ls[m - 1] < mp;
        uint32_t kr = mono ? lane : 0u;
        for (uint32_t j = 0; j < (mono ? 0u : m); ++j) {
            uint64_t kj[KW];
#pragma unroll
            for (int w = 0; w < KW; ++w) kj[w] = lk[j * KW + w];
            kr += (mine && key_less<VARLEN, KW>(kj, ll[j], mk, ml)) ? 1u : 0u;
        }
        __builtin_amdgcn_wave_barrier();  // the LDS list is rewritten on the next leaf
        if (cont) {
            bool eq = ml == xl;
#pragma unroll
            for (int w = 0; w < KW; ++w) eq = eq && mk[w] == x[w];
            if (ballot(mine && kr == 0 && eq)) break;
        }
        const uint32_t e = m < remaining ? m : remaining;
        if (sink.template emit<KW>(t, base, mine && kr < e, mslot, kr, produced, mk, lane)) {
            produced += e;
            break;
        }
        produced += e;
        remaining -= e;
        if (e < m) break;
        // last record popped: continue from its key with le_child = false (next_leaf_after)
        const uint64_t lm = ballot(mine && kr == m - 1);
        const int b = __builtin_ctzll(lm);
#pragma unroll
        for (int w = 0; w < KW; ++w) x[w] = rl64(mk[w], b);
        xl = rl32(ml, b);
        leaf = uni32(next_leaf_after<VARLEN, KW>(t, leaf, x, xl));
        cont = true;
    }
    return produced;
}

// one scan of scan_compact (a wave; the LDS buffers are the wave's)
template <bool VARLEN, int SPL, int KW, bool VIS>
__device__ __forceinline__ void scan_compact_one(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t i,
                                                 uint32_t scan_size, uint32_t *counts, uint8_t *recs,
                                                 const uint32_t *rids, uint8_t *row_status, uint32_t lane,
                                                 uint64_t *s_keys, uint32_t *s_len, uint32_t *s_slot) {
    uint32_t len;
    uint64_t ok[KW];
    const uint32_t leaf = scan_start<VARLEN, KW>(t, keys, lens, i, lane, ok, len);
    RowSink<VIS> sink{recs + i * (uint64_t)scan_size * t.stride, VIS ? row_status + i * (uint64_t)scan_size : nullptr,
                      VIS ? (rids ? rids[i] : 0xFFFFFFFEu) : 0u};
    const uint32_t produced =
        scan_one_compact<VARLEN, SPL, KW>(t, ok, len, leaf, scan_size, lane, sink, s_keys, s_len, s_slot);
    if (lane == 0) counts[i] = produced;
}

template <bool VARLEN, int SPL, int KW, bool VIS>
__global__ __launch_bounds__(256) void scan_kernel_compact(DevTable t, const uint64_t *__restrict__ keys,
                                                           const uint16_t *__restrict__ lens, uint64_t n,
                                                           uint32_t scan_size, uint32_t *__restrict__ counts,
                                                           uint8_t *__restrict__ recs,
                                                           const uint32_t *__restrict__ rids,
                                                           uint8_t *__restrict__ row_status) {
    __shared__ uint64_t s_keys[4][64 * KW];
    __shared__ uint32_t s_len[4][64], s_slot[4][64];
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t i = wave; i < n; i += nwaves)
        scan_compact_one<VARLEN, SPL, KW, VIS>(t, keys, lens, i, scan_size, counts, recs, rids, row_status, lane,
                                               s_keys[wv], s_len[wv], s_slot[wv]);
}

// two single scans of two tables (the same leaf size, 8-byte keys, at most 63 records each) in
// one launch: block 0 scans t0 from k0[0], block 1 t1 from k1[0] -- CH-Q2's REGION and NATION
// scans, whose latency chains then overlap instead of running back to back
template <int SPL>
__global__ __launch_bounds__(64) void scan_pair_compact_kernel(DevTable t0, DevTable t1, const uint64_t *__restrict__ k0,
                                                             const uint64_t *__restrict__ k1, uint32_t sz0, uint32_t sz1,
                                                             uint32_t *__restrict__ c0, uint32_t *__restrict__ c1,
                                                             uint8_t *__restrict__ r0, uint8_t *__restrict__ r1) {
    __shared__ uint64_t s_keys[64];
    __shared__ uint32_t s_len[64], s_slot[64];
    const uint32_t lane = lane_id();
    if (blockIdx.x == 0)
        scan_compact_one<false, SPL, 1, false>(t0, k0, nullptr, 0, sz0, c0, r0, nullptr, nullptr, lane, s_keys, s_len,
                                               s_slot);
    else
        scan_compact_one<false, SPL, 1, false>(t1, k1, nullptr, 0, sz1, c1, r1, nullptr, nullptr, lane, s_keys, s_len,
                                               s_slot);
}

// The IndexScanExecutor range scan of `scan_size` records from key i (a wave per scan, the
// start-leaf descents of kFirstChunk scans done lane-parallel first), kept
// only up to its first produced tuple with the start key's first `words` order words
// (FirstPrefixSink); img_out[i] / st_out[i] = that tuple's heap row and status.
constexpr int kFirstChunk = 16;
constexpr uint8_t kFirstUndecided = 0xFE;  // scan_first_split_kernel -> scan_first_rest_kernel

// Chunk-cooperative lower bound of kFirstChunk fixed-width start keys: lane L works for scan
// L/4 and compares a quarter of each node (4 of the 16 inner entries, 2 of the 8 bottom ones);
// two xor-shuffles sum the quarter counts.  Same result as tree_lower_bound (le_child = true),
// one round trip per level for all 16 scans, a quarter of the per-lane loads and compares.
template <int KW>
__device__ __forceinline__ uint32_t chunk_lower_bound(const DevTable &t, const uint64_t *x, uint32_t part) {
    static_assert(kTreeFanout == 16 && kLeafFanout == 8, "quarters sized for 16 / 8 entries");
    uint32_t node = 0;
    for (int lvl = (int)t.levels - 1; lvl >= 0; --lvl) {
        const bool inner = lvl > 0;
        const uint32_t f = inner ? (uint32_t)kTreeFanout : (uint32_t)kLeafFanout;
        const uint32_t per = f / 4;
        const uint64_t *e = t.tree + (t.level_off[lvl] + (uint64_t)node * f + part * per) * KW;
        uint64_t w0[KW], w1[KW], w2[KW], w3[KW];
#pragma unroll
        for (int j = 0; j < KW; ++j) {
            w0[j] = e[j];
            w1[j] = e[KW + j];
            w2[j] = inner ? e[2 * KW + j] : ~0ull;
            w3[j] = inner ? e[3 * KW + j] : ~0ull;
        }
        int c = (kw_lt<KW>(w0, x) ? 1 : 0) + (kw_lt<KW>(w1, x) ? 1 : 0);
        if (inner) c += (kw_lt<KW>(w2, x) ? 1 : 0) + (kw_lt<KW>(w3, x) ? 1 : 0);
        c += __shfl_xor(c, 1);
        c += __shfl_xor(c, 2);
        node = node * f + (uint32_t)c;
    }
    return node < t.nseps ? node : t.nseps;
}

// The first-tuple scans split in two stages per chunk of 16 (same results as scan_first_kernel):
//  A (wave per scan, in turn): the start leaf's first visit -- active groups (all 16 scans' in
//    one round trip), the first group prefetched while the previous scan runs, the kept records
//    ranked (slot order when increasing), and the first e = min(m, scan_size) of them in rank
//    order written to LDS as candidates: the slot of a record carrying the start key's prefix,
//    or a hole;
//  B (lane per scan, all 16 together): the candidates' slot words and visibility in rank order,
//    the first LATEST / OLD one is the result -- one round trip for the 16 scans instead of one
//    per scan;
//  a scan whose first visit decides nothing (no candidate passed, the visit held m <= e records
//    and the scan has records left) is re-run by the general loop (scan_one_compact +
//    FirstPrefixSink), which continues across leaves.
template <int SPL, int KW, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void scan_first_split_kernel(
    DevTable t, const uint64_t *__restrict__ keys, uint64_t n, uint32_t scan_size, const uint32_t *__restrict__ rids,
    uint32_t words, uint32_t *__restrict__ img_out, uint8_t *__restrict__ st_out) {
    __shared__ uint64_t s_keys[4][64 * KW];
    __shared__ uint32_t s_slot[4][64];
    __shared__ uint16_t s_cand[4][kFirstChunk][64];
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t len = t.key_width;
    uint64_t *lk = s_keys[wv];
    uint32_t *ls = s_slot[wv];
    constexpr uint16_t kHole = 0xFFFF;
    for (uint64_t c0 = wave * kFirstChunk; c0 < n; c0 += nwaves * kFirstChunk) {
        const uint64_t i = c0 + (lane >> 2);  // the scan this lane descends for
        const bool valid = i < n;
        uint64_t ok[KW];
        load_okey<KW>(keys, i, valid, len, ok);
        const uint32_t leafv = chunk_lower_bound<KW>(t, ok, lane & 3);
        const uint32_t ridv = valid && rids ? rids[i] : 0xFFFFFFFEu;
        const int cnt = (int)((n - c0) < (uint64_t)kFirstChunk ? (n - c0) : (uint64_t)kFirstChunk);
        // active slot groups of every start leaf (lane L tests groups L%4, L%4+4, ... of scan L/4)
        uint32_t actv = 0;
        {
            const uint64_t *gm = reinterpret_cast<const uint64_t *>(t.head + (uint64_t)leafv * t.head_bytes +
                                                                    head_gmax_offset(t.cap));
#pragma unroll
            for (int g = 0; g < SPL; g += 4) {
                const uint32_t gg = (uint32_t)g + (lane & 3);
                if (gg < (uint32_t)SPL) {
                    uint64_t e[KW];
#pragma unroll
                    for (int w = 0; w < KW; ++w) e[w] = gm[gg * KW + w];
                    actv |= kw_lt<KW>(e, ok) ? 0u : (1u << gg);
                }
            }
            actv |= (uint32_t)__shfl_xor((int)actv, 1);
            actv |= (uint32_t)__shfl_xor((int)actv, 2);
        }
        // the start leaf's monotone prefix length mp (info word, beside the group maxima): slots
        // [0, mp) hold strictly increasing keys
        const uint32_t mpv = *reinterpret_cast<const uint32_t *>(t.head + (uint64_t)leafv * t.head_bytes +
                                                                 head_info_offset(t.cap, KW)) >> 16;
        uint64_t pf_vm, pf_col[KW];
        int pf_s = -1;
        uint32_t pf_leaf = 0xFFFFFFFFu;
        // the next scan's first active group; the scans of a chunk are mostly one transaction's
        // consecutive orders in one leaf, so that group is often the one already held in the
        // pf registers (data of a kernel's lifetime never changes): then nothing is loaded and
        // the scan starts without a round trip
        auto prefetch = [&](int jn) {
            const uint32_t an = rl32(actv, 4 * jn), ln = rl32(leafv, 4 * jn);
            const int s = an ? __builtin_ctz(an) : 0;
            if (ln == pf_leaf && s == pf_s) return;
            pf_s = s;
            pf_leaf = ln;
            pf_vm = head_vis(t, ln, pf_s);
#pragma unroll
            for (int w = 0; w < KW; ++w) pf_col[w] = t.okey[((uint64_t)ln * KW + w) * t.cap + pf_s * 64 + lane];
        };
        prefetch(0);
        uint32_t my_info = 0;  // lane j: scan j's candidate count e | 0x100 if an undecided visit continues
        // ---- stage A
        for (int j = 0; j < cnt; ++j) {
            const int src = 4 * j;
            uint64_t x[KW];
#pragma unroll
            for (int w = 0; w < KW; ++w) x[w] = rl64(ok[w], src);
            const uint32_t leaf = rl32(leafv, src);
            const uint32_t mp = rl32(mpv, src);
            uint64_t active = ballot(lane < (uint32_t)SPL && ((rl32(actv, src) >> lane) & 1));
            bool pending = true, mono = false;
            uint32_t kept = 0;
            while (active) {
                const int s = __builtin_ctzll(active);
                active &= active - 1;
                uint64_t vm, col[KW];
                const bool from_pf = pending && s == pf_s;
                // a later group may be the one just prefetched for the next scan (in flight
                // since this scan's first group was consumed)
                if (from_pf || (leaf == pf_leaf && s == pf_s)) {
                    vm = pf_vm;
#pragma unroll
                    for (int w = 0; w < KW; ++w) col[w] = pf_col[w];
                } else {
                    vm = head_vis(t, leaf, s);
#pragma unroll
                    for (int w = 0; w < KW; ++w) col[w] = t.okey[((uint64_t)leaf * KW + w) * t.cap + s * 64 + lane];
                }
                const bool vis = (vm >> lane) & 1;
                const uint64_t q = ballot(vis && !kw_lt<KW>(col, x));
                const uint32_t rank = kept + count_below(q);
                // fast path: nothing kept yet, the group lies in the monotone prefix and holds
                // more than scan_size qualifying records -- the kept scan_size + 1 records are
                // its first ones, already in key order (unique keys), so their ranks are their
                // slot order and the first e = scan_size are the candidates; no LDS list
                if (kept == 0 && (uint32_t)s * 64u + 64u <= mp && (uint32_t)__builtin_popcountll(q) > scan_size) {
                    if (((q >> lane) & 1) && rank < scan_size) {
                        bool pfx = true;
#pragma unroll
                        for (int w = 0; w < KW; ++w)
                            if ((uint32_t)w < words) pfx = pfx && col[w] == x[w];
                        s_cand[wv][j][rank] = pfx ? (uint16_t)(s * 64 + (int)lane) : kHole;
                    }
                    if (from_pf) {
                        pending = false;
                        if (j + 1 < cnt) prefetch(j + 1);
                    }
                    mono = true;
                    break;
                }
                const bool take = ((q >> lane) & 1) && rank <= scan_size;
                if (take) {
#pragma unroll
                    for (int w = 0; w < KW; ++w) lk[rank * KW + w] = col[w];
                    ls[rank] = (uint32_t)(s * 64) + lane;
                }
                if (from_pf) {
                    pending = false;
                    if (j + 1 < cnt) prefetch(j + 1);
                }
                kept += (uint32_t)__builtin_popcountll(ballot(take));
                if (kept > scan_size) break;
            }
            if (pending && j + 1 < cnt) prefetch(j + 1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t m = kept;
            uint32_t info = 0;
            if (mono) {
                info = scan_size;
            } else if (m > 0) {
                const bool mine = lane < m;
                uint64_t mk[KW];
                uint32_t mslot = 0;
#pragma unroll
                for (int w = 0; w < KW; ++w) mk[w] = mine ? lk[lane * KW + w] : 0ull;
                bool ord = true;
                if (mine) {
                    mslot = ls[lane];
                    if (lane > 0) {
                        uint64_t pk[KW];
#pragma unroll
                        for (int w = 0; w < KW; ++w) pk[w] = lk[(lane - 1) * KW + w];
                        ord = kw_lt<KW>(pk, mk);
                    }
                }
                uint32_t kr = lane;
                bool dup = false;
                if (ballot(!ord)) {
                    kr = 0;
                    for (uint32_t jj = 0; jj < m; ++jj) {
                        uint64_t kj[KW];
                        bool eq = jj != lane;
#pragma unroll
                        for (int w = 0; w < KW; ++w) {
                            kj[w] = lk[jj * KW + w];
                            eq = eq && kj[w] == mk[w];
                        }
                        kr += (mine && kw_lt<KW>(kj, mk)) ? 1u : 0u;
                        dup = dup || (mine && eq);
                    }
                }
                const uint32_t e = m < scan_size ? m : scan_size;
                if (ballot(dup)) {
                    info = 0x200u;  // equal keys share a rank: the general loop decides
                } else {
                    if (lane < e) s_cand[wv][j][lane] = kHole;
                    if (mine && kr < e) {
                        bool pfx = true;
#pragma unroll
                        for (int w = 0; w < KW; ++w)
                            if ((uint32_t)w < words) pfx = pfx && mk[w] == x[w];
                        if (pfx) s_cand[wv][j][kr] = (uint16_t)mslot;
                    }
                    info = e | (e == m && scan_size > e ? 0x100u : 0u);
                }
            }
            __builtin_amdgcn_wave_barrier();  // the LDS list is rewritten by the next scan
            if (lane == (uint32_t)j) my_info = info;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- stage B: lane j resolves scan j's candidates in rank order
        const uint32_t my_leaf = (uint32_t)__shfl((int)leafv, (int)(4 * (lane & 15)));
        const uint32_t my_rid = (uint32_t)__shfl((int)ridv, (int)(4 * (lane & 15)));
        uint32_t my_img = 0xFFFFFFFFu, my_st = ST_NOT_FOUND;
        bool found = false;
        if (lane < (uint32_t)cnt) {
            const uint32_t e = my_info & 0xFF;
            const uint64_t base = (uint64_t)my_leaf * t.cap;
            for (uint32_t c = 0; c < e; ++c) {
                const uint16_t sl = s_cand[wv][lane][c];
                if (sl == kHole) continue;
                uint8_t sv;
                const uint32_t im = scan_visible(t, t.slot[base + sl], my_rid, sv);
                if (sv == ST_LATEST || sv == ST_OLD) {
                    my_img = im;
                    my_st = sv;
                    found = true;
                    break;
                }
            }
        }
        // ---- undecided scans: marked for scan_first_rest_kernel
        if (lane < (uint32_t)cnt && ((!found && (my_info & 0x100u)) || (my_info & 0x200u))) my_st = kFirstUndecided;
        if (lane < (uint32_t)cnt) {
            img_out[c0 + lane] = my_img;
            st_out[c0 + lane] = (uint8_t)my_st;
        }
        __builtin_amdgcn_wave_barrier();  // s_cand is rewritten by the next chunk
    }
}

// The scans scan_first_split_kernel left undecided (st_out == kFirstUndecided): the general loop
// (scan_one_compact + FirstPrefixSink) from the start key, a wave per scan; 64 statuses are
// read per wave and step, so a batch without undecided scans costs one pass over st_out.
template <int SPL, int KW>
__global__ __launch_bounds__(256) void scan_first_rest_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                              uint64_t n, uint32_t scan_size,
                                                              const uint32_t *__restrict__ rids, uint32_t words,
                                                              uint32_t *__restrict__ img_out,
                                                              uint8_t *__restrict__ st_out) {
    __shared__ uint64_t s_keys[4][64 * KW];
    __shared__ uint32_t s_len[4][64], s_slot[4][64];
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t len = t.key_width;
    for (uint64_t c0 = wave * 64; c0 < n; c0 += nwaves * 64) {
        const uint64_t i = c0 + lane;
        uint64_t und = ballot(i < n && st_out[i] == kFirstUndecided);
        while (und) {
            const int b = __builtin_ctzll(und);
            und &= und - 1;
            const uint64_t k = c0 + (uint64_t)b;
            uint64_t x[KW];
            load_okey<KW>(keys, k, true, len, x);
            FirstPrefixSink<KW> sink;
#pragma unroll
            for (int w = 0; w < KW; ++w) sink.pre[w] = x[w];
            sink.words = words;
            sink.rid = rids ? rids[k] : 0xFFFFFFFEu;
            sink.img = 0xFFFFFFFFu;
            sink.st = ST_NOT_FOUND;
            const uint32_t leaf = uni32(resolve_leaf_uniform<false, KW>(t, x, len, true, lane));
            scan_one_compact<false, SPL, KW>(t, x, len, leaf, scan_size, lane, sink, s_keys[wv], s_len[wv],
                                             s_slot[wv]);
            if (lane == 0) {
                img_out[k] = sink.img;
                st_out[k] = (uint8_t)sink.st;
            }
        }
    }
}

// One wave per scan (grid-stride over scans): the start key's descent is wave-uniform, and a
// wide grid keeps many scans -- and their R rows in flight each -- resident per CU.
template <bool VARLEN, int SPL, int R, int KW = 1, bool VIS = false>
__global__ __launch_bounds__(256) void scan_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                   const uint16_t *__restrict__ lens, uint64_t n, uint32_t scan_size,
                                                   uint32_t *__restrict__ counts, uint8_t *__restrict__ recs,
                                                   const uint32_t *__restrict__ rids = nullptr,
                                                   uint8_t *__restrict__ row_status = nullptr) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t i = wave; i < n; i += nwaves) {
        uint32_t len;
        uint64_t ok[KW];
        const uint32_t leaf = scan_start<VARLEN, KW>(t, keys, lens, i, lane, ok, len);
        scan_one<VARLEN, SPL, R, KW, VIS>(t, ok, len, leaf, scan_size, recs + i * (uint64_t)scan_size * t.stride,
                                          counts + i, lane, VIS ? (rids ? rids[i] : 0xFFFFFFFEu) : 0u,
                                          VIS ? row_status + i * (uint64_t)scan_size : nullptr);
    }
}

// ----------------------------------------------------------------------------------------
// column-window range scan (stage_scan_batch_window / stage_index_scan_batch_window): per scanned
// record the payload bytes [payload_off, payload_off + len) instead of its row, and optionally
// the row's first key_pad bytes (its key).  Kernels of their own: scan_kernel's and
// scan_kernel_compact's instances stay the measured ones.

// scan_one_compact's sink of the window scan: the visit's heap rows go to the LDS list by rank
template <bool VIS>
struct WindowSink {
    uint64_t pos0;  // first output position of the scan: i * scan_size
    uint8_t *row_status;
    uint32_t rid;
    uint32_t *rk;  // the wave's LDS list, 64 words
    ScanWindowArgs a;
    template <int KW>
    __device__ __forceinline__ bool emit(const DevTable &t, uint64_t base, bool on, uint32_t mslot, uint32_t kr,
                                         uint32_t produced, const uint64_t *, uint32_t lane) {
        if (on) rk[kr & 63u] = kept_row<VIS>(t, t.slot[base + mslot], rid, row_status, produced + kr);
        const uint32_t e = (uint32_t)__builtin_popcountll(ballot(on));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        store_scan_windows(t, lane, pos0 + produced, e, rk, a);
        __builtin_amdgcn_wave_barrier();  // the list is rewritten on the next leaf
        return false;
    }
};

template <bool VARLEN, int SPL, int KW, bool VIS>
__global__ __launch_bounds__(256) void scan_window_kernel_compact(DevTable t, const uint64_t *__restrict__ keys,
                                                                  const uint16_t *__restrict__ lens, uint64_t n,
                                                                  uint32_t scan_size, uint32_t *__restrict__ counts,
                                                                  const uint32_t *__restrict__ rids,
                                                                  uint8_t *__restrict__ row_status, ScanWindowArgs a) {
    __shared__ uint64_t s_keys[4][64 * KW];
    __shared__ uint32_t s_len[4][64], s_slot[4][64], s_rank[4][64];
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t i = wave; i < n; i += nwaves) {
        uint32_t len;
        uint64_t ok[KW];
        const uint32_t leaf = scan_start<VARLEN, KW>(t, keys, lens, i, lane, ok, len);
        WindowSink<VIS> sink{i * (uint64_t)scan_size, VIS ? row_status + i * (uint64_t)scan_size : nullptr,
                             VIS ? (rids ? rids[i] : 0xFFFFFFFEu) : 0u, s_rank[wv], a};
        const uint32_t produced =
            scan_one_compact<VARLEN, SPL, KW>(t, ok, len, leaf, scan_size, lane, sink, s_keys[wv], s_len[wv], s_slot[wv]);
        if (lane == 0) counts[i] = produced;
    }
}

// scan_one with the ScanWindow policy: the row scan's collection, ranking and continuation, one
// body; the emitting lanes hold (heap row, rank) by slot, the LDS list s_rank (SPL * 64 words per
// wave) turns that into rank order for store_scan_windows.  R is unused by the window form.
template <bool VARLEN, int SPL, int KW, bool VIS>
__global__ __launch_bounds__(256) void scan_window_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                          const uint16_t *__restrict__ lens, uint64_t n,
                                                          uint32_t scan_size, uint32_t *__restrict__ counts,
                                                          const uint32_t *__restrict__ rids,
                                                          uint8_t *__restrict__ row_status, ScanWindowArgs a) {
    __shared__ uint32_t s_rank[4][SPL * 64];
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t i = wave; i < n; i += nwaves) {
        uint32_t len;
        uint64_t ok[KW];
        const uint32_t leaf = scan_start<VARLEN, KW>(t, keys, lens, i, lane, ok, len);
        scan_one<VARLEN, SPL, 4, KW, VIS>(t, ok, len, leaf, scan_size, nullptr, counts + i, lane,
                                          VIS ? (rids ? rids[i] : 0xFFFFFFFEu) : 0u,
                                          VIS ? row_status + i * (uint64_t)scan_size : nullptr,
                                          ScanWindow{i * (uint64_t)scan_size, s_rank[wv], &a});
    }
}

template <int KW, bool VIS, int R = 4>
static void launch_scan_w(const DevTable &t, const uint64_t *keys, uint64_t n, uint32_t scan_size, uint32_t *counts,
                          uint8_t *recs, const uint32_t *rids, uint8_t *st, hipStream_t s, int blocks) {
    with_slot_groups(t, [&](auto S) {
        if (scan_size <= 63)  // at most 64 kept records per leaf visit: group-skipping LDS form
            scan_kernel_compact<false, S(), KW, VIS><<<blocks, 256, 0, s>>>(t, keys, nullptr, n, scan_size, counts,
                                                                            recs, rids, st);
        else
            scan_kernel<false, S(), R, KW, VIS><<<blocks, 256, 0, s>>>(t, keys, nullptr, n, scan_size, counts, recs,
                                                                       rids, st);
    });
}

template <int R, bool VIS>
static void launch_scan_r(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t n,
                          uint32_t scan_size, uint32_t *counts, uint8_t *recs, const uint32_t *rids, uint8_t *st,
                          hipStream_t s, int blocks) {
    const bool var = t.key_width == 0;
    if (t.key_words == 2) return launch_scan_w<2, VIS>(t, keys, n, scan_size, counts, recs, rids, st, s, blocks);
    if (t.key_words == 4) return launch_scan_w<4, VIS>(t, keys, n, scan_size, counts, recs, rids, st, s, blocks);
    if (!var && t.cap > 128) return launch_scan_w<1, VIS, R>(t, keys, n, scan_size, counts, recs, rids, st, s, blocks);
    auto launch = [&](auto kernel) {
        kernel<<<blocks, 256, 0, s>>>(t, keys, lens, n, scan_size, counts, recs, rids, st);
    };
    if (t.cap == 64) {
        if (var) launch(scan_kernel<true, 1, R, 1, VIS>);
        else launch(scan_kernel<false, 1, R, 1, VIS>);
    } else {
        if (var) launch(scan_kernel<true, 2, R, 1, VIS>);
        else launch(scan_kernel<false, 2, R, 1, VIS>);
    }
}

hipError_t launch_scan(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t n, uint32_t scan_size,
                       uint32_t *counts, uint8_t *recs, hipStream_t s, const ScanTuning &tune, const uint32_t *rids,
                       uint8_t *row_status) {
    if (n == 0) return hipSuccess;
    const int blocks = grid_for(n, 4, max_blocks(tune));
    if (row_status) {  // IndexScanExecutor range branch: per-record visibility
        launch_scan_r<4, true>(t, keys, lens, n, scan_size, counts, recs, rids, row_status, s, blocks);
    } else {  // 4 rows in flight per wave (2 and 8 measured no faster)
        launch_scan_r<4, false>(t, keys, lens, n, scan_size, counts, recs, nullptr, nullptr, s, blocks);
    }
    return hipGetLastError();
}

// launch_scan's dispatch for the window kernels: the compact form for scans of at most 63 records
// on wide-key and large-leaf tables, the direct form everywhere else
template <bool VIS>
static hipError_t launch_scan_window_v(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t n,
                                       uint32_t scan_size, uint32_t *counts, const uint32_t *rids, uint8_t *st,
                                       const ScanWindowArgs &a, hipStream_t s, int blocks) {
    const bool var = t.key_width == 0;
    hipError_t e = hipErrorInvalidValue;  // variable-length keys in leaves above 128 slots: no scan kernel either
    with_geometry(t, [&](auto S, auto KW) {
        auto launch = [&](auto kernel) {
            kernel<<<blocks, 256, 0, s>>>(t, keys, lens, n, scan_size, counts, rids, st, a);
            e = hipGetLastError();
        };
        if constexpr (KW() > 1 || S() > 2) {
            if (KW() == 1 && var) return;
            if (scan_size <= 63) launch(scan_window_kernel_compact<false, S(), KW(), VIS>);
            else launch(scan_window_kernel<false, S(), KW(), VIS>);
        } else {
            if (var) launch(scan_window_kernel<true, S(), 1, VIS>);
            else launch(scan_window_kernel<false, S(), 1, VIS>);
        }
    });
    return e;
}

hipError_t launch_scan_window(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t n,
                              uint32_t scan_size, uint32_t row_off, uint32_t len, uint32_t key_pad, uint32_t *counts,
                              uint8_t *win, uint8_t *row_keys, hipStream_t s, const ScanTuning &tune,
                              const uint32_t *rids, uint8_t *row_status) {
    // the window and the key lie inside a heap row (window_piece's and the key writer's loads rest on it)
    if (len == 0 || (uint64_t)row_off + len > t.hstride || key_pad > t.hstride || (key_pad & 7u))
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (scan_size == 0)  // nothing to deliver: the counts are the row form's zeros
        return counts ? hipMemsetAsync(counts, 0, n * sizeof(uint32_t), s) : hipSuccess;
    if (!win) return hipErrorInvalidValue;
    const ScanWindowArgs a{WindowArgs{row_off, len, (len + 15u) >> 4, win}, row_keys, key_pad};
    const int blocks = grid_for(n, 4, max_blocks(tune));
    if (row_status) return launch_scan_window_v<true>(t, keys, lens, n, scan_size, counts, rids, row_status, a, s, blocks);
    return launch_scan_window_v<false>(t, keys, lens, n, scan_size, counts, nullptr, nullptr, a, s, blocks);
}

hipError_t launch_scan_pair(const DevTable &t0, const uint64_t *k0, uint32_t sz0, uint32_t *c0, uint8_t *r0,
                            const DevTable &t1, const uint64_t *k1, uint32_t sz1, uint32_t *c1, uint8_t *r1,
                            hipStream_t s) {
    if (!scan_pair_supported(t0, sz0, t1, sz1)) return hipErrorInvalidValue;
    with_slot_groups(t0, [&](auto S) {
        scan_pair_compact_kernel<S()><<<2, 64, 0, s>>>(t0, t1, k0, k1, sz0, sz1, c0, c1, r0, r1);
    });
    return hipGetLastError();
}

bool scan_pair_supported(const DevTable &t0, uint32_t sz0, const DevTable &t1, uint32_t sz1) {
    auto one = [](const DevTable &t, uint32_t sz) {
        return t.key_width == 8 && t.key_words == 1 && t.cap > 128 && sz >= 1 && sz <= 63;
    };
    return one(t0, sz0) && one(t1, sz1) && t0.cap == t1.cap;
}

hipError_t launch_scan_first(const DevTable &t, const uint64_t *keys, uint64_t n, uint32_t scan_size,
                             const uint32_t *rids, uint32_t words, uint32_t *img_out, uint8_t *st_out, hipStream_t s,
                             const ScanTuning &tune) {
    if (n == 0) return hipSuccess;
    if (t.key_width == 0 || scan_size == 0 || scan_size > 63) return hipErrorInvalidValue;
    const int blocks = grid_for((n + kFirstChunk - 1) / kFirstChunk, 4, max_blocks(tune));
    // scan_first_split_kernel decides the scans whose start leaf's first visit does, then
    // scan_first_rest_kernel runs the general loop for the rest.  Retired variants (measured
    // no faster): a single-scan kernel, NS scans in lockstep, the prefetching
    // "fast" kernel, the lane-parallel "mono" kernel, segmented stage A, a point-probe first
    // pass, the split kernel at 6 / 7 waves per SIMD.
    with_geometry(t, [&](auto S, auto KW) {
        scan_first_split_kernel<S(), KW(), 8><<<blocks, 256, 0, s>>>(t, keys, n, scan_size, rids, words, img_out,
                                                                     st_out);
        scan_first_rest_kernel<S(), KW()><<<grid_for((n + 63) / 64, 4, 4096), 256, 0, s>>>(t, keys, n, scan_size, rids,
                                                                                          words, img_out, st_out);
    });
    return hipGetLastError();
}

}  // namespace stage
