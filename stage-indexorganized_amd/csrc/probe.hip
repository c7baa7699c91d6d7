// probe.hip -- gfx950 (CDNA4, wave64) point probes of the index-organized read path: leaf resolve,
// the five probe kernels, window probes, the resident reader, revisit / ident / for-update, launchers.
// Integer/pointer work only (no MFMA).  Mapping:
//   * leaf probe: wave-per-probe.  64 lanes read the leaf head's fingerprints (1 byte per
//     slot, 0 = empty/invisible: one 64-B sector); ballot gives the fingerprint candidates, the
//     candidate lanes read their 32-B slot words and a second ballot confirms the order key:
//     first visible slot holding the key in slot order == BaseNode::SearchRecordMeta
//     (b_tree.cpp:18-122).
//   * visibility: wave-uniform scalar walk (BTree::Read copy path b_tree.cpp:2087-2123,
//     IndexScanExecutor executor.h:383-450); latest-version fast path inline.
#include <algorithm>

#include "kernel_api.hpp"
#include "launch_util.hpp"
#include "row_store.hpp"
#include "tree_search.hpp"

namespace stage {

template <int KW>
__global__ __launch_bounds__(256) void resolve_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                      const uint16_t *__restrict__ lens, uint64_t n, int le_child,
                                                      uint32_t *__restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t len = t.key_width ? t.key_width : (lens ? lens[i] : 8u);
    uint64_t ok[KW];
    load_okey<KW>(keys, i, true, len, ok);
    out[i] = t.key_width ? resolve_leaf<false, KW>(t, ok, len, le_child != 0)
                         : resolve_leaf<true, 1>(t, ok, len, le_child != 0);
}

// ----------------------------------------------------------------------------------------
// point probe

// Point probes of 8-byte and variable-length keys in leaves of 64 / 128 slots, a wave per chunk
// of 64 probes, G probes in flight per wave (wide keys and larger leaves: probe_lane_kernel /
// probe_split_kernel).
// ST: status record bytes -- 32 (stage_probe_out) or 16 (stage_probe_out16, opt-in: status |
// flags | hops, cstamp, copy_sstamp, rec_cstamp -- what IndexScanExecutor and PerformRead use)
// FAN: fan-out probes (the sharded front-end's coalesced requests, dist.hip): probe i's status
// record and row go to every caller position flist[k], k in [fan[i].lo, fan[i].hi) (flist null:
// the positions k themselves; fan null: {i, i + 1}, probe i's one position flist[i]) instead of
// position i -- the row leaves registers once per caller and no second pass copies it (rows of
// at most 1024 B, recs required).
template <bool VARLEN, int SPL, int G, int POL = 1, int ST = 32, bool FAN = false, bool DEST = false>
__global__ __launch_bounds__(256) void probe_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                    const uint16_t *__restrict__ lens,
                                                    const uint32_t *__restrict__ rids,
                                                    const uint32_t *__restrict__ leaf_in, uint64_t n,
                                                    stage_probe_out_dev *__restrict__ out,
                                                    uint8_t *__restrict__ recs, const FanRange *__restrict__ fan,
                                                    const uint32_t *__restrict__ flist,
                                                    const FanDest *__restrict__ dest = nullptr) {
    const uint32_t lane = lane_id();
    // FAN with per-segment destinations: the segment table in LDS (every thread reaches this
    // barrier: nothing returns before it)
    __shared__ uint32_t s_dend[DEST ? kFanDests : 1];
    __shared__ stage_probe_out_dev *s_dout[DEST ? kFanDests : 1];
    __shared__ uint8_t *s_drec[DEST ? kFanDests : 1];
    uint32_t nseg = 0;
    if constexpr (DEST) {
        nseg = dest->nseg;
        for (uint32_t g = threadIdx.x; g < nseg; g += blockDim.x)
            s_dend[g] = dest->end[g], s_dout[g] = dest->out[g], s_drec[g] = dest->recs[g];
        __syncthreads();
    }
    // threadIdx.x / 64 made provably wave-uniform: the chunk base and the output row addresses
    // live in SGPRs (probe_kernel<.., 8>: 78 VGPRs, 6 waves/SIMD, instead of 95 and 5)
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t out_chunks = t.stride >> 4;
    for (uint64_t base = wave * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        // lane < 64 always holds; without it hipcc allocates probe_kernel's registers differently
        // (<true, 2, 4>: 93 VGPRs instead of 94, fewer SGPR spills), which would have to be
        // re-timed: kept so that the instances are the measured ones, instruction for instruction
        const bool valid = lane < 64u && i < n;
        u32x4 my_a = u32x4{0, 0, 0, 0}, my_b = u32x4{0, 0, 0, 0};  // this lane's probe result
        const uint32_t len = t.key_width ? t.key_width : (lens && valid ? (uint32_t)lens[i] : 8u);
        const uint32_t rid = rids ? (valid ? rids[i] : 0u) : 0xFFFFFFFEu;
        FanRange my_fan = FanRange{0u, 0u};
        if (FAN && valid) my_fan = fan ? fan[i] : FanRange{(uint32_t)i, (uint32_t)i + 1u};
        uint64_t my_o = 0, my_r = 0;  // DEST: this lane's probe's segment's buffers
        if constexpr (DEST) {
            uint32_t sg = 0;
            for (uint32_t g = 0; g + 1 < nseg; ++g) sg += i >= s_dend[g] ? 1u : 0u;
            my_o = (uint64_t)s_dout[sg];
            my_r = (uint64_t)s_drec[sg];
        }
        uint64_t ok;
        load_okey<1>(keys, i, valid, len, &ok);
        uint32_t leaf = 0;
        if (valid) leaf = leaf_in ? leaf_in[i] : resolve_leaf<VARLEN, 1>(t, &ok, len, true);
        if (leaf > t.nseps) leaf = t.nseps;  // host-supplied ids are clamped to the table
        const int cnt = (int)((n - base) < 64 ? (n - base) : 64);
        // one probe in flight (G = 1, stage_set_probe_tuning only): the next probe's
        // fingerprint bytes load while this one runs, so a probe exposes one dependent round
        // trip (its candidates' slot words) instead of two
        constexpr bool PFH = G == 1;
        uint32_t nfp[SPL];
        if (PFH) {
            const uint8_t *h = t.head + (uint64_t)rl32(leaf, 0) * t.head_bytes;
#pragma unroll
            for (int s = 0; s < SPL; ++s) nfp[s] = h[s * 64 + lane];
        }
        for (int j0 = 0; j0 < cnt; j0 += G) {
            uint32_t lf[G], rd[G], xl[G];
            uint64_t x[G];
            uint32_t fpb[G][SPL];
            // phase 1: leaf heads of G probes -- the fingerprint bytes only: an empty or
            // invisible slot holds fingerprint 0, which no key has (key_fp_words), so the
            // visible masks behind them are not read
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int j = j0 + g < cnt ? j0 + g : cnt - 1;
                lf[g] = rl32(leaf, j);
                rd[g] = rl32(rid, j);
                x[g] = rl64(ok, j);
                xl[g] = VARLEN ? rl32(len, j) : t.key_width;
                if (PFH) {
#pragma unroll
                    for (int s = 0; s < SPL; ++s) fpb[g][s] = nfp[s];
                    if (j0 + 1 < cnt) {
                        const uint8_t *h = t.head + (uint64_t)rl32(leaf, j0 + 1) * t.head_bytes;
#pragma unroll
                        for (int s = 0; s < SPL; ++s) nfp[s] = h[s * 64 + lane];
                    }
                } else {
                    const uint8_t *h = t.head + (uint64_t)lf[g] * t.head_bytes;
#pragma unroll
                    for (int s = 0; s < SPL; ++s) fpb[g][s] = h[s * 64 + lane];
                }
            }
            // phase 2: fingerprint candidates read their slot words
            uint64_t wok[G][SPL], wmeta[G][SPL];
            uint32_t wnext[G][SPL], wimg[G][SPL];
            bool cand[G][SPL];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint32_t fx = key_fp_words(&x[g], 1);
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    cand[g][s] = fpb[g][s] == fx;
                    wok[g][s] = 0;
                    wmeta[g][s] = 0;
                    wnext[g][s] = 0;
                    wimg[g][s] = 0;
                    if (cand[g][s]) {
                        const SlotWords w = slot_words(t.slot + (uint64_t)lf[g] * t.cap + s * 64 + lane);
                        wok[g][s] = w.okey;
                        wmeta[g][s] = w.meta;
                        wnext[g][s] = w.next;
                        wimg[g][s] = w.image;
                    }
                }
            }
            // phase 3: confirm (order key, key length), first hit in slot order, visibility
            ProbeRes r[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                int slot = -1;
                uint64_t m = 0;
                uint32_t nx = 0, im = 0;
#pragma unroll
                for (int s = SPL - 1; s >= 0; --s) {
                    const bool hitl = cand[g][s] && wok[g][s] == x[g] && (!VARLEN || meta_keylen(wmeta[g][s]) == xl[g]);
                    const uint64_t hit = ballot(hitl);
                    if (hit) {
                        const int b = __builtin_ctzll(hit);
                        slot = s * 64 + b;
                        m = rl64(wmeta[g][s], b);
                        nx = rl32(wnext[g][s], b);
                        im = rl32(wimg[g][s], b);
                    }
                }
                const bool fast = slot >= 0 && !meta_inserting(m) && rd[g] >= meta_cstamp(m) &&
                                  (nx & kNextKindMask) != kNextCopy;
                if (fast) {
                    r[g].status = ST_LATEST;
                    r[g].flags = 0;
                    r[g].hops = 0;
                    r[g].slot = (uint32_t)slot;
                    r[g].meta_hi = (uint32_t)(m >> 32);
                    r[g].cstamp = rd[g];
                    r[g].rec_cstamp = meta_cstamp(m);
                    r[g].copy_sstamp = kMaxCid;
                    r[g].image = im;
                } else {
                    visibility(t, slot, m, nx, im, rd[g], r[g]);
                }
            }
            // phase 4 (FAN): G rows in flight, each stored at its caller positions with its
            // status record (lanes 0-1); up to 64 positions are loaded at once, one per lane
            if constexpr (FAN) {
                // the G rows and the first 64 caller positions of each request, all in flight
                // together (a request has at most kFanCap = 64 callers; longer runs loop)
                u32x4 v[G];
                uint32_t mine0[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    v[g] = u32x4{0, 0, 0, 0};
                    if (lane < out_chunks && r[g].image != 0xFFFFFFFFu)
                        v[g] = heap_chunk(t, r[g].image, lane);
                    const int j = j0 + g;
                    const uint32_t lo = rl32(my_fan.lo, j & 63), hi = rl32(my_fan.hi, j & 63);
                    const uint32_t kk = lo + lane;
                    mine0[g] = j < cnt && kk < hi ? (flist ? flist[kk] : kk) : 0u;
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int j = j0 + g;
                    if (j >= cnt) break;
                    u32x4 a, b;
                    pack_out(lf[g], r[g], a, b);
                    const u32x4 half = lane == 0 ? a : b;
                    const uint32_t lo = rl32(my_fan.lo, j), hi = rl32(my_fan.hi, j);
                    stage_probe_out_dev *o_j = out;
                    uint8_t *r_j = recs;
                    if constexpr (DEST) {  // probe j's segment's buffers (wave-uniform: scalar registers)
                        o_j = reinterpret_cast<stage_probe_out_dev *>(rl64(my_o, j));
                        r_j = reinterpret_cast<uint8_t *>(rl64(my_r, j));
                    }
                    for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
                        const uint32_t kk = k0 + lane;
                        const uint32_t mine = k0 == lo ? mine0[g] : kk < hi ? (flist ? flist[kk] : kk) : 0u;
                        const uint32_t kn = hi - k0 < 64u ? hi - k0 : 64u;
                        for (uint32_t k = 0; k < kn; ++k) {
                            const uint64_t pos = rl32(mine, (int)k);
                            if (lane < out_chunks) st16<POL>(v[g], r_j + pos * (uint64_t)t.stride, lane * 16u);
                            if (lane < 2) st16<POL>(half, reinterpret_cast<uint8_t *>(o_j + pos), lane * 16u);
                        }
                    }
                }
                continue;
            }
            // phase 4: tuple rows (G rows in flight), then nontemporal stores
            if (recs) {
                for (uint32_t c0 = 0; c0 < out_chunks; c0 += 64) {
                    const uint32_t c = c0 + lane;
                    u32x4 v[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        v[g] = u32x4{0, 0, 0, 0};
                        if (c < out_chunks && r[g].image != 0xFFFFFFFFu)
                            v[g] = heap_chunk(t, r[g].image, c);
                    }
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const int j = j0 + g;
                        if (j < cnt && c < out_chunks)
                            st16<POL>(v[g], recs + (base + j) * (uint64_t)t.stride, c * 16u);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                u32x4 a, b;
                pack_out(lf[g], r[g], a, b);
                if (lane == (uint32_t)(j0 + g)) {
                    my_a = a;
                    my_b = b;
                }
            }
        }
        // one coalesced 2-KiB (1-KiB) store of the chunk's 64 results
        if constexpr (FAN) {
        } else if constexpr (ST == 16) {
            if (valid)
                st16<POL>(u32x4{my_a.x, my_a.w, my_b.y, my_b.x}, reinterpret_cast<uint8_t *>(out) + base * 16u,
                          lane * 16u);
        } else {
            if (valid) {
                uint8_t *ob = reinterpret_cast<uint8_t *>(out + base);
                st16<POL>(my_a, ob, lane * 32u);
                st16<POL>(my_b, ob, lane * 32u + 16u);
            }
        }
    }
}

// ----------------------------------------------------------------------------------------
// column-window probe (stage_probe_batch_window): payload bytes [payload_off, payload_off + len)
// of the tuple instead of its whole row

// probe_kernel's probe (phases 1-3, G probes in flight per wave) with the window writer in place
// of the row copy: one launch, the geometries probe_kernel serves (keys of <= 8 bytes, leaves of
// 64 / 128 slots).  ST: status record bytes, as probe_kernel.  A kernel of its own: probe_kernel's
// instances stay the measured ones, and nothing here is tuned by stage_set_probe_tuning's group
// or by the store policy (nontemporal stores throughout).
template <bool VARLEN, int SPL, int G, int ST>
__global__ __launch_bounds__(256) void probe_window_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                           const uint16_t *__restrict__ lens,
                                                           const uint32_t *__restrict__ rids,
                                                           const uint32_t *__restrict__ leaf_in, uint64_t n,
                                                           stage_probe_out_dev *__restrict__ out, WindowArgs w) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = wave * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        const bool valid = i < n;
        u32x4 my_a = u32x4{0, 0, 0, 0}, my_b = u32x4{0, 0, 0, 0};  // this lane's probe result
        uint32_t my_img = 0xFFFFFFFFu;
        const uint32_t len = t.key_width ? t.key_width : (lens && valid ? (uint32_t)lens[i] : 8u);
        const uint32_t rid = rids ? (valid ? rids[i] : 0u) : 0xFFFFFFFEu;
        uint64_t ok;
        load_okey<1>(keys, i, valid, len, &ok);
        uint32_t leaf = 0;
        if (valid) leaf = leaf_in ? leaf_in[i] : resolve_leaf<VARLEN, 1>(t, &ok, len, true);
        if (leaf > t.nseps) leaf = t.nseps;  // host-supplied ids are clamped to the table
        const int cnt = (int)((n - base) < 64 ? (n - base) : 64);
        for (int j0 = 0; j0 < cnt; j0 += G) {
            uint32_t lf[G], rd[G], xl[G];
            uint64_t x[G];
            uint32_t fpb[G][SPL];
            // phase 1: the fingerprint bytes of G probes' leaf heads
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int j = j0 + g < cnt ? j0 + g : cnt - 1;
                lf[g] = rl32(leaf, j);
                rd[g] = rl32(rid, j);
                x[g] = rl64(ok, j);
                xl[g] = VARLEN ? rl32(len, j) : t.key_width;
                const uint8_t *h = t.head + (uint64_t)lf[g] * t.head_bytes;
#pragma unroll
                for (int s = 0; s < SPL; ++s) fpb[g][s] = h[s * 64 + lane];
            }
            // phase 2: fingerprint candidates read their slot words
            SlotWords sw[G][SPL];
            bool cand[G][SPL];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint32_t fx = key_fp_words(&x[g], 1);
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    cand[g][s] = fpb[g][s] == fx;
                    sw[g][s] = SlotWords{0, 0, 0, 0};
                    if (cand[g][s]) sw[g][s] = slot_words(t.slot + (uint64_t)lf[g] * t.cap + s * 64 + lane);
                }
            }
            // phase 3: confirm (order key, key length), first hit in slot order, visibility
#pragma unroll
            for (int g = 0; g < G; ++g) {
                int slot = -1;
                uint64_t m = 0;
                uint32_t nx = 0, im = 0;
#pragma unroll
                for (int s = SPL - 1; s >= 0; --s) {
                    const bool hitl =
                        cand[g][s] && sw[g][s].okey == x[g] && (!VARLEN || meta_keylen(sw[g][s].meta) == xl[g]);
                    const uint64_t hit = ballot(hitl);
                    if (hit) {
                        const int b = __builtin_ctzll(hit);
                        slot = s * 64 + b;
                        m = rl64(sw[g][s].meta, b);
                        nx = rl32(sw[g][s].next, b);
                        im = rl32(sw[g][s].image, b);
                    }
                }
                ProbeRes r;
                visibility(t, slot, m, nx, im, rd[g], r);
                u32x4 a, b;
                pack_out(lf[g], r, a, b);
                if (lane == (uint32_t)(j0 + g)) {
                    my_a = a;
                    my_b = b;
                    my_img = r.image;
                }
            }
        }
        // phase 4: the chunk's windows, then one coalesced store of its status records
        store_windows(t, lane, base, cnt, my_img, w);
        if constexpr (ST == 16) {
            if (valid)
                st16<1>(u32x4{my_a.x, my_a.w, my_b.y, my_b.x}, reinterpret_cast<uint8_t *>(out) + base * 16u, lane * 16u);
        } else {
            if (valid) {
                uint8_t *ob = reinterpret_cast<uint8_t *>(out + base);
                st16<1>(my_a, ob, lane * 32u);
                st16<1>(my_b, ob, lane * 32u + 16u);
            }
        }
    }
}

// The windows of probes already answered (32-B status records: the heap row is their image
// word): the second launch of the window probe on the tables probe_lane_kernel /
// probe_split_kernel serve.  A wave per 64 probes.
__global__ __launch_bounds__(256) void window_gather_kernel(DevTable t, const stage_probe_out_dev *__restrict__ out,
                                                            uint64_t n, WindowArgs w) {
    const uint32_t lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = wave * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        const uint32_t image = i < n ? out[i].w[6] : 0xFFFFFFFFu;
        store_windows(t, lane, base, (int)((n - base) < 64 ? (n - base) : 64), image, w);
    }
}

// ----------------------------------------------------------------------------------------
// resident single-key reader: one-wave workgroups poll a request ring in pinned host memory
// (the stage_reader_* adapter of BTree::Read callers, b_tree.cpp:2066-2129, without a launch
// per request).  Ticket q belongs to wave w = q % W as its k-th ticket, k = q / W, and lives in
// slot w * P + k % P of the ring (P = slots / W, a multiple of 64): concurrent callers land on
// different waves, and a wave's tickets are contiguous in the ring.  A caller writes its 16-B
// request record -- key, read id, then the tag (q + 1) << 4 | key length with release -- so a
// wave's poll is one 16-B load per lane over PCIe that brings the key along with the tag; the
// wave takes the published prefix of its
// current 64-ticket block, probes it (lane j = the block's j-th ticket throughout), writes the
// status record and the row into the slot and publishes done[slot] = q + 1 (system-scope
// release).  Every instance ends after life_ticks of the
// 100 MHz real-time counter or when *stop is set, saving its position in pos[w] for the next
// instance queued behind it on the same stream -- no wave outlives its instance's lifetime.

// one wave-uniform probe (request j of the wave's lanes) with one probe in flight
template <bool VARLEN, int SPL, bool FU = false>
__device__ __forceinline__ void ring_probe_one(const DevTable &t, uint32_t lane, int j, uint32_t leaf_l, uint64_t ok_l,
                                               uint32_t len_l, uint32_t rid_l, uint8_t *row, uint32_t out_chunks,
                                               u32x4 &a, u32x4 &b, uint32_t &id_loc, uint32_t &id_next) {
    const uint32_t lf = rl32(leaf_l, j);
    const uint64_t x = rl64(ok_l, j);
    const uint32_t xl = VARLEN ? rl32(len_l, j) : t.key_width;
    const uint32_t rd = rl32(rid_l, j);
    const uint8_t *h = t.head + (uint64_t)lf * t.head_bytes;
    const uint32_t fx = key_fp_words(&x, 1);
    int slot = -1;
    uint64_t m = 0;
    uint32_t nx = 0, im = 0, lc = 0;
#pragma unroll
    for (int s = SPL - 1; s >= 0; --s) {  // first hit in slot order (SearchRecordMeta)
        const bool cand = h[s * 64 + lane] == fx;
        uint64_t wok = 0, wmeta = 0;
        uint32_t wnext = 0, wimg = 0, wloc = 0;
        if (cand) {
            // unpacked here, not through slot_words(): with it hipcc numbers the reader's
            // registers differently (same counts), and the reader is timed separately
            const u32x4 *w = reinterpret_cast<const u32x4 *>(t.slot + (uint64_t)lf * t.cap + s * 64 + lane);
            const u32x4 w0 = w[0], w1 = w[1];
            wok = ((uint64_t)w0.y << 32) | w0.x;
            wmeta = ((uint64_t)w0.w << 32) | w0.z;
            wnext = w1.x;
            wimg = w1.y;
            wloc = w1.z;
        }
        const uint64_t hit = ballot(cand && wok == x && (!VARLEN || meta_keylen(wmeta) == xl));
        if (hit) {
            const int bl = __builtin_ctzll(hit);
            slot = s * 64 + bl;
            m = rl64(wmeta, bl);
            nx = rl32(wnext, bl);
            im = rl32(wimg, bl);
            lc = rl32(wloc, bl);
        }
    }
    ProbeRes r;
    visibility<FU>(t, slot, m, nx, im, rd, r);
    id_loc = r.status == ST_NOT_FOUND ? 0u : lc;
    id_next = r.status == ST_NOT_FOUND ? 0u : nx;
    for (uint32_t c0 = 0; c0 < out_chunks; c0 += 64) {
        const uint32_t c = c0 + lane;
        if (c < out_chunks) {
            u32x4 v = u32x4{0, 0, 0, 0};
            if (r.image != 0xFFFFFFFFu) v = heap_chunk(t, r.image, c);
            reinterpret_cast<u32x4 *>(row)[c] = v;
        }
    }
    pack_out(lf, r, a, b);
}

template <bool VARLEN, int SPL>
__global__ __launch_bounds__(64) void resident_reader_kernel(DevTable t, ReaderRing g) {
    const uint32_t lane = lane_id();
    const uint32_t w = blockIdx.x;
    const uint32_t out_chunks = t.stride >> 4;
    const uint32_t per = g.slots / g.waves;
    uint64_t pos = g.pos[w];  // this wave's next k
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        if (__hip_atomic_load(g.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > g.life_ticks) break;
        const uint64_t blk = pos & ~63ull;
        const uint32_t d = (uint32_t)(pos & 63u);
        const uint32_t s0 = w * per + (uint32_t)(blk % per);
        const uint32_t want = (uint32_t)((blk + lane) * g.waves + w + 1u);
        u32x4 rq = u32x4{0, 0, 0, 0};
        // the whole record in one load (volatile: system-coherent, past the caches); the tag is
        // written after the key and read id, in the same 16-B line, so seeing it brings them
        if (lane >= d) rq = *reinterpret_cast<const volatile u32x4 *>(g.req + s0 + lane);
        const bool ready = lane >= d && (rq.w >> 4) == (want & 0x0FFFFFFFu);
        const uint64_t m = ballot(ready) >> d;
        const uint32_t k = ~m ? (uint32_t)__builtin_ctzll(~m) : 64u;  // published prefix from d
        if (k == 0) {
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        const bool mine = lane >= d && lane < d + k;
        // tag low nibble: key length - 1 (bits 0-2), is_for_update (bit 3)
        const uint32_t len = t.key_width ? t.key_width : (mine ? (rq.w & 7u) + 1u : 8u);
        const uint32_t rid = mine ? rq.z : 0u;
        const bool fu = mine && (rq.w & 8u) != 0;
        const uint64_t ok = order_key(mine ? ((uint64_t)rq.y << 32 | rq.x) : 0ull, len);
        uint32_t leaf = mine ? resolve_leaf<VARLEN, 1>(t, &ok, len, true) : 0u;
        u32x4 my_a = u32x4{0, 0, 0, 0}, my_b = u32x4{0, 0, 0, 0};
        uint32_t my_loc = 0, my_next = 0;
        for (uint32_t j = d; j < d + k; ++j) {
            u32x4 a, b;
            uint32_t il, in;
            if (rl32(fu ? 1u : 0u, (int)j))
                ring_probe_one<VARLEN, SPL, true>(t, lane, (int)j, leaf, ok, len, rid,
                                                  g.rows + (uint64_t)(s0 + j) * t.stride, out_chunks, a, b, il, in);
            else
                ring_probe_one<VARLEN, SPL>(t, lane, (int)j, leaf, ok, len, rid, g.rows + (uint64_t)(s0 + j) * t.stride,
                                            out_chunks, a, b, il, in);
            if (lane == j) {
                my_a = a;
                my_b = b;
                my_loc = il;
                my_next = in;
            }
        }
        if (mine) {
            u32x4 *o = reinterpret_cast<u32x4 *>(g.out + s0 + lane);
            o[0] = my_a;
            o[1] = my_b;
            g.ident[2 * (uint64_t)(s0 + lane)] = my_loc;
            g.ident[2 * (uint64_t)(s0 + lane) + 1] = my_next;
            // status record and row before the flag, system-wide
            __hip_atomic_store(g.done + s0 + lane, want, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        pos += k;
    }
    if (lane == 0) g.pos[w] = pos;
}

// Point probes of the tables probe_kernel does not serve (fixed-width keys of 9..32 bytes, or
// 8-byte keys in leaves above 128 slots) in two stages per chunk of CH probes (4 / 16 / 64 by
// batch size, launch_probe) -- probe_kernel's results:
//  A (wave per probe, in turn): the leaf head's fingerprint bytes (the next 4 probes' in flight
//    while this one runs -- the next one only for leaves above 256 slots, whose larger heads
//    would cost occupancy), one ballot per slot group, and the candidate slots in slot order
//    written to LDS (at most kProbeCand; a probe with more is resolved by a lane-serial walk of
//    its leaf head in stage B);
//  B (lane per probe, all CH together): each candidate's slot word and remaining key words in
//    slot order until the first confirmed one (SearchRecordMeta's first hit), then
//    visibility() -- per lane, so the CH probes' dependent loads are in flight together instead
//    of one probe's at a time.
//  Rows (if requested) are then copied wave-wide, probe by probe, as probe_kernel's phase 4.
constexpr int kProbeCand = 8;

// ---- steps shared by probe_split_kernel and probe_lane_kernel (fixed-width keys, a lane per
// probe of the wave's chunk).  The chunk prologue (device batch size, wave position, read id,
// key words, leaf clamp) is written out in both: as a helper it changes the code hipcc
// generates for all of their instances, down to how blockDim is read, for six lines saved.

// slot sl of the probe's leaf (first slot lb = leaf * cap) against its key: the slot word's
// order key, then the other key words (okey planes).  A match sets slot / m / nx / im
// (visibility()'s arguments).
template <int KW>
__device__ __forceinline__ bool confirm_slot(const DevTable &t, uint32_t leaf, uint64_t lb, uint32_t sl,
                                             const uint64_t *ok, int &slot, uint64_t &m, uint32_t &nx,
                                             uint32_t &im) {
    const SlotWords w = slot_words(t.slot + lb + sl);
    bool eq = w.okey == ok[0];
#pragma unroll
    for (int k = 1; k < KW; ++k) eq = eq && t.okey[((uint64_t)leaf * KW + k) * t.cap + sl] == ok[k];
    if (eq) {
        slot = (int)sl;
        m = w.meta;
        nx = w.next;
        im = w.image;
    }
    return eq;
}

// the chunk's output: the rows (if requested) wave-wide, probe by probe (lane j holds probe
// base + j's result, cnt probes), then every probe's 32-B status record from its lane
__device__ __forceinline__ void store_chunk(const DevTable &t, uint32_t lane, uint64_t base, int cnt, bool valid,
                                            uint32_t leaf, const ProbeRes &r, stage_probe_out_dev *out,
                                            uint8_t *recs, uint32_t out_chunks) {
    if (recs) {
        for (int j = 0; j < cnt; ++j) {
            const uint32_t img = rl32(r.image, j);
            for (uint32_t c0 = 0; c0 < out_chunks; c0 += 64) {
                const uint32_t c = c0 + lane;
                if (c >= out_chunks) continue;
                u32x4 v = u32x4{0, 0, 0, 0};
                if (img != 0xFFFFFFFFu) v = heap_chunk(t, img, c);
                st16<1>(v, recs + (base + j) * (uint64_t)t.stride, c * 16u);
            }
        }
    }
    if (valid) {
        u32x4 a, b;
        pack_out(leaf, r, a, b);
        uint8_t *ob = reinterpret_cast<uint8_t *>(out + base);
        st16<1>(a, ob, lane * 32u);
        st16<1>(b, ob, lane * 32u + 16u);
    }
}

template <int SPL, int KW, int CH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void probe_split_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ rids,
                                                          const uint32_t *__restrict__ leaf_in, uint64_t n,
                                                          stage_probe_out_dev *__restrict__ out,
                                                          uint8_t *__restrict__ recs,
                                                          const uint64_t *__restrict__ dn) {
    __shared__ uint16_t s_cand[4][64][kProbeCand];
    if (dn) n = *dn < n ? *dn : n;  // the batch's size as a previous kernel left it (launched for n at most)
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t out_chunks = t.stride >> 4;
    const uint32_t len = t.key_width;
    for (uint64_t base = wave * CH; base < n; base += nwaves * CH) {
        const uint64_t i = base + lane;
        const bool valid = lane < (uint32_t)CH && i < n;
        const uint32_t rid = rids ? (valid ? rids[i] : 0u) : 0xFFFFFFFEu;
        uint64_t ok[KW];
        load_okey<KW>(keys, i, valid, len, ok);
        uint32_t leaf = 0;
        if (valid) leaf = leaf_in ? leaf_in[i] : resolve_leaf<false, KW>(t, ok, len, true);
        if (leaf > t.nseps) leaf = t.nseps;  // host-supplied ids are clamped to the table
        const uint32_t fx_mine = key_fp_words(ok, KW);
        const int cnt = (int)((n - base) < CH ? (n - base) : CH);
        // ---- stage A: the heads of the next PD probes in flight while one is examined (a ring of
        // PD register sets, indexed statically by unrolling PD probes per pass)
        constexpr int PD = SPL <= 4 ? 4 : 1;
        uint32_t pf[PD][SPL];
#pragma unroll
        for (int d = 0; d < PD; ++d) {
            if (d < cnt) {
                const uint8_t *h = t.head + (uint64_t)rl32(leaf, d) * t.head_bytes;
#pragma unroll
                for (int s = 0; s < SPL; ++s) pf[d][s] = h[s * 64 + lane];
            }
        }
        uint32_t my_nc = 0;
        for (int j0 = 0; j0 < cnt; j0 += PD) {
#pragma unroll
            for (int u = 0; u < PD; ++u) {
                const int j = j0 + u;
                if (j >= cnt) break;
                uint32_t fpb[SPL];
#pragma unroll
                for (int s = 0; s < SPL; ++s) fpb[s] = pf[u][s];
                if (j + PD < cnt) {
                    const uint8_t *h = t.head + (uint64_t)rl32(leaf, j + PD) * t.head_bytes;
#pragma unroll
                    for (int s = 0; s < SPL; ++s) pf[u][s] = h[s * 64 + lane];
                }
                const uint32_t fx = rl32(fx_mine, j);
                uint32_t nc = 0;
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    const bool c = fpb[s] == fx;
                    const uint64_t cm = ballot(c);
                    const uint32_t r = nc + count_below(cm);
                    if (c && r < (uint32_t)kProbeCand) s_cand[wv][j][r] = (uint16_t)(s * 64 + lane);
                    nc += (uint32_t)__builtin_popcountll(cm);
                }
                if (lane == (uint32_t)j) my_nc = nc;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- stage B: lane = probe
        int slot = -1;
        uint64_t m = 0;
        uint32_t nx = 0, im = 0;
        if (valid) {
            const uint64_t lb = (uint64_t)leaf * t.cap;
            if (my_nc <= (uint32_t)kProbeCand) {
                for (uint32_t c = 0; c < my_nc; ++c)
                    if (confirm_slot<KW>(t, leaf, lb, s_cand[wv][lane][c], ok, slot, m, nx, im)) break;
            } else {  // more candidates than the list holds: walk the head in slot order
                const uint8_t *h = t.head + (uint64_t)leaf * t.head_bytes;
                for (uint32_t sl = 0; sl < t.cap; ++sl)
                    if (h[sl] == fx_mine && confirm_slot<KW>(t, leaf, lb, sl, ok, slot, m, nx, im)) break;
            }
        }
        ProbeRes r;
        visibility(t, slot, m, nx, im, rid, r);
        store_chunk(t, lane, base, cnt, valid, leaf, r, out, recs, out_chunks);
        __builtin_amdgcn_wave_barrier();  // s_cand is rewritten by the next chunk
    }
}

// Wave-cooperative lower bound of the wave's 64 fixed-width keys (one per lane, le_child), for
// the one-probe-in-flight tables whose separators are 2-4 words: per level a team of f lanes
// (the node's fanout, 16 inner / 8 bottom) reads one key's node, one entry per lane -- 64 / f
// keys per load instruction, each team's f entries contiguous -- instead of every lane reading
// its own whole node (a lane's 16 loads of 16 B touch 64 different nodes per instruction: 4x the
// cache lines for the texture addresser, CH-Q2's STOCK probe ran it 58-79 % busy, r05/lanepmc).
// A team's ballot bits count its key's separators below the key; the keys and their nodes pass
// through LDS (s_x: 64 keys, s_node: their nodes at this level).  All 64 lanes take part.
template <int KW>
__device__ __forceinline__ uint32_t coop_lower_bound(const DevTable &t, const uint64_t *ok, uint32_t lane,
                                                     uint64_t *s_x, uint32_t *s_node) {
#pragma unroll
    for (int j = 0; j < KW; ++j) s_x[lane * KW + j] = ok[j];
    uint32_t node = 0;
    for (int lvl = (int)t.levels - 1; lvl >= 0; --lvl) {
        const uint32_t f = lvl > 0 ? (uint32_t)kTreeFanout : (uint32_t)kLeafFanout;
        const uint32_t sh = lvl > 0 ? 4u : 3u, kpr = 64u >> sh;  // keys per round: 4 / 8
        const uint32_t rounds = 64u / kpr;                        // 16 / 8
        s_node[lane] = node;
        __builtin_amdgcn_wave_barrier();
        const uint64_t lbase = t.level_off[lvl];
        const uint32_t e = lane & (f - 1), kq = lane >> sh;  // entry of the node, key in the round
        const uint32_t my_round = lane / kpr, my_team = lane % kpr;
        uint64_t ball = 0;
        // rounds in batches of 8 whose loads are in flight together (8 x KW x 8 B per lane)
        constexpr int kBatch = 8;
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += kBatch) {
            if ((uint32_t)r0 >= rounds) break;  // wave-uniform: the bottom level has 8 rounds
            uint64_t w[kBatch][KW];
#pragma unroll
            for (int r = 0; r < kBatch; ++r) {
                const uint32_t kk = (uint32_t)(r0 + r) * kpr + kq;
                const uint64_t ent = lbase + (uint64_t)s_node[kk] * f + e;
#pragma unroll
                for (int j = 0; j < KW; ++j) w[r][j] = t.tree[ent * KW + j];
            }
#pragma unroll
            for (int r = 0; r < kBatch; ++r) {
                const uint32_t kk = (uint32_t)(r0 + r) * kpr + kq;
                uint64_t x[KW];
#pragma unroll
                for (int j = 0; j < KW; ++j) x[j] = s_x[kk * KW + j];
                const uint64_t b = __builtin_amdgcn_ballot_w64(kw_lt<KW>(w[r], x));
                ball = (uint32_t)(r0 + r) == my_round ? b : ball;
            }
        }
        const uint32_t cnt = (uint32_t)__builtin_popcountll((ball >> (my_team * f)) & ((1ull << f) - 1));
        node = node * f + cnt;
        __builtin_amdgcn_wave_barrier();  // s_node is rewritten by the next level
    }
    return node < t.nseps ? node : t.nseps;
}

// Point probes of the same instances as probe_split_kernel with a lane per probe throughout
// (the default for leaves of up to 256 slots): each lane descends, loads its leaf head's
// fingerprint bytes itself (SPL x 4 16-B loads, all in flight), finds its candidate slots in slot
// order with byte-wise compares in registers, and confirms the first three candidates in up to
// three rounds of loads that every lane of the wave issues together -- 64 probes' dependent
// loads in flight per wave at every step instead of 4-16 (SearchRecordMeta's first hit; a probe
// with more than three candidates falls back to a walk of the rest).  Then visibility() and the
// rows, wave-wide, as probe_split_kernel.
// MISS (launch_probe_missed): the hit is also evaluated at every read id mrids[0..mnq) and a
// probe that produces no tuple at read id q sets missed[q] -- launch_revisit_segments' miss pass
// folded into the probe, whose slot word is already in registers.
template <int SPL, int KW, bool MISS = false>
__global__ __launch_bounds__(256) void probe_lane_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                         const uint32_t *__restrict__ rids,
                                                         const uint32_t *__restrict__ leaf_in, uint64_t n,
                                                         stage_probe_out_dev *__restrict__ out,
                                                         uint8_t *__restrict__ recs, const uint64_t *__restrict__ dn,
                                                         const uint32_t *__restrict__ mrids = nullptr,
                                                         uint32_t mnq = 0, int32_t *__restrict__ missed = nullptr) {
    static_assert(SPL <= 4, "head of at most 256 slots in registers");
    __shared__ uint64_t s_x[4][64 * KW];
    __shared__ uint32_t s_node[4][64];
    if (dn) n = *dn < n ? *dn : n;  // the batch's size as a previous kernel left it (launched for n at most)
    const uint32_t lane = lane_id(), wv = uni32(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t out_chunks = t.stride >> 4;
    const uint32_t len = t.key_width;
    for (uint64_t base = wave * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        const bool valid = i < n;
        const uint32_t rid = rids ? (valid ? rids[i] : 0u) : 0xFFFFFFFEu;
        uint64_t ok[KW];
        load_okey<KW>(keys, i, valid, len, ok);
        uint32_t leaf = 0;
        if (leaf_in) leaf = valid ? leaf_in[i] : 0u;
        else leaf = coop_lower_bound<KW>(t, ok, lane, s_x[wv], s_node[wv]);  // every lane takes part
        if (!valid) leaf = 0;
        if (leaf > t.nseps) leaf = t.nseps;
        // the lane-local leaf search, down to visibility(): probe_rows_kernel holds the same lines with KW = 1
        // (a shared helper moved probe_lane_kernel<1, 4, *> from 113 / 115 to 115 / 117 VGPRs): fix both
        const uint32_t rep = (key_fp_words(ok, KW) & 0xFFu) * 0x01010101u;
        // the head: fingerprint byte j = slot j
        u32x4 hv[SPL * 4];
        const u32x4 *hp = reinterpret_cast<const u32x4 *>(t.head + (uint64_t)leaf * t.head_bytes);
#pragma unroll
        for (int q = 0; q < SPL * 4; ++q) hv[q] = valid ? hp[q] : u32x4{0, 0, 0, 0};
        // candidates in slot order: the first three kept, the count of all
        uint32_t c0 = 0, c1 = 0, c2 = 0, nc = 0;
#pragma unroll
        for (int q = 0; q < SPL * 4; ++q) {
            const uint32_t wq[4] = {hv[q].x, hv[q].y, hv[q].z, hv[q].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t w = wq[e] ^ rep;
                uint32_t zm = ~(((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;  // bytes equal to the fingerprint
                while (zm) {
                    const uint32_t sl = (uint32_t)(q * 16 + e * 4) + ((uint32_t)__builtin_ctz(zm) >> 3);
                    c0 = nc == 0 ? sl : c0;
                    c1 = nc == 1 ? sl : c1;
                    c2 = nc == 2 ? sl : c2;
                    ++nc;
                    zm &= zm - 1;
                }
            }
        }
        if (!valid) nc = 0;
        int slot = -1;
        uint64_t m = 0;
        uint32_t nx = 0, im = 0;
        const uint64_t lb = (uint64_t)leaf * t.cap;
        auto confirm = [&](uint32_t sl) { return confirm_slot<KW>(t, leaf, lb, sl, ok, slot, m, nx, im); };
        // rounds: every lane still looking confirms its next candidate, the loads together
        if (nc > 0) confirm(c0);
        if (slot < 0 && nc > 1) confirm(c1);
        if (slot < 0 && nc > 2) confirm(c2);
        if (slot < 0 && nc > 3) {  // rare: walk the rest of the head in slot order
            const uint8_t *h = t.head + (uint64_t)leaf * t.head_bytes;
            const uint8_t fx = (uint8_t)rep;
            for (uint32_t sl = c2 + 1; sl < t.cap; ++sl)
                if (h[sl] == fx && confirm(sl)) break;
        }
        ProbeRes r;
        visibility(t, slot, m, nx, im, rid, r);
        if (MISS && valid)
            for (uint32_t q = 0; q < mnq; ++q) {
                ProbeRes rq;
                visibility(t, slot, m, nx, im, mrids[q], rq);
                if (rq.status != ST_LATEST && rq.status != ST_COPY && rq.status != ST_OLD) atomicOr(missed + q, 1);
            }
        store_chunk(t, lane, base, (int)((n - base) < 64 ? (n - base) : 64), valid, leaf, r, out, recs, out_chunks);
    }
}

// Point probes of probe_kernel's fixed-width geometry (keys of at most 8 bytes, leaves of 64 /
// 128 slots) in its second form (ProbeTuning::form = 1, stage_set_probe_form): the front end a
// lane per probe as probe_lane_kernel's -- descent, the leaf head's fingerprint bytes as SPL x 4
// 16-B loads, byte-wise compares in registers, the first three candidates confirmed in rounds
// that all lanes issue together, then the walk of the rest; visibility() per lane with the
// latest-version fast path inline -- and no broadcast, ballot or LDS: probe_kernel's phases 1-3
// are wave-uniform work that 63 of 64 lanes repeat.  The status record and the image
// index stay in the probe's own lane; invalid lanes (i >= n) issue no load.  The back end is
// probe_kernel's phase 4 with R rows in flight per wave: image by readlane, the heap row's 16-B
// chunks, nontemporal stores -- the same bytes as probe_kernel's (a probe without a tuple gets a
// zero row, row bytes past the heap row are zero, nothing is written when recs is null).
// A kernel of its own so that probe_kernel's instances stay instruction for instruction as measured.
template <int SPL, int R, int ST>
__global__ __launch_bounds__(256) void probe_rows_kernel(DevTable t, const uint64_t *__restrict__ keys,
                                                         const uint32_t *__restrict__ rids,
                                                         const uint32_t *__restrict__ leaf_in, uint64_t n,
                                                         stage_probe_out_dev *__restrict__ out,
                                                         uint8_t *__restrict__ recs) {
    static_assert(SPL <= 2, "probe_kernel's leaves: 64 or 128 slots");
    const uint32_t lane = lane_id();
    // wave-uniform wave index: the chunk base and the row addresses in SGPRs (as probe_kernel)
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t out_chunks = t.stride >> 4;
    const uint32_t len = t.key_width;
    for (uint64_t base = wave * 64; base < n; base += nwaves * 64) {
        const uint64_t i = base + lane;
        const bool valid = i < n;
        const uint32_t rid = rids ? (valid ? rids[i] : 0u) : 0xFFFFFFFEu;
        uint64_t ok;
        load_okey<1>(keys, i, valid, len, &ok);
        uint32_t leaf = 0;
        if (valid) leaf = leaf_in ? leaf_in[i] : resolve_leaf<false, 1>(t, &ok, len, true);
        if (leaf > t.nseps) leaf = t.nseps;  // host-supplied ids are clamped to the table
        // the lane-local leaf search, down to the ProbeRes: probe_lane_kernel holds the same lines with KW key
        // words (a shared helper changed that kernel's register counts): fix both
        const uint32_t rep = (key_fp_words(&ok, 1) & 0xFFu) * 0x01010101u;
        // the head: fingerprint byte j = slot j
        u32x4 hv[SPL * 4];
        const u32x4 *hp = reinterpret_cast<const u32x4 *>(t.head + (uint64_t)leaf * t.head_bytes);
#pragma unroll
        for (int q = 0; q < SPL * 4; ++q) hv[q] = valid ? hp[q] : u32x4{0, 0, 0, 0};
        // candidates in slot order: the first three kept, the count of all
        uint32_t c0 = 0, c1 = 0, c2 = 0, nc = 0;
#pragma unroll
        for (int q = 0; q < SPL * 4; ++q) {
            const uint32_t wq[4] = {hv[q].x, hv[q].y, hv[q].z, hv[q].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t w = wq[e] ^ rep;
                uint32_t zm = ~(((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;  // bytes equal to the fingerprint
                while (zm) {
                    const uint32_t sl = (uint32_t)(q * 16 + e * 4) + ((uint32_t)__builtin_ctz(zm) >> 3);
                    c0 = nc == 0 ? sl : c0;
                    c1 = nc == 1 ? sl : c1;
                    c2 = nc == 2 ? sl : c2;
                    ++nc;
                    zm &= zm - 1;
                }
            }
        }
        if (!valid) nc = 0;
        int slot = -1;
        uint64_t m = 0;
        uint32_t nx = 0, im = 0;
        const uint64_t lb = (uint64_t)leaf * t.cap;
        auto confirm = [&](uint32_t sl) { return confirm_slot<1>(t, leaf, lb, sl, &ok, slot, m, nx, im); };
        // rounds: every lane still looking confirms its next candidate, the loads together
        if (nc > 0) confirm(c0);
        if (slot < 0 && nc > 1) confirm(c1);
        if (slot < 0 && nc > 2) confirm(c2);
        if (slot < 0 && nc > 3) {  // rare: walk the rest of the head in slot order
            const uint8_t *h = t.head + (uint64_t)leaf * t.head_bytes;
            const uint8_t fx = (uint8_t)rep;
            for (uint32_t sl = c2 + 1; sl < t.cap; ++sl)
                if (h[sl] == fx && confirm(sl)) break;
        }
        ProbeRes r;
        if (slot >= 0 && !meta_inserting(m) && rid >= meta_cstamp(m) && (nx & kNextKindMask) != kNextCopy) {
            r.status = ST_LATEST;
            r.flags = 0;
            r.hops = 0;
            r.slot = (uint32_t)slot;
            r.meta_hi = (uint32_t)(m >> 32);
            r.cstamp = rid;
            r.rec_cstamp = meta_cstamp(m);
            r.copy_sstamp = kMaxCid;
            r.image = im;
        } else {
            visibility(t, slot, m, nx, im, rid, r);
        }
        // the chunk's 64 status records, one coalesced 2-KiB (1-KiB) store from their lanes
        if (valid) {
            u32x4 a, b;
            pack_out(leaf, r, a, b);
            if constexpr (ST == 16) {
                st16<1>(u32x4{a.x, a.w, b.y, b.x}, reinterpret_cast<uint8_t *>(out) + base * 16u, lane * 16u);
            } else {
                uint8_t *ob = reinterpret_cast<uint8_t *>(out + base);
                st16<1>(a, ob, lane * 32u);
                st16<1>(b, ob, lane * 32u + 16u);
            }
        }
        if (!recs) continue;
        // the rows, wave-wide, R in flight
        const int cnt = (int)((n - base) < 64 ? (n - base) : 64);
        for (int j0 = 0; j0 < cnt; j0 += R) {
            for (uint32_t k0 = 0; k0 < out_chunks; k0 += 64) {
                const uint32_t c = k0 + lane;
                u32x4 v[R];
#pragma unroll
                for (int g = 0; g < R; ++g) {
                    const uint32_t img = rl32(r.image, j0 + g < cnt ? j0 + g : cnt - 1);
                    v[g] = u32x4{0, 0, 0, 0};
                    if (c < out_chunks && img != 0xFFFFFFFFu) v[g] = heap_chunk(t, img, c);
                }
#pragma unroll
                for (int g = 0; g < R; ++g) {
                    const int j = j0 + g;
                    if (j < cnt && c < out_chunks) st16<1>(v[g], recs + (base + j) * (uint64_t)t.stride, c * 16u);
                }
            }
        }
    }
}

// ----------------------------------------------------------------------------------------
// launchers

hipError_t launch_resolve(const DevTable &t, const uint64_t *keys, const uint16_t *lens, uint64_t n, int le_child,
                          uint32_t *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned b = (unsigned)((n + 255) / 256);
    with_key_words(t, [&](auto KW) { resolve_kernel<KW()><<<b, 256, 0, s>>>(t, keys, lens, n, le_child, out); });
    return hipGetLastError();
}

constexpr uint64_t kSmallBelow = 16384;  // 64-probe chunks: about the waves the chip holds at once

hipError_t launch_probe(const DevTable &t, const uint64_t *keys, const uint16_t *lens, const uint32_t *rids,
                        const uint32_t *leaf_in, uint64_t n, stage_probe_out_dev *out, uint8_t *recs, hipStream_t s,
                        const ProbeTuning &tune, const uint64_t *d_n, uint64_t shape_n) {
    if (n == 0) return hipSuccess;
    if (d_n) {  // device-sized batches: the wide-key / large-leaf kernels only
        if (!(t.key_words > 1 || (t.key_width != 0 && t.cap > 128))) return hipErrorInvalidValue;
    }
    const int mb = max_blocks(tune);
    const int blocks = grid_for((n + 63) / 64, 4, mb);
    const bool var = t.key_width == 0;
    // wide fixed-width keys, and 8-byte keys in leaves above 128 slots (small rows): leaves of
    // up to 1024 slots -- probe_lane_kernel for leaves of up to 256 slots, probe_split_kernel
    // above (in 16-probe wave chunks when 64-probe ones cannot fill the chip).  probe_kernel
    // serves neither.
    if (t.key_words > 1 || (!var && t.cap > 128)) {
        // launch shape from the expected size (a device-sized batch's hint), the grid from n
        const uint64_t sn = d_n && shape_n ? std::min(shape_n, n) : n;
        const bool small = (sn + 63) / 64 < (uint64_t)kSmallBelow;  // fewer 64-probe chunks than the chip holds waves
        // tiny batches (fewer 16-probe chunks than a quarter of that, e.g. CH-Q2's ~2.5 K item
        // lookups): 4-probe wave chunks, a quarter of the serial probes per wave
        const bool tiny = (sn + 15) / 16 < (uint64_t)kSmallBelow / 4;
        with_geometry(t, [&](auto S, auto KW) {
            if constexpr (S() <= 4) {  // the lane kernel strides over the batch: its grid from the expected size too
                probe_lane_kernel<S(), KW()><<<grid_for((sn + 63) / 64, 4, mb), 256, 0, s>>>(t, keys, rids, leaf_in, n,
                                                                                             out, recs, d_n);
            } else if (tiny) {
                probe_split_kernel<S(), KW(), 4><<<grid_for((sn + 3) / 4, 4, mb), 256, 0, s>>>(t, keys, rids, leaf_in, n,
                                                                                               out, recs, d_n);
            } else if (small) {
                probe_split_kernel<S(), KW(), 16><<<grid_for((sn + 15) / 16, 4, mb), 256, 0, s>>>(t, keys, rids, leaf_in,
                                                                                                  n, out, recs, d_n);
            } else {
                probe_split_kernel<S(), KW(), 64><<<blocks, 256, 0, s>>>(t, keys, rids, leaf_in, n, out, recs, d_n);
            }
        });
        return hipGetLastError();
    }
    // the lane-per-probe form (stage_set_probe_form): fixed-width keys at the default group and
    // store policy; every other shape, and form WAVE, keeps probe_kernel
    if (!var && tune.form == kProbeFormLane && tune.group == 8 && tune.store == 1 &&
        (tune.status_bytes != 16 || t.cap == 64)) {
        auto launch_rows = [&](auto kernel) { kernel<<<blocks, 256, 0, s>>>(t, keys, rids, leaf_in, n, out, recs); };
        if (tune.status_bytes == 16) launch_rows(probe_rows_kernel<1, kProbeRows, 16>);
        else if (t.cap == 64) launch_rows(probe_rows_kernel<1, kProbeRows, 32>);
        else launch_rows(probe_rows_kernel<2, kProbeRows, 32>);
        return hipGetLastError();
    }
    // probe_kernel<VARLEN, SPL, G, POL, ST>: 10 of its 12 instances, the other 2 in launch_probe_fanout
    auto launch = [&](auto kernel) {
        kernel<<<blocks, 256, 0, s>>>(t, keys, lens, rids, leaf_in, n, out, recs, nullptr, nullptr, nullptr);
    };
    if (tune.status_bytes == 16) {  // opt-in lean status records: the YCSB geometry only
        if (var || t.cap != 64 || tune.group != 8 || tune.store != 1) return hipErrorInvalidValue;
        launch(probe_kernel<false, 1, 8, 1, 16>);
        return hipGetLastError();
    }
    if (t.cap == 64) {
        if (var) launch(probe_kernel<true, 1, 4>);
        else if (tune.group == 1) launch(probe_kernel<false, 1, 1>);
        else if (tune.group == 2) launch(probe_kernel<false, 1, 2>);
        else if (tune.group == 4) launch(probe_kernel<false, 1, 4>);
        else if (tune.store == 0) launch(probe_kernel<false, 1, 8, 0>);
        else if (tune.store == 2) launch(probe_kernel<false, 1, 8, 2>);
        else launch(probe_kernel<false, 1, 8>);
    } else {
        if (var) launch(probe_kernel<true, 2, 4>);
        else launch(probe_kernel<false, 2, 4>);
    }
    return hipGetLastError();
}

hipError_t launch_probe_window(const DevTable &t, const uint64_t *keys, const uint16_t *lens, const uint32_t *rids,
                               const uint32_t *leaf_in, uint64_t n, uint32_t row_off, uint32_t len,
                               stage_probe_out_dev *out, uint8_t *win, hipStream_t s, const ProbeTuning &tune) {
    // the window lies inside a heap row (window_piece's loads rest on it)
    if (len == 0 || (uint64_t)row_off + len > t.hstride || (n && !win)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const WindowArgs w{row_off, len, (len + 15u) >> 4, win};
    const int mb = max_blocks(tune);
    const int blocks = grid_for((n + 63) / 64, 4, mb);
    const bool var = t.key_width == 0;
    if (t.key_words > 1 || (!var && t.cap > 128)) {
        // probe_lane_kernel / probe_split_kernel tables: status records only, then the windows
        // from their image words, both on the caller's stream
        ProbeTuning full = tune;
        full.status_bytes = 32;
        const hipError_t e = launch_probe(t, keys, lens, rids, leaf_in, n, out, nullptr, s, full);
        if (e != hipSuccess) return e;
        window_gather_kernel<<<blocks, 256, 0, s>>>(t, out, n, w);
        return hipGetLastError();
    }
    if (tune.status_bytes == 16 && (var || t.cap != 64)) return hipErrorInvalidValue;  // as launch_probe
    hipError_t e = hipErrorInvalidValue;  // a leaf size probe_kernel does not serve either
    with_slot_groups(t, [&](auto S) {
        if constexpr (S() <= 2) {
            auto launch = [&](auto kernel) {
                kernel<<<blocks, 256, 0, s>>>(t, keys, lens, rids, leaf_in, n, out, w);
                e = hipGetLastError();
            };
            // probes in flight per wave: probe_kernel's default shapes
            if (var) {
                launch(probe_window_kernel<true, S(), 4, 32>);
            } else if constexpr (S() == 1) {
                if (tune.status_bytes == 16) launch(probe_window_kernel<false, 1, 8, 16>);
                else launch(probe_window_kernel<false, 1, 8, 32>);
            } else {
                launch(probe_window_kernel<false, 2, 4, 32>);
            }
        }
    });
    return e;
}

hipError_t launch_probe_missed(const DevTable &t, const uint64_t *keys, uint64_t n, stage_probe_out_dev *out,
                               hipStream_t s, const ProbeTuning &tune, const uint64_t *d_n, uint64_t shape_n,
                               const uint32_t *mrids, uint32_t mnq, int32_t *missed) {
    if (!probe_missed_supported(t)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const uint64_t sn = d_n && shape_n ? std::min(shape_n, n) : n;
    const int blocks = grid_for((sn + 63) / 64, 4, max_blocks(tune));
    with_geometry(t, [&](auto S, auto KW) {
        if constexpr (S() <= 4)  // probe_missed_supported: leaves of up to 256 slots
            probe_lane_kernel<S(), KW(), true><<<blocks, 256, 0, s>>>(t, keys, nullptr, nullptr, n, out, nullptr, d_n,
                                                                      mrids, mnq, missed);
    });
    return hipGetLastError();
}

bool probe_missed_supported(const DevTable &t) {
    // the lane kernel's instances: wide fixed-width keys, or 8-byte keys in leaves above 128
    // slots, in leaves of up to 256 slots
    const bool wide = t.key_words > 1 || (t.key_width != 0 && t.cap > 128);
    return wide && t.key_width != 0 && t.cap <= 256 && (t.cap == 64 || t.cap == 128 || t.cap == 256);
}

hipError_t launch_probe_fanout(const DevTable &t, const uint64_t *keys, const uint32_t *rids, uint64_t n,
                               const FanRange *fan, const uint32_t *flist, stage_probe_out_dev *out, uint8_t *recs,
                               hipStream_t s, const ProbeTuning &tune, const FanDest *dest) {
    if (!probe_fanout_supported(t)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if ((!recs && !dest) || (!fan && !flist)) return hipErrorInvalidValue;
    const int blocks = grid_for((n + 63) / 64, 4, max_blocks(tune));
    if (dest)
        probe_kernel<false, 1, 4, 1, 32, true, true><<<blocks, 256, 0, s>>>(t, keys, nullptr, rids, nullptr, n, out,
                                                                            recs, fan, flist, dest);
    else
        probe_kernel<false, 1, 8, 1, 32, true><<<blocks, 256, 0, s>>>(t, keys, nullptr, rids, nullptr, n, out, recs,
                                                                      fan, flist);
    return hipGetLastError();
}

bool probe_fanout_supported(const DevTable &t) {
    return t.key_width != 0 && t.key_words == 1 && t.cap == 64 && t.stride <= 1024;
}

// launch_revisit: thread per (key i, read id q), revisit_one (visibility.hpp)
__global__ __launch_bounds__(256) void revisit_kernel(DevTable t, const stage_probe_out_dev *__restrict__ base,
                                                      uint64_t n, const uint32_t *__restrict__ rids, uint32_t nq,
                                                      const uint32_t *__restrict__ perm,
                                                      stage_probe_out_dev *__restrict__ out,
                                                      const uint64_t *__restrict__ dn) {
    if (dn) n = *dn < n ? *dn : n;  // out[q * n + i] with the device count n
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * nq) return;
    const uint64_t i = g % n, q = g / n;
    const u32x4 *bp = reinterpret_cast<const u32x4 *>(base + i);
    u32x4 a = bp[0], b = bp[1];
    revisit_one(t, rids[q], a, b);
    u32x4 *op = reinterpret_cast<u32x4 *>(out + q * n + (perm ? perm[i] : i));
    op[0] = a;
    op[1] = b;
}

// launch_revisit_segments, the misses: thread per (probe i, kRevisitQ read ids) -- the probe's
// status record and slot word are loaded once and the visibility walk redone per read id; nothing
// is stored but a miss (rare: the transaction aborts)
constexpr uint32_t kRevisitQ = 16;
__global__ __launch_bounds__(256) void revisit_missed_kernel(DevTable t, const stage_probe_out_dev *__restrict__ base,
                                                             uint64_t n, const uint32_t *__restrict__ rids, uint32_t nq,
                                                             int32_t *__restrict__ missed, const uint64_t *__restrict__ dn) {
    if (dn) n = *dn < n ? *dn : n;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * ((nq + kRevisitQ - 1) / kRevisitQ)) return;
    const uint64_t i = g % n;
    const uint32_t q0 = (uint32_t)(g / n) * kRevisitQ, q1 = q0 + kRevisitQ < nq ? q0 + kRevisitQ : nq;
    const u32x4 *bp = reinterpret_cast<const u32x4 *>(base + i);
    const u32x4 a0 = bp[0];
    const uint32_t slot = a0.z & 0xFFFF, leaf = a0.y;
    const bool redo = (a0.x & 0xFF) != ST_NOT_FOUND && slot < t.cap && leaf < t.nleaves;
    SlotInfo si = {};
    if (redo) si = t.slot[(uint64_t)leaf * t.cap + slot];
    for (uint32_t q = q0; q < q1; ++q) {
        uint32_t st = a0.x & 0xFF;
        if (redo) {
            ProbeRes r;
            visibility(t, (int)slot, si.meta, si.next, si.image, rids[q], r);
            st = r.status;
        }
        if (st != ST_LATEST && st != ST_COPY && st != ST_OLD) atomicOr(missed + q, 1);
    }
}

// launch_revisit_segments, the last probes: thread per (read id q, segment k)
__global__ __launch_bounds__(256) void revisit_last_kernel(DevTable t, const stage_probe_out_dev *__restrict__ base,
                                                           const uint64_t *__restrict__ seg_off,
                                                           const uint32_t *__restrict__ seg_cnt, uint32_t nseg,
                                                           const uint32_t *__restrict__ rids, uint32_t nq,
                                                           stage_probe_out_dev *__restrict__ last,
                                                           const uint64_t *__restrict__ dseg) {
    if (dseg) nseg = *dseg < nseg ? (uint32_t)*dseg : nseg;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (uint64_t)nseg * nq) return;
    const uint32_t k = (uint32_t)(g % nseg), q = (uint32_t)(g / nseg);
    const uint32_t c = seg_cnt[k];
    if (c == 0) return;
    const u32x4 *bp = reinterpret_cast<const u32x4 *>(base + seg_off[k] + c - 1);
    u32x4 a = bp[0], b = bp[1];
    revisit_one(t, rids[q], a, b);
    u32x4 *op = reinterpret_cast<u32x4 *>(last + g);
    op[0] = a;
    op[1] = b;
}

hipError_t launch_revisit_segments(const DevTable &t, const stage_probe_out_dev *base, uint64_t n,
                                   const uint64_t *seg_off, const uint32_t *seg_cnt, uint32_t nseg,
                                   const uint32_t *rids, uint32_t nq, stage_probe_out_dev *last, int32_t *missed,
                                   hipStream_t s, const uint64_t *d_n, const uint64_t *d_nseg) {
    if (nq == 0) return hipSuccess;
    const uint64_t tm = n * ((nq + kRevisitQ - 1) / kRevisitQ), tl = (uint64_t)nseg * nq;
    if (tm) revisit_missed_kernel<<<(unsigned)((tm + 255) / 256), 256, 0, s>>>(t, base, n, rids, nq, missed, d_n);
    if (tl)
        revisit_last_kernel<<<(unsigned)((tl + 255) / 256), 256, 0, s>>>(t, base, seg_off, seg_cnt, nseg, rids, nq, last,
                                                                         d_nseg);
    return hipGetLastError();
}

hipError_t launch_revisit(const DevTable &t, const stage_probe_out_dev *base, uint64_t n, const uint32_t *rids,
                          uint32_t nq, const uint32_t *perm, stage_probe_out_dev *out, hipStream_t s,
                          const uint64_t *d_n) {
    if (n == 0 || nq == 0) return hipSuccess;
    revisit_kernel<<<(unsigned)((n * nq + 255) / 256), 256, 0, s>>>(t, base, n, rids, nq, perm, out, d_n);
    return hipGetLastError();
}

// stage_probe_ident: a probe's hit slot (leaf, slot in its status record) -> the slot word's
// location handle and next handle, from the same published image.  A thread per probe.
__global__ __launch_bounds__(256) void ident_kernel(DevTable t, const stage_probe_out_dev *__restrict__ out, uint64_t n,
                                                    uint32_t *__restrict__ ident) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32x4 a = reinterpret_cast<const u32x4 *>(out + i)[0];
    const uint32_t status = a.x & 0xFF, leaf = a.y, slot = a.z & 0xFFFF;
    uint32_t loc = 0, next = 0;
    if (status != ST_NOT_FOUND && slot < t.cap && leaf < t.nleaves) {
        const u32x4 w1 = reinterpret_cast<const u32x4 *>(t.slot + (uint64_t)leaf * t.cap + slot)[1];
        next = w1.x;
        loc = w1.z;
    }
    reinterpret_cast<uint2 *>(ident)[i] = make_uint2(loc, next);
}

// stage_probe_batch_ex's is_for_update probes: a second pass over the flagged probes of a batch
// the ordinary probe has answered (so the probe kernels stay as they are).  The hit slot is in
// each status record -- also for an in-flight record the ordinary rule left NOT_FOUND (an
// uncommitted insert without a copy) -- and its slot word gives the for-update outcome
// (visibility<true>); the status record is rewritten and the row re-copied from the leaf image.
// A wave takes 64 probes and walks its flagged ones wave-uniformly (lanes 0-1 store the record,
// every lane a 16-B chunk of the row).
__global__ __launch_bounds__(256) void for_update_kernel(DevTable t, const uint8_t *__restrict__ fu,
                                                         const uint32_t *__restrict__ rids, uint64_t n,
                                                         stage_probe_out_dev *__restrict__ out, uint8_t *__restrict__ recs) {
    const uint32_t lane = lane_id();
    const uint64_t base = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + uni32(threadIdx.x >> 6)) * 64;
    const uint64_t i = base + lane;
    uint64_t todo = ballot(i < n && fu[i] != 0);
    const uint32_t chunks = t.stride >> 4;
    while (todo) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint64_t p = base + (uint64_t)j;
        const u32x4 *op = reinterpret_cast<const u32x4 *>(out + p);
        u32x4 a = op[0], b = op[1];
        const uint32_t rid = rids ? rids[p] : 0xFFFFFFFEu;
        const uint32_t slot = a.z & 0xFFFF, leaf = a.y;
        uint32_t image = 0xFFFFFFFFu;
        if (slot < t.cap && leaf < t.nleaves) {
            const SlotInfo si = t.slot[(uint64_t)leaf * t.cap + slot];
            ProbeRes r;
            visibility<true>(t, (int)slot, si.meta, si.next, si.image, rid, r);
            pack_out(leaf, r, a, b);
            image = r.image;
        } else {
            a.x |= 2u << 8;  // no record: NOT_FOUND stays, flagged for update
        }
        if (lane < 2) reinterpret_cast<u32x4 *>(out + p)[lane] = lane == 0 ? a : b;
        if (recs) {
            for (uint32_t c = lane; c < chunks; c += 64) {
                u32x4 v = u32x4{0, 0, 0, 0};
                if (image != 0xFFFFFFFFu) v = heap_chunk(t, image, c);
                reinterpret_cast<u32x4 *>(recs + p * (uint64_t)t.stride)[c] = v;
            }
        }
    }
}

hipError_t launch_for_update(const DevTable &t, const uint8_t *fu, const uint32_t *rids, uint64_t n,
                             stage_probe_out_dev *out, uint8_t *recs, hipStream_t s) {
    if (n == 0) return hipSuccess;
    for_update_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(t, fu, rids, n, out, recs);
    return hipGetLastError();
}

hipError_t launch_ident(const DevTable &t, const stage_probe_out_dev *out, uint64_t n, uint32_t *ident, hipStream_t s) {
    if (n == 0) return hipSuccess;
    ident_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(t, out, n, ident);
    return hipGetLastError();
}

hipError_t launch_resident_reader(const DevTable &t, const ReaderRing &g, hipStream_t s) {
    if (t.key_words != 1 || g.waves == 0 || g.slots % (64 * g.waves)) return hipErrorInvalidValue;
    const dim3 grid(g.waves), block(64);
    if (t.key_width == 0 && t.cap > 128) return hipErrorInvalidValue;
    with_slot_groups(t, [&](auto S) {
        if (t.key_width != 0) resident_reader_kernel<false, S()><<<grid, block, 0, s>>>(t, g);
        else if constexpr (S() <= 2) resident_reader_kernel<true, S()><<<grid, block, 0, s>>>(t, g);
    });
    return hipGetLastError();
}

}  // namespace stage
