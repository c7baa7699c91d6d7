// row_store.hpp -- slot and heap-row reads and the output stores of the probe and scan kernels:
//   * tuple copy: 63 lanes x 16 B = the 1008-B [key|payload] row (Record::New b_tree.h:407-428),
//     read from a 128-B aligned heap row, written with nontemporal stores.
#pragma once
#include "visibility.hpp"
#include "wave.hpp"

namespace stage {
// chunk c (16 B) of heap row img; zeros past the heap row (an output stride above the heap
// stride, stage_set_output_layout: the rest of the output row is zero, not the next heap row)
__device__ __forceinline__ u32x4 heap_chunk(const DevTable &t, uint32_t img, uint32_t c) {
    return c < (t.hstride >> 4) ? reinterpret_cast<const u32x4 *>(t.heap + (uint64_t)img * t.hstride)[c]
                                : u32x4{0, 0, 0, 0};
}

// a slot's two 16-B words as a probe candidate reads them (SlotInfo without the padding)
struct SlotWords {
    uint64_t okey, meta;
    uint32_t next, image;
};
__device__ __forceinline__ SlotWords slot_words(const SlotInfo *p) {
    const u32x4 *w = reinterpret_cast<const u32x4 *>(p);
    const u32x4 w0 = w[0], w1 = w[1];
    return SlotWords{((uint64_t)w0.y << 32) | w0.x, ((uint64_t)w0.w << 32) | w0.z, w1.x, w1.y};
}

// 16-B output store at base + off (base wave-uniform).  POL 0: temporal; 1: nontemporal (the
// line is still kept in the XCD's L2); 2: write-through (sc1 buffer store: the line leaves L2,
// so the output stream does not evict cached rows, heads and separator nodes --
// MI355X_MICROARCH.md, store flavours).  Measured (scripts/ab_store.py, 100M rows): 1 is
// fastest (6.35 ms), 0 +1.7 %, 2 +2.6 %; nontemporal heap-row loads on top of 1 +5 %.
template <int POL>
__device__ __forceinline__ void st16(u32x4 v, uint8_t *base, uint32_t off) {
    if constexpr (POL == 2) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7FFFFFFF, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)off, 0, 16);
    } else {
        // plain pointer arithmetic (u32x4 *) + chunk: the (base, off) form above, used for the
        // flat stores too, raised probe_kernel<.., 8> from 95 to 154 VGPRs (3 waves/SIMD
        // instead of 5) and cost 9 % of the launch time
        u32x4 *p = reinterpret_cast<u32x4 *>(base) + (off >> 4);
        if constexpr (POL == 1) __builtin_nontemporal_store(v, p);
        else *p = v;
    }
}

// What a window launch carries beside the probe's arguments (wave-uniform).
struct WindowArgs {
    uint32_t src;   // first source byte inside the heap row: key pad + payload_off
    uint32_t len;   // window bytes, >= 1; src + len <= key pad + payload <= hstride
    uint32_t W;     // 16-B pieces per window: stage_window_stride(len) / 16
    uint8_t *win;   // n windows of 16 * W bytes
};

// 16-B piece c of the window of heap row img.  The source byte src + 16 * c is in general not
// 16-B aligned (key pad 8 + column offset 100 = byte 108), so the piece comes out of the one or
// two aligned 16-B chunks that hold it: the second is read only when the piece's last byte lies
// in it, and that byte is below src + len <= hstride, so no load leaves the row's own hstride
// bytes (the last heap row is not overrun).  The shift is the same for every piece of a launch
// (src & 15), so it selects between registers with scalar conditions: no indexed register array.
// Bytes past len are zero.
__device__ __forceinline__ u32x4 window_piece(const DevTable &t, uint32_t img, const WindowArgs &w, uint32_t c) {
    const uint32_t s = w.src + 16u * c;           // first source byte of the piece
    const uint32_t left = w.len - 16u * c;        // window bytes from this piece on (>= 1)
    const uint32_t nb = left < 16u ? left : 16u;  // bytes of this piece
    const uint32_t sh = uni32(w.src & 15u);
    const u32x4 *row = reinterpret_cast<const u32x4 *>(t.heap + (uint64_t)img * t.hstride);
    const u32x4 lo = row[s >> 4];
    u32x4 hi = u32x4{0, 0, 0, 0};
    if (sh + nb > 16u) hi = row[(s >> 4) + 1u];
    const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t ds = sh >> 2, bs = 8u * (sh & 3u);
    uint32_t e[5];  // the five words that hold the piece's 16 bytes, from word ds on
#pragma unroll
    for (int k = 0; k < 5; ++k)
        e[k] = ds == 0 ? d[k] : ds == 1 ? d[k + 1] : ds == 2 ? d[k + 2] : d[k + 3];
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[k] = (uint32_t)(((((uint64_t)e[k + 1]) << 32) | e[k]) >> bs);
        const uint32_t have = nb > 4u * k ? nb - 4u * k : 0u;  // window bytes in output word k
        o[k] &= have >= 4u ? ~0u : ((1u << (8u * have)) - 1u);
    }
    return u32x4{o[0], o[1], o[2], o[3]};
}

// The windows of one wave's chunk of cnt <= 64 probes, lane j holding probe base + j's heap row
// (0xFFFFFFFF: the probe yields no tuple, its window is zero) -- the shape store_chunk receives.
// The chunk's cnt * W output pieces are consecutive in memory, so they are stored wave-wide and
// coalesced whatever W is: piece q = 64 * k + lane belongs to probe q / W, piece q % W, and takes
// that probe's heap row from its lane (ds_bpermute; every lane of the wave is active here).  A
// probe's pieces may straddle two iterations (W = 7).  U pieces per lane are in flight together.
// Called by every lane of the wave.
template <int U = 4>
__device__ __forceinline__ void store_windows(const DevTable &t, uint32_t lane, uint64_t base, int cnt, uint32_t image,
                                              const WindowArgs &w) {
    const uint32_t total = (uint32_t)cnt * w.W;
    uint8_t *wb = w.win + base * (16ull * w.W);
    for (uint32_t q0 = 0; q0 < total; q0 += 64u * U) {
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t q = q0 + 64u * u + lane;
            const uint32_t p = q / w.W, c = q - p * w.W;
            const uint32_t img = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((p & 63u) << 2), (int)image);
            v[u] = u32x4{0, 0, 0, 0};
            if (q < total && img != 0xFFFFFFFFu) v[u] = window_piece(t, img, w, c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t q = q0 + 64u * u + lane;
            if (q < total) st16<1>(v[u], wb, q * 16u);
        }
    }
}

template <int R>
__device__ __forceinline__ void copy_rows(const DevTable &t, const uint32_t *img, const uint32_t *dst, int n,
                                          uint8_t *recs, uint32_t lane) {
    const uint32_t chunks = t.stride >> 4;
    for (uint32_t c0 = 0; c0 < chunks; c0 += 64) {
        const uint32_t c = c0 + lane;
        u32x4 v[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            v[k] = u32x4{0, 0, 0, 0};
            if (k < n && c < chunks && img[k] != 0xFFFFFFFFu)
                v[k] = heap_chunk(t, img[k], c);
        }
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (k < n && c < chunks)
                __builtin_nontemporal_store(v[k], reinterpret_cast<u32x4 *>(recs + (uint64_t)dst[k] * t.stride) + c);
    }
}

// Rows of at most 32 16-B chunks (512 B): the emitting lanes' rows (lane b of em: heap row
// img, output position dst) copied with the whole wave spread over (row, chunk) pairs -- U
// loads in flight per lane cover 64 * U / chunks rows per round trip (16 rows of 256 B), where
// copy_rows moves R rows per round trip whatever their size.  Same bytes as copy_rows.
template <int U>
__device__ __forceinline__ void copy_rows_flat(const DevTable &t, uint64_t em, uint32_t img, uint32_t dst,
                                               uint8_t *recs, uint32_t lane) {
    const uint32_t chunks = t.stride >> 4;
    const uint32_t rpr = (uint32_t)(U * 64) / chunks, nrows = (uint32_t)__builtin_popcountll(em);
    uint32_t rk[U], ck[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t f = (uint32_t)u * 64u + lane;
        rk[u] = f / chunks;
        ck[u] = f - rk[u] * chunks;
    }
    for (uint32_t r0 = 0; r0 < nrows; r0 += rpr) {
        u32x4 v[U];
        uint32_t d[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t k = r0 + rk[u];
            ok[u] = rk[u] < rpr && k < nrows;
            const int src = ok[u] ? (int)kth_set_bit(em, k) : 0;
            const uint32_t im = (uint32_t)__shfl((int)img, src);
            d[u] = (uint32_t)__shfl((int)dst, src);
            v[u] = u32x4{0, 0, 0, 0};
            if (ok[u] && im != 0xFFFFFFFFu) v[u] = heap_chunk(t, im, ck[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (ok[u]) __builtin_nontemporal_store(v[u], reinterpret_cast<u32x4 *>(recs + (uint64_t)d[u] * t.stride) + ck[u]);
    }
}

// IndexScanExecutor range branch (executor.h:456-530) for one iterator record: the leaf
// image when rid >= its commit id, else the TupleHeader version with begin <= rid <= end
// (nothing when begin/end is INVALID_CID, the chain ends, or next is an overwrite copy).
__device__ __forceinline__ uint32_t scan_visible(const DevTable &t, const SlotInfo &si, uint32_t rid, uint8_t &st) {
    if (rid >= meta_cstamp(si.meta)) {
        st = ST_LATEST;
        return si.image;
    }
    st = ST_NOT_FOUND;
    uint32_t chain = si.next;
    for (uint32_t guard = 0; guard < (1u << 24) && (chain & kNextKindMask) == kNextVersion; ++guard) {
        const VersionHdr v = t.vhdr[chain & kNextIndexMask];
        if (v.begin_id == kInvalidCid || v.comm_id == kInvalidCid) break;
        if (rid >= v.begin_id && rid <= v.comm_id) {
            st = ST_OLD;
            return v.image;
        }
        chain = v.next;
    }
    return 0xFFFFFFFFu;
}

// What a window scan launch carries beside the scan's arguments (wave-uniform).
struct ScanWindowArgs {
    WindowArgs w;       // w.win: n * scan_size windows, record j of scan i at i * scan_size + j
    uint8_t *row_keys;  // optional: n * scan_size keys of key_pad bytes
    uint32_t key_pad;   // key bytes at the head of a heap row (a multiple of 8)
};

// One leaf visit's e records, output positions pos0 .. pos0 + e - 1, their heap rows in rank
// order in the wave's LDS list rk (0xFFFFFFFF: the record yields no tuple, window and key are
// zero).  The e * W window pieces are consecutive in memory: chunks of 64 ranks go through
// store_windows (a 128-slot leaf emits up to 128 records in one visit).  The keys are written by
// one lane per rank, 64 * key_pad consecutive bytes, from the head of the heap row -- the bytes
// the row form copies.  Called by every lane of the wave, after the list's writes are fenced.
__device__ __forceinline__ void store_scan_windows(const DevTable &t, uint32_t lane, uint64_t pos0, uint32_t e,
                                                   const uint32_t *rk, const ScanWindowArgs &a) {
    for (uint32_t r0 = 0; r0 < e; r0 += 64u) {
        const uint32_t cnt = e - r0 < 64u ? e - r0 : 64u;
        const uint32_t img = lane < cnt ? rk[r0 + lane] : 0xFFFFFFFFu;
        store_windows(t, lane, pos0 + r0, (int)cnt, img, a.w);
        if (a.row_keys && lane < cnt) {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(t.heap + (uint64_t)img * t.hstride);
            uint64_t *dst = reinterpret_cast<uint64_t *>(a.row_keys + (pos0 + r0 + lane) * a.key_pad);
            for (uint32_t k = 0; k < (a.key_pad >> 3); ++k)
                __builtin_nontemporal_store(img != 0xFFFFFFFFu ? src[k] : 0ull, dst + k);
        }
    }
}

}  // namespace stage
