// tree_search.hpp -- key order and the separator-tree descent of the probe and scan kernels:
//   * leaf resolve: lane-per-probe descent of the implicit separator tree (16-entry 128-B
//     inner nodes, 8-entry 64-B bottom nodes), replaces InternalNode::GetChildIndex
//     (b_tree.cpp:664-702) / BTree::TraverseToLeaf (b_tree.cpp:1804-1846).
#pragma once
#include "visibility.hpp"
#include "wave.hpp"

namespace stage {
__device__ __forceinline__ bool kv_lt(uint64_t ao, uint32_t al, uint64_t bo, uint32_t bl) {
    return ao < bo || (ao == bo && al < bl);
}
__device__ __forceinline__ uint64_t head_vis(const DevTable &t, uint32_t leaf, int s) {
    return *reinterpret_cast<const uint64_t *>(t.head + (uint64_t)leaf * t.head_bytes + t.cap + 8 * s);
}

// branch-free lexicographic a < b (for several compares in flight in one lane)
template <int KW>
__device__ __forceinline__ bool kw_lt_flat(const uint64_t *a, const uint64_t *b) {
    bool lt = false, eq = true;
#pragma unroll
    for (int j = 0; j < KW; ++j) {
        lt = lt | (eq & (a[j] < b[j]));
        eq = eq & (a[j] == b[j]);
    }
    return lt;
}

// multi-word order keys (fixed-width keys of 9..32 bytes): lexicographic word order.  Written
// as selects from the last word to the first rather than early returns: per-lane early exits
// become exec-mask branches and lane-mask logic on the CU's one scalar pipe, which the
// first-tuple scans saturate; selects stay on the SIMD's vector pipe
template <int KW>
__device__ __forceinline__ bool kw_lt(const uint64_t *a, const uint64_t *b) {
    uint32_t r = 0;
#pragma unroll
    for (int j = KW - 1; j >= 0; --j) r = a[j] < b[j] ? 1u : (a[j] != b[j] ? 0u : r);
    return r != 0;
}

// separators of one node (F entries) below x.  KW = 1: the node is F x 8 B (F/2 16-B loads
// per lane); KW > 1: F entries of KW words each, compared lexicographically.
template <bool VARLEN, int KW, int F>
__device__ __forceinline__ uint32_t node_count_below(const DevTable &t, uint64_t off, const uint64_t *x, uint32_t xl) {
    uint32_t cnt = 0;
    if (KW > 1) {
        const uint64_t *e = t.tree + off * KW;
#pragma unroll
        for (int k = 0; k < F; ++k) {
            uint64_t w[KW];
#pragma unroll
            for (int j = 0; j < KW; ++j) w[j] = e[k * KW + j];
            cnt += kw_lt<KW>(w, x) ? 1u : 0u;
        }
        return cnt;
    }
    const u32x4 *e = reinterpret_cast<const u32x4 *>(t.tree + off);
    u32x4 q[F / 2];
#pragma unroll
    for (int k = 0; k < F / 2; ++k) q[k] = e[k];
    if (VARLEN) {
        const uint64_t *lp = reinterpret_cast<const uint64_t *>(t.tree_len + off);
        uint64_t lw[F / 8];
#pragma unroll
        for (int k = 0; k < F / 8; ++k) lw[k] = lp[k];
#pragma unroll
        for (int k = 0; k < F / 2; ++k) {
            const uint64_t l = lw[k / 4];
            const int sh = 16 * (k & 3);
            const uint64_t v0 = ((uint64_t)q[k].y << 32) | q[k].x, v1 = ((uint64_t)q[k].w << 32) | q[k].z;
            cnt += kv_lt(v0, (uint32_t)((l >> sh) & 0xFF), x[0], xl) ? 1u : 0u;
            cnt += kv_lt(v1, (uint32_t)((l >> (sh + 8)) & 0xFF), x[0], xl) ? 1u : 0u;
        }
    } else {
#pragma unroll
        for (int k = 0; k < F / 2; ++k) {
            cnt += ((((uint64_t)q[k].y << 32) | q[k].x) < x[0]) ? 1u : 0u;
            cnt += ((((uint64_t)q[k].w << 32) | q[k].z) < x[0]) ? 1u : 0u;
        }
    }
    return cnt;
}

// lower_bound over the separators: number of separators < x, i.e. the leaf whose range
// (sep[i-1], sep[i]] holds x (le_child semantics).  Upper-bound callers pass succ(x).
// Inner levels are 16-entry nodes (one 128-B line for 8-B keys), the bottom level 8-entry
// nodes (one 64-B sector): the bottom node is the one the probe usually fetches from beyond L2.
template <bool VARLEN, int KW>
__device__ __forceinline__ uint32_t tree_lower_bound(const DevTable &t, const uint64_t *x, uint32_t xl) {
    static_assert(kTreeFanout == 16 && kLeafFanout == 8, "node loads sized for 16 / 8 entries");
    uint32_t node = 0;
    for (int lvl = (int)t.levels - 1; lvl > 0; --lvl)
        node = node * kTreeFanout +
               node_count_below<VARLEN, KW, kTreeFanout>(t, t.level_off[lvl] + (uint64_t)node * kTreeFanout, x, xl);
    node = node * kLeafFanout + node_count_below<VARLEN, KW, kLeafFanout>(t, t.level_off[0] + (uint64_t)node * kLeafFanout,
                                                                          x, xl);
    return node < t.nseps ? node : t.nseps;
}

template <bool VARLEN, int KW>
__device__ __forceinline__ uint32_t resolve_leaf(const DevTable &t, const uint64_t *okey, uint32_t len, bool le_child) {
    if (le_child) return tree_lower_bound<VARLEN, KW>(t, okey, len);
    if (VARLEN) return tree_lower_bound<VARLEN, KW>(t, okey, len + 1);  // (okey, len+1) = succ
    // fixed width: succ = the key plus one in its last word, with carry
    uint64_t s[KW];
    bool carry = true;
#pragma unroll
    for (int j = KW - 1; j >= 0; --j) {
        s[j] = okey[j] + (carry ? 1ull : 0ull);
        carry = carry && okey[j] == ~0ull;
    }
    if (carry) return t.nseps;
    return tree_lower_bound<VARLEN, KW>(t, s, len);
}

// Wave-cooperative descent for a wave-uniform key (range scans): per level, lane e < fanout loads
// separator e of the node and one ballot counts the separators below the key -- one load
// round per level instead of every lane reading the whole node.
template <bool VARLEN, int KW>
__device__ __forceinline__ uint32_t tree_lower_bound_uniform(const DevTable &t, const uint64_t *x, uint32_t xl,
                                                             uint32_t lane) {
    uint32_t node = 0;
    for (int lvl = (int)t.levels - 1; lvl >= 0; --lvl) {
        const uint32_t f = (uint32_t)tree_fanout(lvl);
        const uint64_t off = t.level_off[lvl] + (uint64_t)node * f;
        bool lt = false;
        if (lane < f) {
            uint64_t e[KW];
#pragma unroll
            for (int j = 0; j < KW; ++j) e[j] = t.tree[(off + lane) * KW + j];
            if (KW == 1) lt = VARLEN ? kv_lt(e[0], t.tree_len[off + lane], x[0], xl) : e[0] < x[0];
            else lt = kw_lt<KW>(e, x);
        }
        node = node * f + (uint32_t)__builtin_popcountll(ballot(lt));
    }
    return node < t.nseps ? node : t.nseps;
}

template <bool VARLEN, int KW>
__device__ __forceinline__ uint32_t resolve_leaf_uniform(const DevTable &t, const uint64_t *okey, uint32_t len,
                                                         bool le_child, uint32_t lane) {
    if (le_child) return tree_lower_bound_uniform<VARLEN, KW>(t, okey, len, lane);
    if (VARLEN) return tree_lower_bound_uniform<VARLEN, KW>(t, okey, len + 1, lane);
    uint64_t s[KW];
    bool carry = true;
#pragma unroll
    for (int j = KW - 1; j >= 0; --j) {
        s[j] = okey[j] + (carry ? 1ull : 0ull);
        carry = carry && okey[j] == ~0ull;
    }
    if (carry) return t.nseps;
    return tree_lower_bound_uniform<VARLEN, KW>(t, s, len, lane);
}

// Iterator continuation (le_child = false from the last popped key x) when x came from
// `leaf`: every key of a leaf lies in its separator range (sep[leaf-1], sep[leaf]], so the
// separators <= x are those left of `leaf` plus sep[leaf] itself when it equals x -- the
// upper-bound descent collapses to one load of sep[leaf] (+inf padding past the last leaf).
template <bool VARLEN, int KW>
__device__ __forceinline__ uint32_t next_leaf_after(const DevTable &t, uint32_t leaf, const uint64_t *x, uint32_t xl) {
    if (leaf >= t.nseps) return t.nseps;
    const uint64_t e = t.level_off[0] + leaf;
    uint64_t sep[KW];
#pragma unroll
    for (int w = 0; w < KW; ++w) sep[w] = t.tree[e * KW + w];
    bool x_lt_sep;
    if (KW == 1) x_lt_sep = VARLEN ? kv_lt(x[0], xl, sep[0], t.tree_len[e]) : x[0] < sep[0];
    else x_lt_sep = kw_lt<KW>(x, sep);
    return x_lt_sep ? leaf : leaf + 1;
}

// order words of a key passed as KW little-endian u64 words (fixed width) or one word
template <int KW>
__device__ __forceinline__ void load_okey(const uint64_t *keys, uint64_t i, bool valid, uint32_t len, uint64_t *okw) {
#pragma unroll
    for (int j = 0; j < KW; ++j) {
        const uint64_t le = valid ? keys[i * KW + j] : 0ull;
        okw[j] = KW == 1 ? order_key(le, len) : order_word(le, len, (uint32_t)j, key_order_unsigned(len));
    }
}

template <bool VARLEN, int KW>
__device__ __forceinline__ bool key_less(const uint64_t *a, uint32_t al, const uint64_t *b, uint32_t bl) {
    if (KW == 1) return kv_lt(a[0], al, b[0], bl);
    return kw_lt<KW>(a, b);  // fixed width: equal lengths
}

}  // namespace stage
