// launch_util.hpp -- grid sizing and the geometry dispatch shared by the kernel launchers.
#pragma once
#include <type_traits>
#include "stage_core.hpp"

namespace stage {
static int grid_for(uint64_t waves_needed, int waves_per_block, int max_blocks) {
    uint64_t b = (waves_needed + waves_per_block - 1) / waves_per_block;
    if (b < 1) b = 1;
    if (b > (uint64_t)max_blocks) b = (uint64_t)max_blocks;
    return (int)b;
}

// grid cap of the probe and scan launchers unless the tuning struct (ProbeTuning / ScanTuning) sets one
constexpr int kDefaultMaxBlocks = 16384;
template <class Tuning>
static int max_blocks(const Tuning &tune) { return tune.max_blocks > 0 ? tune.max_blocks : kDefaultMaxBlocks; }

// Geometry dispatch, the one place a table's run-time shape becomes template arguments:
// f(S) / f(KW) / f(S, KW) is called with std::integral_constant values, S = slot groups per leaf
// (cap / 64: 1, 2, 4, 8 or 16 -- HostTable admits no other capacity) and KW = order words per
// key (1, 2 or 4, table_key_words).  A launcher that has no kernel for part of the range
// guards it with `if constexpr`, so the lambda instantiates exactly the kernels it can launch.
template <int N>
using int_c = std::integral_constant<int, N>;
template <class F>
static void with_slot_groups(const DevTable &t, F &&f) {
    switch (t.cap / 64) {
        case 1: f(int_c<1>()); break;
        case 2: f(int_c<2>()); break;
        case 4: f(int_c<4>()); break;
        case 8: f(int_c<8>()); break;
        default: f(int_c<16>()); break;
    }
}
template <class F>
static void with_key_words(const DevTable &t, F &&f) {
    if (t.key_words == 4) f(int_c<4>());
    else if (t.key_words == 2) f(int_c<2>());
    else f(int_c<1>());
}
template <class F>
static void with_geometry(const DevTable &t, F &&f) {
    with_key_words(t, [&](auto KW) { with_slot_groups(t, [&](auto S) { f(S, KW); }); });
}

}  // namespace stage
