// tuple_read.hpp -- what the transaction kernels (tpcc.hip, chq2.hip) ask of a probe's answer:
// whether it produced a tuple, and a little-endian column of its heap row at any alignment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "stage_core.hpp"

namespace stage {

__device__ __forceinline__ bool produced_tuple(uint32_t st) {
    return st == ST_LATEST || st == ST_COPY || st == ST_OLD;
}

__device__ __forceinline__ int32_t ld_i32(const uint8_t *p) {
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

}  // namespace stage
