// The summation order of deterministic mode (include/maestro_hip.h): shared by mh_reduce_ordered (reduce_det.hip) and the
// entry points that finish a reduction of their own in that order (embed.hip).
#pragma once
#include "common.hpp"
#include "../../include/maestro_hip.h"

// job_total of one column: `src` points at the column's element of row 0.  The chunk's MH_ORDERED_ROWS loads go out together, the
// adds keep their order.  Rows beyond the end are added as +0, which changes no bit: a running sum that started from +0 is
// never -0.
__device__ __forceinline__ float ordered_job_total(const float* __restrict__ src, int rows, size_t ld) {
    float total = 0.f;
    for (int r0 = 0; r0 < rows; r0 += MH_ORDERED_ROWS) {
        float v[MH_ORDERED_ROWS];
#pragma unroll
        for (int i = 0; i < MH_ORDERED_ROWS; ++i) v[i] = r0 + i < rows ? src[(size_t)(r0 + i) * ld] : 0.f;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MH_ORDERED_ROWS; ++i) s += v[i];
        total += s;
    }
    return total;
}
