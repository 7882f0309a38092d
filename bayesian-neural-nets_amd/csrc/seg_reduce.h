// Reductions over the G neighbouring lanes that hold one row's classes (eval_metrics.hip, eval_uncertainty.hip): G a power of
// two <= 64, rows aligned to G, every lane of the row ends with the result.
#pragma once
#include <type_traits>
#include "lbbnn_device.h"

namespace lbbnn {

template <int CTRL>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t b) {
    const uint32_t lo = (uint32_t)dpp_mov<CTRL>((int)(uint32_t)b), hi = (uint32_t)dpp_mov<CTRL>((int)(uint32_t)(b >> 32));
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t u64max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Sum / maximum over the G lanes of a row (G a power of two, rows aligned to G); every lane of the row ends with the result.
// Same DPP steps as wave_sum; rows wider than a DPP row of 16 lanes finish through the LDS crossbar.
template <int G>
__device__ __forceinline__ float seg_sum(float v) {
    if (G >= 2) v += dpp_get<0xB1>(v);
    if (G >= 4) v += dpp_get<0x4E>(v);
    if (G >= 8) v += dpp_get<0x141>(v);
    if (G >= 16) v += dpp_get<0x140>(v);
    if (G >= 32) v += __shfl_xor(v, 16);
    if (G >= 64) v += __shfl_xor(v, 32);
    return v;
}
template <int G>
__device__ __forceinline__ uint64_t seg_max(uint64_t v) {
    if (G >= 2) v = u64max(v, dpp_u64<0xB1>(v));
    if (G >= 4) v = u64max(v, dpp_u64<0x4E>(v));
    if (G >= 8) v = u64max(v, dpp_u64<0x141>(v));
    if (G >= 16) v = u64max(v, dpp_u64<0x140>(v));
    if (G >= 32) v = u64max(v, (uint64_t)__shfl_xor((unsigned long long)v, 16));
    if (G >= 64) v = u64max(v, (uint64_t)__shfl_xor((unsigned long long)v, 32));
    return v;
}

// numpy.argmax over the classes of a row: a NaN compares as the maximum, the lowest index of the maximum wins.  The value
// becomes a key that orders as the floats do (-0 = +0, every NaN on top), the index rides below it inverted; lanes past C
// carry 0, below every key of a real class.
template <int G>
__device__ __forceinline__ int seg_argmax(float x, int c, bool cok) {
    uint32_t bits = __builtin_bit_cast(uint32_t, x);
    if (x == 0.f) bits = 0u;
    const uint32_t key = (x != x) ? 0xFFFFFFFFu : ((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u));
    const uint64_t packed = cok ? (((uint64_t)key << 32) | (uint32_t)(63 - c)) : 0ull;
    return 63 - (int)(uint32_t)seg_max<G>(packed);
}

// Host side of the layout: G for C classes, the 256-thread workgroups B rows take, and the call of f with G as a constant.
inline int lanes_per_row(int C) {
    int G = 1;
    while (G < C) G <<= 1;
    return G;
}

inline long long row_workgroups(long long B, int C) {
    const long long rows = 256 / lanes_per_row(C);
    return (B + rows - 1) / rows;
}

template <class F>
void with_lanes_per_row(int C, F&& f) {
    switch (lanes_per_row(C)) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 8: f(std::integral_constant<int, 8>()); break;
        case 16: f(std::integral_constant<int, 16>()); break;
        case 32: f(std::integral_constant<int, 32>()); break;
        default: f(std::integral_constant<int, 64>()); break;
    }
}

}  // namespace lbbnn
