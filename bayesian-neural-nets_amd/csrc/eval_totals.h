// The running totals of the evaluation kernels (eval_metrics.hip, eval_uncertainty.hip, eval_regression.hip, eval_scores.hip),
// written once; DESIGN.md, "Evaluation totals", has the scheme and why the bits repeat.  Integer totals: counted per workgroup
// (flags by ballot, bins by LDS atomics), added to the caller's with 64-bit integer atomics, zeros skipped.  Double sums: thread
// j adds column j of the workgroup's slots in slot order and leaves the partial at work[j * nblk + workgroup]; ONE second
// launch adds every column's partials in a fixed order.  Also the argument checks the four entry points share.
#pragma once
#include <initializer_list>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"

namespace lbbnn {

constexpr int kEvalThreads = 256;          // the workgroup of all four kernels and of the sums launch

// THE bin rule: clamp((int)(v * scale), 0, n - 1).  The product is clamped to [0, n] as a float first (a NaN or an overflowed
// product cannot reach the conversion: fmaxf returns its other operand for a NaN), the integer afterwards.
__device__ __forceinline__ int bin_of(float v, float scale, int n) {
    const float p = fminf(fmaxf(v * scale, 0.f), (float)n);
    return min(max((int)p, 0), n - 1);
}

// cnt[k] += the wave's lanes with flags[k]: one ballot and at most one atomic per flag.  cnt is the workgroup's LDS counters
// (unsigned), or the caller's totals themselves where one wave holds the whole workgroup's elements (unsigned long long).
template <int N, class T>
__device__ __forceinline__ void count_flags(const bool (&flags)[N], T* cnt) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const unsigned long long bal = __ballot(flags[k]);
        if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&cnt[k], (T)__popcll(bal));
    }
}

// dst[i] += lds[i], i < n, by the whole workgroup: one 64-bit integer atomic per non-zero counter.
__device__ __forceinline__ void flush_counters(const unsigned* lds, int n, unsigned long long* dst) {
    for (int i = threadIdx.x; i < n; i += kEvalThreads) {
        const unsigned c = lds[i];
        if (c) atomicAdd(&dst[i], (unsigned long long)c);
    }
}

// Column j of the workgroup's N slots, added in slot order, in double: slot i enters when its flags hold every bit of `need`
// and, for mb >= 0, when bin[i] == mb.  The partial goes to partials[j * nblk + workgroup].
template <int N>
__device__ __forceinline__ void column_partial(int j, const float* col, const int* flag, int need, double* partials, long long nblk,
                                               const int* bin = nullptr, int mb = -1) {
    double s = 0.0;
    for (int i = 0; i < N; ++i)
        if ((flag[i] & need) == need && (mb < 0 || bin[i] == mb)) s += (double)col[i];
    partials[(size_t)j * (size_t)nblk + blockIdx.x] = s;
}

// The second launch: dst(j) += the workgroups' partials of column j, where dst(j) is dst0 + j for j < split and
// dst1 + (j - split) after.  Wave w takes the columns j = w, w + 4, ...; lane l adds partials l, l + 64, ... in ascending
// order, then the fixed wave butterfly.
static __global__ __launch_bounds__(kEvalThreads) void eval_column_sums_kernel(const double* __restrict__ partials, long long nblk,
                                                                              int ncols, int split, double* dst0, double* dst1) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = w; j < ncols; j += kEvalThreads / 64) {
        double s = 0.0;
        for (long long i = lane; i < nblk; i += 64) s += partials[(size_t)j * (size_t)nblk + i];
        s = wave_sum(s);
        if (lane == 0) {
            double* dst = j < split ? dst0 + j : dst1 + (j - split);
            *dst += s;
        }
    }
}

inline int launch_column_sums(const void* work, long long nblk, int ncols, double* dst0, hipStream_t s, int split = 0x7FFFFFFF,
                              double* dst1 = nullptr) {
    hipLaunchKernelGGL(eval_column_sums_kernel, dim3(1), dim3(kEvalThreads), 0, s, (const double*)work, nblk, ncols, split, dst0, dst1);
    return (int)hipGetLastError();
}

// The running totals come all (with `work`) or none: 1, 0, or -1 when only some are there.
inline int totals_given(std::initializer_list<const void*> totals, const void* work) {
    bool any = false, all = work != nullptr;
    for (const void* p : totals) {
        any = any || p;
        all = all && p;
    }
    return !any ? 0 : all ? 1 : -1;
}

// The (S, B, W) member block: S members of B rows of W values, rows ldp apart, members m_stride apart and not overlapping.
inline int check_member_block(int S, int max_S, int B, int W, int max_W, int64_t ldp, int64_t m_stride) {
    if (S < 1 || S > max_S || W < 1 || W > max_W || B < 0) return LBBNN_E_SHAPE;
    if (ldp < W) return LBBNN_E_SHAPE;
    if (S > 1 && B > 0 && m_stride < (int64_t)(B - 1) * ldp + W) return LBBNN_E_SHAPE;
    return 0;
}

}  // namespace lbbnn
