// lbbnn_fold_rows: out[r] = ((0 + v[r][0]) + v[r][1]) + ... + v[r][n - 1] in fp32, for `rows` short rows of one buffer.
//
// The log-probability totals of a baseline network deeper than three layers: every layer's lbbnn_gate_sample_draw writes its
// log_prior into slot [0][i] and its log_q into slot [1][i] of one [2][n] buffer, and ONE launch of this kernel forms both
// network totals -- the fp32 left fold in layer order that the chain of torch adds of a three-layer network forms.  One thread per
// row, plain loads and one plain vector store per row, no atomics, no LDS: the same bits from run to run, capturable.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(64) void fold_rows_kernel(const float* __restrict__ v, int rows, int n, int ld, float* __restrict__ out) {
    const int r = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (r >= rows) return;
    const float* p = v + (size_t)r * (size_t)ld;
    float s = 0.f;
#pragma unroll 1
    for (int i = 0; i < n; ++i) s += p[i];                // fixed order: l1, l2, ..., lN
    out[r] = s;
}

}  // namespace

extern "C" int lbbnn_fold_rows(const float* v, int rows, int n, int ld, float* out, void* stream) {
    if (!v || !out) return LBBNN_E_NULL;
    if (rows < 1 || rows > LBBNN_FOLD_MAX_ROWS || n < 1 || n > LBBNN_FOLD_MAX_N || ld < n) return LBBNN_E_SHAPE;
    if (((uintptr_t)v | (uintptr_t)out) & 3u) return LBBNN_E_ALIGN;
    hipLaunchKernelGGL(fold_rows_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       v, rows, n, ld, out);
    return (int)hipGetLastError();
}
