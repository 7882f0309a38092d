// The count / pack of every sparse median-probability model (sparse_members.hip, base_sparse.hip): ONE kernel template over a
// keep rule, see include/lbbnn.h.
//
//   csr_rows_kernel<Rule, kMaxLevels, kPack>: one launch over the rows of up to LBBNN_MAX_LAYERS layers, ONE WAVE PER ROW (four
//     rows per 256-thread workgroup).  The wave walks its row 64 columns at a time: a lane loads one lambdal (a 256-B line per
//     wave) ONCE and compares it with the K <= kMaxLevels ascending cuts (kernel arguments: scalar registers).  The ballot of
//     level j is that level's kept set of the 64 columns, and a kept lane's place is the running count of (level, row) plus the
//     number of kept lanes below it (mbcnt of the ballot) -- ascending columns without a sort, an atomic or LDS.  Pack: a lane
//     kept at level 0 (the loosest cut: every other level's kept set lies inside it) loads mu / rho once and stores col / mean /
//     the rule's third value into the segment of every level that keeps it; lane 0 does the rule's per-row store.  Count: lane
//     0 stores the totals of the row.  The unrolled level loop keeps run / base / end in registers (constant indices); levels
//     past K do nothing, and kMaxLevels = 1 (a single threshold) is the loop's body once, with K a constant.
//   Rule: the three expressions in which the models differ --
//     LrtRule (frozen LRT / MNF network): lambdal > logit(threshold); var = k1_sigma(rho)^2 and bias_var = softplus_ref(bias_rho)^2,
//       the arithmetic of frozen_operands_kernel, so the values are its bits;
//     BaseRule (baseline network): the keep rule of base_frozen_operands_kernel, sigmoid_ref(lambdal) > threshold in fp32 -- not
//       lambdal > logit(threshold), which can differ at the boundary; sigma = softplus_ref(rho) itself (the draw multiplies by
//       sigma: sqrt(sigma^2) is not sigma to the bit), and per row b_mu / b_sigma.
// No LDS, no atomics, plain vector stores; every index read from row_ptr is clamped into [0, nnz] before it is followed.
#pragma once
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "operand_store.h"
#include "sparse_lanes.h"

namespace lbbnn {

constexpr int kCsrRows = 4;                // weight rows (= waves) per workgroup
constexpr int kCsrNT = 64 * kCsrRows;

// What an entry point copies its descriptor into.  val: the third array (var | sigma); row0 / row1: what lane 0 stores per row
// (bias_var | b_mu, b_sigma).  K = 0: the entry point found its levels or cuts out of range.
template <int kMaxLevels>
struct CsrLayer {
    const float* mu; const float* rho; const float* lambdal; const float* bias_mu; const float* bias_rho;
    const int32_t* row_ptr; int32_t* col; float* mean; float* val; float* row0; float* row1; int32_t* kept_rows;
    int O, I, nnz, K;
    float cut[kMaxLevels];
};
template <int kMaxLevels>
struct CsrBatch { CsrLayer<kMaxLevels> l[LBBNN_MAX_LAYERS]; int wg_end[LBBNN_MAX_LAYERS]; int n; };

struct LrtRule {
    static __device__ __forceinline__ bool keep(float lambdal, float cut) { return lambdal > cut; }   // fp32 compare: NaN is never kept
    static __device__ __forceinline__ float value(float rho) { const float sigma = k1_sigma(rho); return sigma * sigma; }
    template <typename L> static __device__ __forceinline__ void store_row(const L& a, int o) {
        const float sb = softplus_ref(a.bias_rho[o]);
        a.row0[o] = sb * sb;                          // bias.sigma**2, LBBNN-GP-MF-LRT.py:173 (never gated)
    }
    template <typename L> static bool row_null(const L& a) { return !a.bias_rho || !a.row0; }
};

struct BaseRule {
    static __device__ __forceinline__ bool keep(float lambdal, float thr) { return sigmoid_ref(lambdal) > thr; }   // fp32; NaN is never kept
    static __device__ __forceinline__ float value(float rho) { return softplus_ref(rho); }
    template <typename L> static __device__ __forceinline__ void store_row(const L& a, int o) {
        a.row0[o] = a.bias_mu[o];
        a.row1[o] = softplus_ref(a.bias_rho[o]);      // (never gated)
    }
    template <typename L> static bool row_null(const L& a) { return !a.bias_mu || !a.bias_rho || !a.row0 || !a.row1; }
};

template <typename Rule, int kMaxLevels, bool kPack>
static __global__ __launch_bounds__(kCsrNT) void csr_rows_kernel(const CsrBatch<kMaxLevels> bt_) {
    const LBBNN_CONST_AS CsrBatch<kMaxLevels>* bt = kernarg_as<CsrBatch<kMaxLevels>>();
    int wg0;
    const int li = layer_of(bt, wg0);
    const LBBNN_CONST_AS CsrLayer<kMaxLevels>& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kCsrRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;                                                 // (whole waves leave: no barrier below)
    const int I = a.I, K = kMaxLevels == 1 ? 1 : a.K;
    const size_t rowoff = (size_t)o * I;
    int run[kMaxLevels], base[kMaxLevels], end[kMaxLevels];               // run: kept so far in (level, row), wave-uniform
#pragma unroll
    for (int j = 0; j < kMaxLevels; ++j) {
        run[j] = base[j] = end[j] = 0;
        if (kPack && j < K) {
            // the slots of (level j, row o), inside [0, nnz] whatever row_ptr holds
            base[j] = clampi(a.row_ptr[(size_t)j * a.O + o], 0, a.nnz);
            end[j] = clampi(a.row_ptr[(size_t)j * a.O + o + 1], base[j], a.nnz);
        }
    }
    for (int c0 = 0; c0 < I; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < I;
        const float lam = in ? a.lambdal[rowoff + c] : 0.f;
        float mu = 0.f, val = 0.f;
        const auto level = [&](int j) {
            const bool kept = in && Rule::keep(lam, a.cut[j]);
            const unsigned long long m = __ballot(kept);
            if constexpr (kPack) {
                const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                const int pos = base[j] + run[j] + below;
                const bool store = kept && pos < end[j];
                if (j == 0 && kept) {                                     // once: every other level's kept set lies inside level 0's
                    mu = a.mu[rowoff + c];
                    val = Rule::value(a.rho[rowoff + c]);
                }
                if (store) {
                    a.col[pos] = c;
                    a.mean[pos] = mu;
                    a.val[pos] = val;
                }
            }
            run[j] += __popcll(m);
        };
        if constexpr (kMaxLevels == 1) {
            level(0);                                                     // (no loop to unroll: fewer registers than a loop of one)
        } else {
#pragma unroll
            for (int j = 0; j < kMaxLevels; ++j) if (j < K) level(j);     // wave-uniform
        }
    }
    if (lane == 0) {
        if constexpr (kPack) {
            Rule::store_row(a, o);
        } else {
#pragma unroll
            for (int j = 0; j < kMaxLevels; ++j) if (j < K) a.kept_rows[(size_t)j * a.O + o] = run[j];
        }
    }
}

// Every count / pack entry point: `copy(descriptor, layer)` fills the layer from the entry point's descriptor; `args` is the
// code of the entry point's own arguments, returned after the checks of `L` and `n`.  Per layer NULL, then SHAPE, then ALIGN.
template <typename Rule, int kMaxLevels, typename Desc, typename Copy>
int csr_rows(const Desc* L, int n, bool pack, int args, void* stream, Copy copy) {
    if (!L) return LBBNN_E_NULL;
    if (n <= 0 || n > LBBNN_MAX_LAYERS) return LBBNN_E_SHAPE;
    if (args) return args;
    CsrBatch<kMaxLevels> bt = {};
    int wgs = 0;
    for (int i = 0; i < n; ++i) {
        CsrLayer<kMaxLevels>& a = bt.l[i];
        copy(L[i], a);
        if (!a.lambdal) return LBBNN_E_NULL;
        if (pack) {
            if (!a.mu || !a.rho || !a.row_ptr || Rule::row_null(a)) return LBBNN_E_NULL;
            if (a.nnz > 0 && (!a.col || !a.mean || !a.val)) return LBBNN_E_NULL;
        } else if (!a.kept_rows) return LBBNN_E_NULL;
        if (a.O <= 0 || a.I <= 0 || (pack && a.nnz < 0) || a.K < 1) return LBBNN_E_SHAPE;
        if (!aligned4(a.lambdal)) return LBBNN_E_ALIGN;
        if (pack) {
            if (!aligned4(a.mu) || !aligned4(a.rho) || !aligned4(a.bias_mu) || !aligned4(a.bias_rho) || !aligned4(a.row_ptr) ||
                !aligned4(a.col) || !aligned4(a.mean) || !aligned4(a.val) || !aligned4(a.row0) || !aligned4(a.row1))
                return LBBNN_E_ALIGN;
        } else if (!aligned4(a.kept_rows)) return LBBNN_E_ALIGN;
        if (!pack) a.nnz = 0;
        wgs += (a.O + kCsrRows - 1) / kCsrRows;
        bt.wg_end[i] = wgs;
    }
    bt.n = n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (pack) hipLaunchKernelGGL((csr_rows_kernel<Rule, kMaxLevels, true>), dim3(wgs), dim3(kCsrNT), 0, s, bt);
    else hipLaunchKernelGGL((csr_rows_kernel<Rule, kMaxLevels, false>), dim3(wgs), dim3(kCsrNT), 0, s, bt);
    return (int)hipGetLastError();
}

}  // namespace lbbnn
