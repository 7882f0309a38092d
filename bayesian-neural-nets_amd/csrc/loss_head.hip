// The scalar head of the training step, fused (round 3; VERDICT r02 item 7: torch-native nll_loss / softmax / add / mul
// kernels inside the captured step -- ~45 us of a 0.84 ms step, nll_loss_forward alone 13 us for 4096 x 10 values).
//
//   lbbnn_elbo_loss           loss = -sum_b logp[b][t_b] + kl * kl_scale            F.nll_loss(reduction='sum') + kl / NUM_BATCHES,
//                                                                                  LBBNN-GP-MF-MNF.py:268-271 (train())
//   lbbnn_elbo_loss_monitor   the same loss (bitwise) plus the running totals of a training log and a per-step non-finite flag,
//                             still one launch of one workgroup
//   lbbnn_elbo_loss_backward  g_logp[b][c] = -g (c == t_b),  *g_kl = g * kl_scale
//   lbbnn_log_softmax_backward g_logits = g_logp - exp(logp) * sum_c g_logp         backward of F.log_softmax(dim=1), :256
// One workgroup / one pass each; sums in a fixed order (deterministic).
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "train_totals.h"

namespace {

using namespace lbbnn;

__global__ __launch_bounds__(1024) void elbo_loss_kernel(const float* __restrict__ logp, int ldp, const int64_t* __restrict__ target,
                                                         int B, int C, const float* kl, float kl_scale, float* loss) {
    __shared__ double scratch[16];
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += 1024) {
        const int64_t t = target[b];
        if (t >= 0 && t < C) s -= (double)logp[(size_t)b * ldp + t];
    }
    s = block_sum<double, 16>(s, scratch);
    if (threadIdx.x == 0) *loss = loss_of(s, kl_term_of(kl, kl_scale));
}

// elbo_loss_kernel plus the training monitor.  The nll sum is elbo_loss_kernel's, term for term (same rows per thread, same
// order, same block_sum), so *loss has its bits.  A thread reads its row's C log-probabilities in batches of 16 independent
// loads (the target's term is picked out of the registers instead of being loaded behind the target), finds the arg-max by
// numpy.argmax's rule (a NaN is the maximum, the lowest index wins a tie) and whether all C values are finite.  The three row
// counts are wave sums left in LDS ahead of block_sum's barriers.  The unit of account of the totals is one row; they are
// loaded in the tail (train_totals.h).
__global__ __launch_bounds__(1024) void elbo_loss_monitor_kernel(const float* __restrict__ logp, int ldp,
                                                                 const int64_t* __restrict__ target, int B, int C, const float* kl,
                                                                 float kl_scale, float* loss, int64_t* totals, int32_t* guard) {
    constexpr int G = 16;
    __shared__ double scratch[16];
    __shared__ int counts[3][16];
    double s = 0.0;
    int n_correct = 0, n_bad = 0, n_nonfinite = 0;                // B < 2^31 rows: every count fits
    int64_t t_next = (int)threadIdx.x < B ? target[threadIdx.x] : 0;
    for (int b = threadIdx.x; b < B; b += 1024) {
        const int64_t t = t_next;
        if (b + 1024 < B) t_next = target[b + 1024];             // the next row's target rides with this row's loads
        const float* __restrict__ row = logp + (size_t)b * ldp;
        const bool valid = t >= 0 && t < C;
        const int tc = valid ? (int)t : -1;
        float best = -INFINITY, term = 0.f;
        int arg = 0;
        bool finite = true;
        for (int c0 = 0; c0 < C; c0 += G) {
            float v[G];
#pragma unroll
            for (int j = 0; j < G; ++j) v[j] = c0 + j < C ? row[c0 + j] : 0.f;
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int c = c0 + j;
                if (c < C) {
                    finite = finite && isfinite(v[j]);
                    if (c == tc) term = v[j];
                    if (best == best && (v[j] > best || v[j] != v[j])) { best = v[j]; arg = c; }
                }
            }
        }
        if (valid) s -= (double)term;
        if (!valid) ++n_bad;
        else if (arg == tc) ++n_correct;
        if (!finite) ++n_nonfinite;
    }
    n_correct = wave_sum(n_correct);
    n_bad = wave_sum(n_bad);
    n_nonfinite = wave_sum(n_nonfinite);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        counts[0][w] = n_correct; counts[1][w] = n_bad; counts[2][w] = n_nonfinite;
    }
    s = block_sum<double, 16>(s, scratch);                        // (its barriers also publish `counts`)
    if (threadIdx.x == 0) {
        int tot[3] = {0, 0, 0};
        for (int q = 0; q < 3; ++q)
            for (int w = 0; w < 16; ++w) tot[q] += counts[q][w];
        const MonitorWords pre = monitor_preload(totals);
        const TrainStep st = {s, kl_term_of(kl, kl_scale), B, tot[0], tot[1], tot[2]};
        *loss = loss_of(st.nll, st.kl_term);
        monitor_commit(totals, guard, pre, st);
    }
}

__global__ __launch_bounds__(256) void elbo_loss_backward_kernel(const float* g, const int64_t* __restrict__ target, int B, int C,
                                                                 float kl_scale, float* g_logp, float* g_kl) {
    const float gv = *g;
    const int n = B * C;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int b = i / C, c = i - b * C;
        g_logp[i] = (target[b] == c) ? -gv : 0.f;
    }
    store_g_kl(g_kl, gv, kl_scale);
}

// ... and, in the same launch, what lbbnn_log_softmax_backward makes of that gradient when the log-probabilities are the
// log_softmax of a layer's logits (the fused head of the training forward): g_logits = g_logp - exp(logp) * sum_c g_logp, with
// the row sum being -g exactly -- or zero for a row whose target lies outside [0, C), which has no one-hot entry and gets no
// gradient.  Same expression, same order: bitwise the two-launch result.
__global__ __launch_bounds__(256) void elbo_loss_backward_logits_kernel(const float* g, const int64_t* __restrict__ target,
                                                                        const float* __restrict__ logp, int ldp, int B, int C,
                                                                        float kl_scale, float* g_logp, float* g_logits, float* g_kl) {
    const float gv = *g;
    const int n = B * C;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int b = i / C, c = i - b * C;
        const int64_t t = target[b];
        const float gl = (t == c) ? -gv : 0.f;
        const float s = (t >= 0 && t < C) ? -gv : 0.f;
        g_logp[i] = gl;
        g_logits[i] = gl - expf(logp[(size_t)b * ldp + c]) * s;
    }
    store_g_kl(g_kl, gv, kl_scale);
}

// thread per row (C <= 64)
__global__ __launch_bounds__(256) void log_softmax_backward_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ logp,
                                                                   int ldp, float* out, int ldo, int B, int C) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += g[(size_t)b * ldg + c];
    for (int c = 0; c < C; ++c) out[(size_t)b * ldo + c] = g[(size_t)b * ldg + c] - expf(logp[(size_t)b * ldp + c]) * s;
}

}  // namespace

extern "C" int lbbnn_elbo_loss(const float* logp, int ldp, const int64_t* target, int B, int C, const float* kl, float kl_scale,
                               float* loss, void* stream) {
    if (!logp || !target || !loss) return LBBNN_E_NULL;
    if (B <= 0 || C <= 0 || ldp < C) return LBBNN_E_SHAPE;
    hipLaunchKernelGGL(elbo_loss_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), logp, ldp, target, B, C, kl,
                       kl_scale, loss);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_elbo_loss_monitor(const float* logp, int ldp, const int64_t* target, int B, int C, const float* kl,
                                       float kl_scale, float* loss, int64_t* totals, int32_t* guard, void* stream) {
    if (!logp || !target || !loss || !totals) return LBBNN_E_NULL;
    if (B <= 0 || C <= 0 || C > 64 || ldp < C) return LBBNN_E_SHAPE;
    hipLaunchKernelGGL(elbo_loss_monitor_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), logp, ldp, target, B, C,
                       kl, kl_scale, loss, totals, guard);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_elbo_loss_backward(const float* g, const int64_t* target, int B, int C, float kl_scale, float* g_logp,
                                        float* g_kl, void* stream) {
    if (!g || !target || !g_logp) return LBBNN_E_NULL;
    if (B <= 0 || C <= 0) return LBBNN_E_SHAPE;
    const int blocks = (B * C + 255) / 256 < 512 ? (B * C + 255) / 256 : 512;
    hipLaunchKernelGGL(elbo_loss_backward_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), g, target, B, C,
                       kl_scale, g_logp, g_kl);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_elbo_loss_backward_logits(const float* g, const int64_t* target, const float* logp, int ldp, int B, int C,
                                               float kl_scale, float* g_logp, float* g_logits, float* g_kl, void* stream) {
    if (!g || !target || !logp || !g_logp || !g_logits) return LBBNN_E_NULL;
    if (B <= 0 || C <= 0 || ldp < C) return LBBNN_E_SHAPE;
    const int blocks = (B * C + 255) / 256 < 512 ? (B * C + 255) / 256 : 512;
    hipLaunchKernelGGL(elbo_loss_backward_logits_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), g, target,
                       logp, ldp, B, C, kl_scale, g_logp, g_logits, g_kl);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_log_softmax_backward(const float* g, int ldg, const float* logp, int ldp, float* out, int ldo, int B, int C,
                                          void* stream) {
    if (!g || !logp || !out) return LBBNN_E_NULL;
    if (B <= 0 || C <= 0 || C > 64 || ldg < C || ldp < C || ldo < C) return LBBNN_E_SHAPE;
    hipLaunchKernelGGL(log_softmax_backward_kernel, dim3((B + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), g, ldg,
                       logp, ldp, out, ldo, B, C);
    return (int)hipGetLastError();
}
