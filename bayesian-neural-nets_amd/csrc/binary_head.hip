// The binary (sigmoid) head and its fused BCE ELBO loss: the logistic-regression form of the latent-binary networks (one
// Bayesian layer, torch.sigmoid on its output, nn.BCELoss(reduction='sum') + kl / NUM_BATCHES).
//
//   lbbnn_binary_head              probs = 1 / (1 + exp(-x));  O == 1: logp2 = [logsigmoid(-x), logsigmoid(x)] from the LOGIT
//   lbbnn_elbo_bce_loss            loss = sum (y - 1) max(log1p(-p), -100) - y max(log p, -100) + kl * kl_scale, and counts
//   lbbnn_elbo_bce_loss_monitor    the same loss and counts (bitwise) plus the running totals of a training log and a per-step
//                                  non-finite flag, still one launch of one workgroup
//   lbbnn_elbo_bce_loss_backward   g_probs = g (p - y) / max((1 - p) p, 1e-12);  g_logits = g_probs ((1 - p) p);  g_kl = g kl_scale
//   lbbnn_sigmoid_backward         out = g ((1 - p) p)
// One pass each; the loss is one workgroup with fp64 partial sums in a fixed order (deterministic), no atomics.  The products and
// sums below are written without contraction into fused multiply-adds, so that g_logits of the fused loss backward and of
// lbbnn_sigmoid_backward applied to g_probs are the same bits.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "train_totals.h"

#pragma clang fp contract(off)

namespace {

using namespace lbbnn;

__device__ __forceinline__ bool target_ok(float y) { return y >= 0.f && y <= 1.f; }      // false for NaN

__global__ __launch_bounds__(256) void binary_head_kernel(const float* logits, int ldi, long long n, int O, float* probs, int ldp,
                                                          float* logp2, int ld2) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / O;
        const int o = (int)(i - b * O);
        const float x = logits[b * ldi + o];            // read before either store: probs may alias logits
        if (probs) probs[b * ldp + o] = sigmoid_ref(x);
        if (logp2) {                                    // O == 1 (checked by the entry point)
            const float t = log1pf(expf(-fabsf(x)));
            logp2[b * ld2] = fminf(-x, 0.f) - t;
            logp2[b * ld2 + 1] = fminf(x, 0.f) - t;
        }
    }
}

// The one pass of the BCE loss: element i of the (B, O) block goes to thread i % 1024, a thread adds its elements in rising i,
// block_sum<double, 16> adds the threads.  Every thread returns the four block totals (the counts are whole numbers < 2^53:
// exact in fp64).
struct BceSums { double s, n_ok, n_bad, n_nonfinite; };

__device__ __forceinline__ BceSums bce_sums(const float* __restrict__ probs, int ldp, const float* __restrict__ target, int ldt,
                                            long long n, int O, double* scratch) {
    double s = 0.0, n_ok = 0.0, n_bad = 0.0, n_nonfinite = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) {
        const long long b = i / O;
        const int o = (int)(i - b * O);
        const float p = probs[b * ldp + o], y = target[b * ldt + o];
        if (!isfinite(p)) n_nonfinite += 1.0;
        if (!target_ok(y)) { n_bad += 1.0; continue; }
        // torch's own spelling (binary_cross_entropy: log(1 - p) as log1p(-p), the two products in this order): p = 2e-9
        // against y = 0 costs 2e-9, not the 0 that logf(1.f - p) rounds to.  log1pf gives torch.log1p's bits; logf differs
        // from torch.log in the last bit for about a third of the probabilities (measured)
        const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
        s += (double)((y - 1.f) * lq - y * lp);
        if ((p > 0.5f) == (y > 0.5f)) n_ok += 1.0;
    }
    BceSums r;
    r.s = block_sum<double, 16>(s, scratch);
    r.n_ok = block_sum<double, 16>(n_ok, scratch);
    r.n_bad = block_sum<double, 16>(n_bad, scratch);
    r.n_nonfinite = block_sum<double, 16>(n_nonfinite, scratch);
    return r;
}

__device__ __forceinline__ void bce_stats(int* stats, int accumulate, const BceSums& r, long long n) {
    const int c[4] = {(int)r.n_ok, (int)n, (int)r.n_bad, (int)r.n_nonfinite};
    for (int k = 0; k < 4; ++k) stats[k] = (accumulate ? stats[k] : 0) + c[k];
}

// MONITOR: plus the training monitor (train_totals.h): the same pass, so *loss and stats are the plain kernel's
// bits.  The unit of account of the totals is one element (b, o): the four block totals of the pass are the counts of the step.
// The totals are loaded in the tail.
template <bool MONITOR>
__global__ __launch_bounds__(1024) void elbo_bce_loss_kernel(const float* __restrict__ probs, int ldp,
                                                             const float* __restrict__ target, int ldt, long long n, int O,
                                                             const float* kl, float kl_scale, float* loss, int* stats,
                                                             int accumulate, int64_t* totals, int32_t* guard) {
    __shared__ double scratch[16];
    const BceSums r = bce_sums(probs, ldp, target, ldt, n, O, scratch);
    if (threadIdx.x == 0) {
        [[maybe_unused]] MonitorWords pre;
        if constexpr (MONITOR) pre = monitor_preload(totals);
        const TrainStep st = {r.s, kl_term_of(kl, kl_scale), n, (int64_t)r.n_ok, (int64_t)r.n_bad, (int64_t)r.n_nonfinite};
        *loss = loss_of(st.nll, st.kl_term);
        if (stats) bce_stats(stats, accumulate, r, n);
        if constexpr (MONITOR) monitor_commit(totals, guard, pre, st);
    }
}

__global__ __launch_bounds__(256) void elbo_bce_loss_backward_kernel(const float* g, const float* __restrict__ probs, int ldp,
                                                                     const float* __restrict__ target, int ldt, long long n, int O,
                                                                     float kl_scale, float* g_probs, float* g_logits, float* g_kl) {
    const float gv = *g;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / O;
        const int o = (int)(i - b * O);
        const float p = probs[b * ldp + o], y = target[b * ldt + o];
        const float d = (1.f - p) * p;
        const float gp = target_ok(y) ? gv * (p - y) / fmaxf(d, 1e-12f) : 0.f;
        g_probs[i] = gp;
        if (g_logits) g_logits[i] = target_ok(y) ? gp * d : 0.f;
    }
    store_g_kl(g_kl, gv, kl_scale);
}

__global__ __launch_bounds__(256) void sigmoid_backward_kernel(const float* g, int ldg, const float* probs, int ldp, float* out,
                                                               int ldo, long long n, int O) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / O;
        const int o = (int)(i - b * O);
        const float p = probs[b * ldp + o];
        out[b * ldo + o] = g[b * ldg + o] * ((1.f - p) * p);
    }
}

}  // namespace

extern "C" int lbbnn_binary_head(const float* logits, int ldi, int B, int O, float* probs, int ldp, float* logp2, int ld2,
                                 void* stream) {
    if (!logits || (!probs && !logp2)) return LBBNN_E_NULL;
    if (bad_shape(B, O) || ldi < O || (probs && ldp < O)) return LBBNN_E_SHAPE;
    if (logp2 && (O != 1 || ld2 < 2)) return LBBNN_E_SHAPE;
    if (off(logits, 4) || off(probs, 4) || off(logp2, 4)) return LBBNN_E_ALIGN;
    if (B == 0) return 0;
    const long long n = (long long)B * O;
    hipLaunchKernelGGL(binary_head_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), logits, ldi, n, O,
                       probs, ldp, logp2, ld2);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_elbo_bce_loss(const float* probs, int ldp, const float* target, int ldt, int B, int O, const float* kl,
                                   float kl_scale, float* loss, int* stats, int accumulate, void* stream) {
    if (!probs || !target || !loss) return LBBNN_E_NULL;
    if (bad_shape(B, O) || ldp < O || ldt < O) return LBBNN_E_SHAPE;
    if (off(probs, 4) || off(target, 4) || off(kl, 4) || off(loss, 4) || off(stats, 4)) return LBBNN_E_ALIGN;
    hipLaunchKernelGGL(elbo_bce_loss_kernel<false>, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), probs, ldp, target,
                       ldt, (long long)B * O, O, kl, kl_scale, loss, stats, accumulate, (int64_t*)nullptr, (int32_t*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_elbo_bce_loss_monitor(const float* probs, int ldp, const float* target, int ldt, int B, int O, const float* kl,
                                           float kl_scale, float* loss, int* stats, int accumulate, int64_t* totals,
                                           int32_t* guard, void* stream) {
    if (!probs || !target || !loss || !totals) return LBBNN_E_NULL;
    if (bad_shape(B, O) || B < 1 || ldp < O || ldt < O) return LBBNN_E_SHAPE;
    if (off(probs, 4) || off(target, 4) || off(kl, 4) || off(loss, 4) || off(stats, 4) || off(guard, 4) || off(totals, 8))
        return LBBNN_E_ALIGN;
    hipLaunchKernelGGL(elbo_bce_loss_kernel<true>, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), probs, ldp, target,
                       ldt, (long long)B * O, O, kl, kl_scale, loss, stats, accumulate, totals, guard);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_elbo_bce_loss_backward(const float* g, const float* probs, int ldp, const float* target, int ldt, int B, int O,
                                            float kl_scale, float* g_probs, float* g_logits, float* g_kl, void* stream) {
    if (!g || !probs || !target || !g_probs) return LBBNN_E_NULL;
    if (bad_shape(B, O) || ldp < O || ldt < O) return LBBNN_E_SHAPE;
    if (off(g, 4) || off(probs, 4) || off(target, 4) || off(g_probs, 4) || off(g_logits, 4) || off(g_kl, 4)) return LBBNN_E_ALIGN;
    const long long n = (long long)B * O;
    // (an empty batch still writes g_kl: one workgroup whose loop runs zero times)
    hipLaunchKernelGGL(elbo_bce_loss_backward_kernel, dim3(n ? grid_for(n) : 1), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       probs, ldp, target, ldt, n, O, kl_scale, g_probs, g_logits, g_kl);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_sigmoid_backward(const float* g, int ldg, const float* probs, int ldp, float* out, int ldo, int B, int O,
                                      void* stream) {
    if (!g || !probs || !out) return LBBNN_E_NULL;
    if (bad_shape(B, O) || ldg < O || ldp < O || ldo < O) return LBBNN_E_SHAPE;
    if (off(g, 4) || off(probs, 4) || off(out, 4)) return LBBNN_E_ALIGN;
    if (B == 0) return 0;
    const long long n = (long long)B * O;
    hipLaunchKernelGGL(sigmoid_backward_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), g, ldg, probs,
                       ldp, out, ldo, n, O);
    return (int)hipGetLastError();
}
