// The fused Gaussian ELBO loss of a regression network (head="identity": the last layer's raw output is the mean of a normal
// likelihood with log-variance lv), what F.gaussian_nll_loss(mean, y, exp(lv), full=True, reduction='sum') + kl / NUM_BATCHES is
// in torch ops.
//
//   lbbnn_elbo_gaussian_loss            loss = sum 0.5 (log(2 pi) + lv + (y - m)^2 exp(-lv)) + kl * kl_scale, the running error
//                                       sums, and with a shared lv its O column sums of d term / d lv
//   lbbnn_elbo_gaussian_loss_monitor    the same loss, sums and column sums (bitwise) plus the running totals of a training log and
//                                       a per-step non-finite flag, still one launch of one workgroup
//   lbbnn_elbo_gaussian_loss_backward   g_mean = g (m - y) exp(-lv);  g_lv = g 0.5 (1 - (y - m)^2 exp(-lv)) per element, or g times
//                                       the forward's column sums for a shared lv;  g_kl = g kl_scale
// Element (b, o), every operation a single fp32 one in this order (no contraction into fused multiply-adds):
//   d = y - m;  iv = expf(-lv);  q = (d * d) * iv;  term = 0.5f * ((log(2 pi) + lv) + q);  dlv = 0.5f * (1.f - q)
// with log(2 pi) = 1.8378770664093453 rounded to fp32.  The loss is one workgroup with fp64 partial sums in a fixed order
// (deterministic), no atomics.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "train_totals.h"

#pragma clang fp contract(off)

namespace {

using namespace lbbnn;

constexpr float kLog2Pi = 1.8378770664093453f;

__device__ __forceinline__ bool target_ok(float y) { return isfinite(y); }                // false for NaN, +inf, -inf

// The one pass of the loss.  The first T = (1024 / O) * O threads work, thread t on the elements t, t + T, t + 2 T, ... in
// rising order: all of them lie in column t % O, so a thread's sum of dlv belongs to one column.  Every sum is reduced the
// same way: the fixed wave butterfly (wave_sum), the 16 wave totals through LDS, added in wave order by ONE thread after the workgroup's single barrier -- thread 0
// for the six totals (the counts are whole numbers < 2^53: exact in fp64), thread o < O for column o, whose wave totals are the
// wave sums of the threads with t % O == o (the others add 0.0).  The totals are valid on thread 0, `col` on thread o < O.
struct GaussSums { double s, se, ae, n_in, n_bad, n_nonfinite, col; };
constexpr int kTotals = 6, kRed = kTotals + 16;                                           // LDS rows: the totals, then the columns

__device__ __forceinline__ double fold16(const double* p) {
    double s = p[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) s += p[i];
    return s;
}

__device__ __forceinline__ GaussSums gauss_sums(const float* __restrict__ mean, int ldm, const float* __restrict__ target, int ldt,
                                                const float* __restrict__ log_var, int ldv, long long n, int O, bool want_cols,
                                                double (*red)[16]) {
    const int T = (1024 / O) * O, t = threadIdx.x, col = t % O;
    double s = 0.0, se = 0.0, ae = 0.0, n_in = 0.0, n_bad = 0.0, n_nonfinite = 0.0, c = 0.0;
    if (t < T) {
        const int rows = 1024 / O;                                                        // rows per round of the T threads
        long long b = t / O;
#pragma unroll 1
        for (long long i = t; i < n; i += T, b += rows) {
            const float m = mean[b * ldm + col], y = target[b * ldt + col];
            const float lv = ldv ? log_var[b * ldv + col] : log_var[col];
            if (!isfinite(m) || !isfinite(lv)) n_nonfinite += 1.0;
            if (!target_ok(y)) { n_bad += 1.0; continue; }
            const float d = y - m;
            const float iv = expf(-lv);
            const float q = (d * d) * iv;
            s += (double)(0.5f * ((kLog2Pi + lv) + q));
            c += (double)(0.5f * (1.f - q));
            se += (double)(d * d);
            ae += (double)fabsf(d);
            if (fabsf(d) <= expf(0.5f * lv)) n_in += 1.0;
        }
    }
    const int lane = t & 63, w = t >> 6;
    const double v[kTotals] = {s, se, ae, n_in, n_bad, n_nonfinite};
#pragma unroll
    for (int k = 0; k < kTotals; ++k) {
        const double ws = wave_sum(v[k]);
        if (lane == 0) red[k][w] = ws;
    }
    if (want_cols) {
        for (int o = 0; o < O; ++o) {                                                     // (O is uniform: every wave takes every column)
            const double ws = wave_sum((t < T && col == o) ? c : 0.0);
            if (lane == 0) red[kTotals + o][w] = ws;
        }
    }
    __syncthreads();
    GaussSums r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (t == 0) {
        r.s = fold16(red[0]); r.se = fold16(red[1]); r.ae = fold16(red[2]);
        r.n_in = fold16(red[3]); r.n_bad = fold16(red[4]); r.n_nonfinite = fold16(red[5]);
    }
    if (want_cols && t < O) r.col = fold16(red[kTotals + t]);
    return r;
}

// What thread 0 adds to: read at the START of the kernel (launches of one stream are ordered: the values are final), so that the
// loads' latency lies under the pass instead of behind it; stored after it.  Plain loads and stores: one workgroup, no atomics.
struct GaussPre { double kl_term, st[4]; };

__device__ __forceinline__ GaussPre gauss_preload(const float* kl, float kl_scale, const double* stats) {
    GaussPre p = {0.0, {0.0, 0.0, 0.0, 0.0}};
    p.kl_term = kl_term_of(kl, kl_scale);
    if (stats) { p.st[0] = stats[0]; p.st[1] = stats[1]; p.st[2] = stats[2]; p.st[3] = stats[3]; }
    return p;
}

__device__ __forceinline__ void gauss_stats(double* stats, const GaussPre& p, const GaussSums& r, long long n) {
    stats[0] = p.st[0] + r.se;
    stats[1] = p.st[1] + r.ae;
    stats[2] = p.st[2] + ((double)n - r.n_bad);
    stats[3] = p.st[3] + r.n_bad;
}

// MONITOR: plus the training monitor (train_totals.h): the same pass, so *loss, stats and lv_cols are the plain kernel's bits.
// The unit of account of the totals is one element (b, o), as for the BCE loss; `correct` counts the elements inside one
// standard deviation.  The totals are loaded with gauss_preload's words, at the start of the kernel.
template <bool MONITOR>
__global__ __launch_bounds__(1024) void elbo_gaussian_loss_kernel(const float* __restrict__ mean, int ldm,
                                                                  const float* __restrict__ target, int ldt,
                                                                  const float* __restrict__ log_var, int ldv, long long n, int O,
                                                                  const float* kl, float kl_scale, float* loss, double* stats,
                                                                  float* lv_cols, int64_t* totals, int32_t* guard) {
    __shared__ double red[kRed][16];
    GaussPre pre = {0.0, {0.0, 0.0, 0.0, 0.0}};
    [[maybe_unused]] MonitorWords words = {{0, 0, 0, 0, 0, 0, 0, 0}, {0.0, 0.0, 0.0, 0.0, 0.0}};
    if (threadIdx.x == 0) {
        pre = gauss_preload(kl, kl_scale, stats);
        if constexpr (MONITOR) words = monitor_preload(totals);
    }
    const GaussSums r = gauss_sums(mean, ldm, target, ldt, log_var, ldv, n, O, lv_cols != nullptr, red);
    if (lv_cols && threadIdx.x < O) lv_cols[threadIdx.x] = (float)r.col;
    if (threadIdx.x == 0) {
        const TrainStep st = {r.s, pre.kl_term, n, (int64_t)r.n_in, (int64_t)r.n_bad, (int64_t)r.n_nonfinite};
        *loss = loss_of(st.nll, st.kl_term);
        if (stats) gauss_stats(stats, pre, r, n);
        if constexpr (MONITOR) monitor_commit(totals, guard, words, st);
    }
}

__global__ __launch_bounds__(256) void elbo_gaussian_loss_backward_kernel(const float* g, const float* __restrict__ mean, int ldm,
                                                                          const float* __restrict__ target, int ldt,
                                                                          const float* __restrict__ log_var, int ldv, long long n,
                                                                          int O, float kl_scale, const float* __restrict__ lv_cols,
                                                                          float* g_mean, float* g_lv, float* g_kl) {
    const float gv = *g;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / O;
        const int o = (int)(i - b * O);
        const float m = mean[b * ldm + o], y = target[b * ldt + o];
        const float lv = ldv ? log_var[b * ldv + o] : log_var[o];
        const bool ok = target_ok(y);
        const float iv = expf(-lv);
        g_mean[i] = ok ? (gv * (m - y)) * iv : 0.f;
        if (g_lv && ldv) {
            const float d = y - m;
            g_lv[i] = ok ? (gv * 0.5f) * (1.f - (d * d) * iv) : 0.f;
        }
    }
    if (g_lv && !ldv && blockIdx.x == 0 && threadIdx.x < O) g_lv[threadIdx.x] = gv * lv_cols[threadIdx.x];
    store_g_kl(g_kl, gv, kl_scale);
}

}  // namespace

extern "C" int lbbnn_elbo_gaussian_loss(const float* mean, int ldm, const float* target, int ldt, const float* log_var, int ldv,
                                        int B, int O, const float* kl, float kl_scale, float* loss, double* stats, float* lv_cols,
                                        void* stream) {
    if (!mean || !target || !log_var || !loss) return LBBNN_E_NULL;
    if (bad_shape(B, O) || ldm < O || ldt < O || (ldv != 0 && ldv < O)) return LBBNN_E_SHAPE;
    if (lv_cols && ldv != 0) return LBBNN_E_SHAPE;
    if (off(mean, 4) || off(target, 4) || off(log_var, 4) || off(kl, 4) || off(loss, 4) || off(lv_cols, 4) || off(stats, 8))
        return LBBNN_E_ALIGN;
    hipLaunchKernelGGL(elbo_gaussian_loss_kernel<false>, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), mean, ldm,
                       target, ldt, log_var, ldv, (long long)B * O, O, kl, kl_scale, loss, stats, lv_cols, (int64_t*)nullptr,
                       (int32_t*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_elbo_gaussian_loss_monitor(const float* mean, int ldm, const float* target, int ldt, const float* log_var,
                                                int ldv, int B, int O, const float* kl, float kl_scale, float* loss, double* stats,
                                                float* lv_cols, int64_t* totals, int32_t* guard, void* stream) {
    if (!mean || !target || !log_var || !loss || !totals) return LBBNN_E_NULL;
    if (bad_shape(B, O) || B < 1 || ldm < O || ldt < O || (ldv != 0 && ldv < O)) return LBBNN_E_SHAPE;
    if (lv_cols && ldv != 0) return LBBNN_E_SHAPE;
    if (off(mean, 4) || off(target, 4) || off(log_var, 4) || off(kl, 4) || off(loss, 4) || off(lv_cols, 4) || off(stats, 8) ||
        off(guard, 4) || off(totals, 8))
        return LBBNN_E_ALIGN;
    hipLaunchKernelGGL(elbo_gaussian_loss_kernel<true>, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), mean, ldm,
                       target, ldt, log_var, ldv, (long long)B * O, O, kl, kl_scale, loss, stats, lv_cols, totals, guard);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_elbo_gaussian_loss_backward(const float* g, const float* mean, int ldm, const float* target, int ldt,
                                                 const float* log_var, int ldv, int B, int O, float kl_scale, const float* lv_cols,
                                                 float* g_mean, float* g_lv, float* g_kl, void* stream) {
    if (!g || !mean || !target || !log_var || !g_mean) return LBBNN_E_NULL;
    if (g_lv && ldv == 0 && !lv_cols) return LBBNN_E_NULL;
    if (bad_shape(B, O) || ldm < O || ldt < O || (ldv != 0 && ldv < O)) return LBBNN_E_SHAPE;
    if (off(g, 4) || off(mean, 4) || off(target, 4) || off(log_var, 4) || off(lv_cols, 4) || off(g_mean, 4) || off(g_lv, 4) ||
        off(g_kl, 4))
        return LBBNN_E_ALIGN;
    const long long n = (long long)B * O;
    // (an empty batch still writes g_kl and a shared g_lv: one workgroup whose loop runs zero times)
    hipLaunchKernelGGL(elbo_gaussian_loss_backward_kernel, dim3(n ? grid_for(n) : 1), dim3(256), 0,
                       static_cast<hipStream_t>(stream), g, mean, ldm, target, ldt, log_var, ldv, n, O, kl_scale, lv_cols, g_mean,
                       g_lv, g_kl);
    return (int)hipGetLastError();
}
