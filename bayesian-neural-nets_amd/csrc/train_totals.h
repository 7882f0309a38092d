// What the three training losses share (loss_head.hip, binary_head.hip, gaussian_head.hip), written once; DESIGN.md 9.4 has
// the scheme.  A loss is ONE launch of ONE workgroup; its thread 0 ends the step:
//   *loss = (float)(nll + kl_term), and with a monitor (include/lbbnn.h: lbbnn_elbo_loss_monitor) the guard word and the running
//   totals of a training log.
// The rules of the monitor tail, for every head:
//   * Launches of one stream are ordered and there is one workgroup: thread 0 adds to the totals with plain loads and stores --
//     no atomics, the same bits from run to run.
//   * Every load of the totals comes ahead of the first store (monitor_preload, into registers).  Where the preload sits is the
//     kernel's choice: at its start, under the pass (the Gaussian loss), or in the tail (the other two).
//   * A step is FINITE when the fp32 loss, (float)(nll + kl_term), is: the guard word is 0 after a finite step and 1 after any
//     other, per step.  nll_rows and the three sums grow on a finite step only, nonfinite_steps on any other; steps, rows,
//     correct, bad_targets and nonfinite_rows always do; last_nll and last_loss are overwritten by every step.
//   * LBBNN_MONITOR_SKIPPED_STEPS is the optimizer's word: never written here.
//   * Thread 0 stores *loss, then the head's own stats, then the guard, then the totals: a kernel stores loss_of() itself
//     and calls monitor_commit last.
// A head says what a unit is (a row, or an element (b, o)) and which units are correct, bad and non-finite: a TrainStep.
#pragma once
#include "lbbnn_device.h"
#include "lbbnn_internal.h"

namespace lbbnn {

// kl / NUM_BATCHES in fp64; no kl, no term
__device__ __forceinline__ double kl_term_of(const float* kl, float kl_scale) {
    return kl ? (double)(*kl) * (double)kl_scale : 0.0;
}

// ... and its gradient, by one thread of the backward launch
__device__ __forceinline__ void store_g_kl(float* g_kl, float gv, float kl_scale) {
    if (g_kl && blockIdx.x == 0 && threadIdx.x == 0) *g_kl = gv * kl_scale;
}

// THE loss of a step: the fp64 sum, rounded once
__device__ __forceinline__ float loss_of(double nll, double kl_term) { return (float)(nll + kl_term); }

struct TrainStep { double nll, kl_term; int64_t units, correct, bad, nonfinite; };

struct MonitorWords { int64_t cnt[LBBNN_MONITOR_COUNTS]; double sum[LBBNN_MONITOR_SUMS]; };

__device__ __forceinline__ MonitorWords monitor_preload(const int64_t* totals) {
    MonitorWords w;
    const double* sums = reinterpret_cast<const double*>(totals + LBBNN_MONITOR_COUNTS);
#pragma unroll
    for (int q = 0; q < LBBNN_MONITOR_COUNTS; ++q) w.cnt[q] = totals[q];
#pragma unroll
    for (int q = 0; q < LBBNN_MONITOR_SUMS; ++q) w.sum[q] = sums[q];
    return w;
}

__device__ __forceinline__ float monitor_commit(int64_t* totals, int32_t* guard, const MonitorWords& w, const TrainStep& st) {
    double* sums = reinterpret_cast<double*>(totals + LBBNN_MONITOR_COUNTS);
    const float lf = loss_of(st.nll, st.kl_term);
    const bool ok = isfinite(lf);
    if (guard) *guard = ok ? 0 : 1;
    totals[LBBNN_MONITOR_STEPS] = w.cnt[LBBNN_MONITOR_STEPS] + 1;
    totals[LBBNN_MONITOR_ROWS] = w.cnt[LBBNN_MONITOR_ROWS] + st.units;
    totals[LBBNN_MONITOR_CORRECT] = w.cnt[LBBNN_MONITOR_CORRECT] + st.correct;
    totals[LBBNN_MONITOR_BAD_TARGETS] = w.cnt[LBBNN_MONITOR_BAD_TARGETS] + st.bad;
    totals[LBBNN_MONITOR_NONFINITE_ROWS] = w.cnt[LBBNN_MONITOR_NONFINITE_ROWS] + st.nonfinite;
    if (ok) {
        totals[LBBNN_MONITOR_NLL_ROWS] = w.cnt[LBBNN_MONITOR_NLL_ROWS] + (st.units - st.bad);
        sums[LBBNN_MONITOR_NLL_SUM] = w.sum[LBBNN_MONITOR_NLL_SUM] + st.nll;
        sums[LBBNN_MONITOR_KL_TERM_SUM] = w.sum[LBBNN_MONITOR_KL_TERM_SUM] + st.kl_term;
        sums[LBBNN_MONITOR_LOSS_SUM] = w.sum[LBBNN_MONITOR_LOSS_SUM] + (st.nll + st.kl_term);
    } else {
        totals[LBBNN_MONITOR_NONFINITE_STEPS] = w.cnt[LBBNN_MONITOR_NONFINITE_STEPS] + 1;
    }
    sums[LBBNN_MONITOR_LAST_NLL] = st.nll;
    sums[LBBNN_MONITOR_LAST_LOSS] = (double)lf;
    return lf;
}

// The two element-wise heads (binary_head.hip, gaussian_head.hip): a (B, O) block of at most 16 columns and 2^31 - 1 elements,
// and the grid of their 256-thread grid-stride kernels.
inline bool bad_shape(int B, int O) { return B < 0 || O < 1 || O > 16 || (long long)B * O > 0x7FFFFFFFLL; }
inline int grid_for(long long n) { const long long b = (n + 255) / 256; return (int)(b < 1024 ? b : 1024); }

}  // namespace lbbnn
