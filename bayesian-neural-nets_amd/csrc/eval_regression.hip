// Regression metrics of an ensemble (include/lbbnn.h: lbbnn_eval_regression) from the (members, B, units) block of raw outputs
// the member GEMMs of an identity-head network leave, with a normal likelihood of log-variance lv[o] per output unit: the
// predictive mean, the epistemic / aleatoric split of the predictive variance, squared error, the log density of the members'
// mixture at the target and its probability integral transform, in ONE pass over the block plus a one-workgroup launch for the
// double sums.
//
// Layout: one thread per element (b, o), 256 elements per workgroup in element order e = b * O + o; the members are two loops of
// independent loads (the second needs the first's mean): eval_member_pass.h, with one log-variance for all members.  Totals:
// DESIGN.md, "Evaluation totals", through eval_totals.h; the LDS counters are the K PIT bins (dynamic LDS, sized from the
// arguments), a slot is an element, the columns are the 8 sums.  The per-member values are single fp32 operations: no contraction.
#include "eval_totals.h"

#pragma clang fp contract(off)
#include "eval_member_pass.h"

namespace {

using namespace lbbnn;

constexpr int kThreads = kEvalThreads;
constexpr int kMaxPitBins = 1024;

enum { kElements = 0, kWithTarget, kBadTargets, kNonfinite, kScored, kCounts };
static_assert(kCounts == LBBNN_REG_COUNTS, "the header's count list");
enum { kSumSq = 0, kSumAbs, kSumLogDensity, kSumEpistemic, kSumTotalVar, kSumY, kSumY2, kSumPmSq, kSums };
static_assert(kSums == LBBNN_REG_SUMS, "the header's sum list");
enum { kInFinite = 1, kInScored = 2 };

struct RegK {
    const float* out; long long m_stride, ldp;
    const float* mean_out; long long ldm;
    const float* target; long long ldt;
    const float* log_var;
    float* pred_mean; float* epistemic; float* aleatoric; float* total_std; float* sq_err; float* log_density; float* pit;
    unsigned long long* counts; unsigned long long* hist;
    double* partials;
    long long n, nblk;
    int S, O, K;
};

__global__ __launch_bounds__(kThreads) void eval_regression_kernel(const RegK a) {
    extern __shared__ __attribute__((aligned(16))) unsigned bins[];   // K PIT counters
    __shared__ unsigned cnt[kCounts];
    __shared__ float colv[kSums][kThreads];
    __shared__ int flagv[kThreads];
    const int tid = threadIdx.x;
    const int S = a.S, O = a.O, K = a.K;
    const long long e = (long long)blockIdx.x * kThreads + tid;
    const bool in = e < a.n;
    const bool totals = a.counts != nullptr;
    if (totals) {
        if (tid < kCounts) cnt[tid] = 0u;
        for (int i = tid; i < K; i += kThreads) bins[i] = 0u;
        __syncthreads();
    }

    const float nanv = __builtin_nanf("");
    float pm = 0.f, ev = 0.f, av = 0.f, tv = 0.f, sq = nanv, ab = 0.f, ld = nanv, pit = nanv, y = 0.f, pmsq = 0.f;
    bool fin = false, tvalid = false, has_t = a.target != nullptr;
    if (in) {
        const long long b = e / O;
        const int o = (int)(e - b * O);
        y = has_t ? a.target[b * a.ldt + o] : nanv;
        tvalid = has_t && isfinite(y);
        const MemberPass r = member_pass<false, false>(a.out + b * a.ldp + o, a.m_stride, a.log_var + o, 0, S, y);
        fin = isfinite(a.log_var[o]) && r.finite;
        pm = r.pm; ev = r.ev; av = r.av;
        tv = ev + av;
        if (tvalid) {
            const float err = y - pm;
            sq = err * err;
            ab = fabsf(err);
            ld = r.ld;
            pit = r.pit;
            if (a.mean_out) {
                const float f = y - a.mean_out[b * a.ldm + o];
                pmsq = f * f;
            }
        }
        if (a.pred_mean) a.pred_mean[e] = pm;
        if (a.epistemic) a.epistemic[e] = ev;
        if (a.aleatoric) a.aleatoric[e] = av;
        if (a.total_std) a.total_std[e] = sqrtf(tv);
        if (a.sq_err) a.sq_err[e] = sq;
        if (a.log_density) a.log_density[e] = ld;
        if (a.pit) a.pit[e] = pit;
    }
    if (!totals) return;

    const bool scored = in && fin && tvalid;
    const bool flags[kCounts] = {in, in && tvalid, in && has_t && !tvalid, in && !fin, scored};
    count_flags(flags, cnt);
    if (scored) atomicAdd(&bins[bin_of(pit, (float)K, K)], 1u);
    flagv[tid] = (in && fin ? kInFinite : 0) | (scored ? kInScored : 0);
    colv[kSumSq][tid] = sq; colv[kSumAbs][tid] = ab; colv[kSumLogDensity][tid] = ld; colv[kSumEpistemic][tid] = ev;
    colv[kSumTotalVar][tid] = tv; colv[kSumY][tid] = y; colv[kSumY2][tid] = y * y; colv[kSumPmSq][tid] = pmsq;
    __syncthreads();
    flush_counters(cnt, kCounts, a.counts);
    flush_counters(bins, K, a.hist);
    if (tid < kSums)
        column_partial<kThreads>(tid, colv[tid], flagv, (tid == kSumEpistemic || tid == kSumTotalVar) ? kInFinite : kInScored,
                                 a.partials, a.nblk);
}

long long workgroups(long long n) { return (n + kThreads - 1) / kThreads; }

}  // namespace

extern "C" int64_t lbbnn_eval_regression_work_bytes(int S, int B, int O) {
    (void)S;
    if (O < 1 || O > 16 || B < 0) return 0;
    const long long nblk = workgroups((long long)B * O);
    return (int64_t)sizeof(double) * kSums * (nblk > 0 ? nblk : 1);
}

extern "C" int lbbnn_eval_regression(const lbbnn_eval_regression_args_t* a, void* stream) {
    if (!a || !a->out || !a->log_var) return LBBNN_E_NULL;
    const int given = totals_given({a->counts, a->sums, a->pit_hist}, a->work);
    if (given < 0) return LBBNN_E_NULL;
    const bool any = given > 0;
    if (check_member_block(a->S, 65535, a->B, a->O, 16, a->ldp, a->m_stride)) return LBBNN_E_SHAPE;
    if ((a->mean_out && a->ldm < a->O) || (a->target && a->ldt < a->O)) return LBBNN_E_SHAPE;
    if ((long long)a->B * a->O > 0x7FFFFFFFll) return LBBNN_E_SHAPE;
    // the LDS counters are sized from pit_bins: 4 * 1024 B at most
    if (any && (a->pit_bins < 1 || a->pit_bins > kMaxPitBins)) return LBBNN_E_SHAPE;
    if (off(a->out, 4) || off(a->mean_out, 4) || off(a->target, 4) || off(a->log_var, 4) || off(a->pred_mean, 4) ||
        off(a->epistemic_var, 4) || off(a->aleatoric_var, 4) || off(a->total_std, 4) || off(a->sq_err, 4) ||
        off(a->log_density, 4) || off(a->pit, 4) || off(a->counts, 8) || off(a->sums, 8) || off(a->pit_hist, 8) || off(a->work, 8))
        return LBBNN_E_ALIGN;
    if (a->B == 0) return 0;
    RegK k;
    k.out = a->out; k.m_stride = a->m_stride; k.ldp = a->ldp;
    k.mean_out = a->mean_out; k.ldm = a->ldm;
    k.target = a->target; k.ldt = a->ldt;
    k.log_var = a->log_var;
    k.pred_mean = a->pred_mean; k.epistemic = a->epistemic_var; k.aleatoric = a->aleatoric_var; k.total_std = a->total_std;
    k.sq_err = a->sq_err; k.log_density = a->log_density; k.pit = a->pit;
    k.counts = (unsigned long long*)a->counts; k.hist = (unsigned long long*)a->pit_hist;
    k.partials = (double*)a->work;
    k.n = (long long)a->B * a->O;
    k.nblk = workgroups(k.n);
    k.S = a->S; k.O = a->O; k.K = any ? a->pit_bins : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(eval_regression_kernel, dim3((unsigned)k.nblk), dim3(kThreads), sizeof(unsigned) * (size_t)k.K, s, k);
    int rc = (int)hipGetLastError();
    if (rc || !any) return rc;
    return launch_column_sums(a->work, k.nblk, kSums, a->sums, s);
}
