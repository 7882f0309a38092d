// Regression metrics of an ensemble (include/lbbnn.h: lbbnn_eval_regression) from the (members, B, units) block of raw outputs
// the member GEMMs of an identity-head network leave, with a normal likelihood of log-variance lv[o] per output unit: the
// predictive mean, the epistemic / aleatoric split of the predictive variance, squared error, the log density of the members'
// mixture at the target and its probability integral transform, in ONE pass over the block plus a one-workgroup launch for the
// double sums.
//
// Layout: one thread per element (b, o), 256 elements per workgroup in element order e = b * O + o; the members are two loops of
// independent loads (the second needs the first's mean).  The integer totals are counted per workgroup in LDS (the counts and
// the PIT bins: dynamic LDS, sized from the arguments) and added to the caller's totals with integer atomics, zeros skipped;
// thread j < 8 then adds column j of the workgroup's elements in element order, in double, and leaves the partial in `work`,
// which the second launch adds in a fixed order.  The per-member values are single fp32 operations: no contraction.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"

#pragma clang fp contract(off)

namespace {

using namespace lbbnn;

constexpr int kThreads = 256;
constexpr int kMaxPitBins = 1024;
constexpr float kLog2Pi = 1.8378770664093453f;
constexpr float kRsqrt2 = 0.70710678118654752f;

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

// clamp((int)(v * scale), 0, n - 1): the product is clamped to [0, n] as a float first (a NaN or an overflowed product cannot
// reach the conversion: fmaxf returns its other operand for a NaN), the integer afterwards -- eval_uncertainty.hip's rule.
__device__ __forceinline__ int bin_of(float v, float scale, int n) {
    const float p = fminf(fmaxf(v * scale, 0.f), (float)n);
    return min(max((int)p, 0), n - 1);
}

__global__ __launch_bounds__(kThreads) void eval_regression_kernel(const RegK a) {
    extern __shared__ __attribute__((aligned(16))) unsigned bins[];   // K PIT counters
    __shared__ unsigned cnt[kCounts];
    __shared__ float colv[kSums][kThreads];
    __shared__ int flagv[kThreads];
    const int tid = threadIdx.x, lane = tid & 63;
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
        const float* p = a.out + b * a.ldp + o;
        const float lv = a.log_var[o];
        y = has_t ? a.target[b * a.ldt + o] : nanv;
        tvalid = has_t && isfinite(y);
        const float iv = expf(-lv), hs = expf(-0.5f * lv);
        av = expf(lv);
        fin = isfinite(lv);
        float acc = 0.f, pacc = 0.f;
        float mx = -INFINITY, ssum = 0.f;                          // streaming logsumexp over the members
        for (int m = 0; m < S; m += 4) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = p[(long long)min(m + k, S - 1) * a.m_stride];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (m + k >= S) break;
                const float x = v[k];
                fin = fin && isfinite(x);
                acc = (m + k == 0) ? x : acc + x;                  // the stated order: m_0, then += m_s
                const float r = y - x;
                const float t = -0.5f * ((kLog2Pi + lv) + (r * r) * iv);
                if (t > mx) {
                    ssum = ssum * expf(mx - t) + 1.f;
                    mx = t;
                } else if (t != -INFINITY) {
                    ssum += expf(t - mx);                          // (a NaN term arrives here and stays)
                }
                const float ph = 0.5f * erfcf(-((r * hs) * kRsqrt2));
                pacc = (m + k == 0) ? ph : pacc + ph;
            }
        }
        pm = acc / (float)S;                                       // IEEE division (hipcc's default)
        float acc2 = 0.f;
        for (int m = 0; m < S; m += 4) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = p[(long long)min(m + k, S - 1) * a.m_stride];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (m + k >= S) break;
                const float d = v[k] - pm;
                acc2 = (m + k == 0) ? d * d : acc2 + d * d;
            }
        }
        ev = acc2 / (float)S;
        tv = ev + av;
        if (tvalid) {
            const float err = y - pm;
            sq = err * err;
            ab = fabsf(err);
            ld = (mx + logf(ssum)) - logf((float)S);
            pit = pacc / (float)S;
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
#pragma unroll
    for (int k = 0; k < kCounts; ++k) {
        const unsigned long long bal = __ballot(flags[k]);
        if (lane == 0 && bal) atomicAdd(&cnt[k], (unsigned)__popcll(bal));
    }
    if (scored) atomicAdd(&bins[bin_of(pit, (float)K, K)], 1u);
    flagv[tid] = (in && fin ? kInFinite : 0) | (scored ? kInScored : 0);
    colv[kSumSq][tid] = sq; colv[kSumAbs][tid] = ab; colv[kSumLogDensity][tid] = ld; colv[kSumEpistemic][tid] = ev;
    colv[kSumTotalVar][tid] = tv; colv[kSumY][tid] = y; colv[kSumY2][tid] = y * y; colv[kSumPmSq][tid] = pmsq;
    __syncthreads();
    if (tid < kCounts && cnt[tid]) atomicAdd(&a.counts[tid], (unsigned long long)cnt[tid]);
    for (int i = tid; i < K; i += kThreads) {
        const unsigned c = bins[i];
        if (c) atomicAdd(&a.hist[i], (unsigned long long)c);
    }
    // column j of the workgroup's elements, added in element order
    if (tid < kSums) {
        const int need = (tid == kSumEpistemic || tid == kSumTotalVar) ? kInFinite : kInScored;
        double s = 0.0;
        for (int i = 0; i < kThreads; ++i)
            if ((flagv[i] & need) == need) s += (double)colv[tid][i];
        a.partials[(size_t)tid * (size_t)a.nblk + blockIdx.x] = s;
    }
}

// sums[j] += the workgroups' partials of column j.  Wave w takes the columns j = w, w + 4; lane l adds partials l, l + 64, ... in
// ascending order, then the fixed wave butterfly.
__global__ __launch_bounds__(kThreads) void eval_regression_sums_kernel(const double* __restrict__ partials, long long nblk,
                                                                         double* sums) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = w; j < kSums; j += kThreads / 64) {
        double s = 0.0;
        for (long long i = lane; i < nblk; i += 64) s += partials[(size_t)j * (size_t)nblk + i];
        s = wave_sum(s);
        if (lane == 0) sums[j] += s;
    }
}

long long workgroups(long long n) { return (n + kThreads - 1) / kThreads; }

bool off(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) != 0; }

}  // namespace

extern "C" int64_t lbbnn_eval_regression_work_bytes(int S, int B, int O) {
    (void)S;
    if (O < 1 || O > 16 || B < 0) return 0;
    const long long nblk = workgroups((long long)B * O);
    return (int64_t)sizeof(double) * kSums * (nblk > 0 ? nblk : 1);
}

extern "C" int lbbnn_eval_regression(const lbbnn_eval_regression_args_t* a, void* stream) {
    if (!a || !a->out || !a->log_var) return LBBNN_E_NULL;
    const bool any = a->counts || a->sums || a->pit_hist;
    if (any && !(a->counts && a->sums && a->pit_hist && a->work)) return LBBNN_E_NULL;
    if (a->S < 1 || a->S > 65535 || a->O < 1 || a->O > 16 || a->B < 0) return LBBNN_E_SHAPE;
    if (a->ldp < a->O || (a->mean_out && a->ldm < a->O) || (a->target && a->ldt < a->O)) return LBBNN_E_SHAPE;
    if (a->S > 1 && a->B > 0 && a->m_stride < (int64_t)(a->B - 1) * a->ldp + a->O) return LBBNN_E_SHAPE;
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
    hipLaunchKernelGGL(eval_regression_sums_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)a->work, k.nblk, a->sums);
    return (int)hipGetLastError();
}
