// Regression scores of an ensemble (include/lbbnn.h: lbbnn_eval_regression_scores): what eval_regression.hip computes, with a
// log-variance operand that has strides of its own -- one value per unit, per element, or per member and element, the last form
// read in place from the upper columns of the members' own buffer -- plus the CRPS of the members' Gaussian mixture in closed form
// and central prediction intervals (quantiles of the mixture CDF by a fixed number of bisection steps), in ONE pass over the block
// plus a one-workgroup launch for the double sums.
//
// Layout: a workgroup of four waves takes 64 consecutive elements e = b * O + o; lane l of EVERY wave holds element l of them.  An
// element's work is a long serial chain (26 bisection steps of S erfcf each per quantile, S (S + 1) / 2 pair terms), and at
// evaluation sizes there are far fewer elements than lanes on the device, so the chain is cut four ways instead of giving every
// element one thread: wave w finds quantiles w and w + 4 (of 2 * n_levels), wave 3 also adds the CRPS's pair sum, wave 0 also runs
// the member pass of eval_regression.hip (means, logsumexp, PIT, the CRPS's first sum); the quantiles and the pair sum go through
// LDS to wave 0, which finishes the element and writes it.  Every wave rescans its element's members for the finite flag and the
// bracket with the same expressions, so no wave waits before its share.  A member's (mean, log-variance) pair is re-read from
// L1 / L2 wherever it is needed (the block is tens of KB at evaluation sizes, a member row a coalesced load across the wave).
// The CRPS sums are kept in double: non-negative terms whose difference cancels.  Totals: DESIGN.md, "Evaluation totals", through
// eval_totals.h; wave 0 holds all 64 slots, so its ballots go straight to the caller's counts, the LDS counters are the K PIT
// bins, the columns are the kSums sums.  The per-member values are single fp32 operations: no contraction.
#include "eval_totals.h"

#pragma clang fp contract(off)
#include "eval_member_pass.h"

namespace {

using namespace lbbnn;

constexpr int kThreads = kEvalThreads;
constexpr int kElems = 64;                  // elements per workgroup: one per lane, shared by the workgroup's four waves
constexpr int kWaves = kThreads / 64;
constexpr int kMaxPitBins = 1024;
constexpr int kMaxLevels = LBBNN_SCORE_MAX_LEVELS;
constexpr int kQuantiles = 2 * kMaxLevels;
static_assert(kQuantiles == 2 * kWaves, "wave w takes quantiles w and w + kWaves");
constexpr int kBisect = 26;                 // the bracket halves 26 times: (hi - lo) * 2^-27 about the returned midpoint
constexpr float kMaxAbsLv = 80.f;
constexpr float kMinLevel = 0.01f, kMaxLevel = 0.999f;

enum { kElements = 0, kWithTarget, kBadTargets, kNonfinite, kScored, kInside, kCounts = kInside + kMaxLevels };
static_assert(kInside == LBBNN_REG_COUNTS, "the first counts are lbbnn_eval_regression's");
static_assert(kCounts == LBBNN_SCORE_COUNTS, "the header's count list");
enum { kSumSq = 0, kSumAbs, kSumLogDensity, kSumEpistemic, kSumTotalVar, kSumY, kSumY2, kSumPmSq, kSumAleatoric, kSumCrps,
       kSumWidth, kSumIScore = kSumWidth + kMaxLevels, kSums = kSumIScore + kMaxLevels };
static_assert(kSumAleatoric == LBBNN_REG_SUMS, "the first sums are lbbnn_eval_regression's");
static_assert(kSums == LBBNN_SCORE_SUMS, "the header's sum list");
enum { kInFinite = 1, kInScored = 2 };

struct ScoreK {
    const float* out; long long m_stride, ldp;
    const float* mean_out; long long ldm;
    const float* target; long long ldt;
    const float* log_var; long long lv_ms, lv_ld;
    float* pred_mean; float* epistemic; float* aleatoric; float* total_std; float* sq_err; float* log_density; float* pit;
    float* crps; float* lower; float* upper; float* iscore;
    unsigned long long* counts; unsigned long long* hist;
    double* partials;
    long long n, nblk;
    int S, O, K, L;
    float levels[kMaxLevels];
};

__global__ __launch_bounds__(kThreads) void eval_scores_kernel(const ScoreK a) {
    extern __shared__ __attribute__((aligned(16))) unsigned bins[];   // K PIT counters
    __shared__ float qs[kQuantiles][kElems];                          // the waves' quantiles, for wave 0
    __shared__ double c2s[kElems];                                    // wave 3's pair sums
    __shared__ float colv[kSums][kElems];
    __shared__ int flagv[kElems];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int S = a.S, O = a.O, K = a.K, L = a.L, nq = 2 * a.L;
    const long long e = (long long)blockIdx.x * kElems + lane;
    const bool in = e < a.n;
    const bool totals = a.counts != nullptr;
    const bool has_t = a.target != nullptr;
    const bool want_q = L > 0 && (a.lower || a.upper || a.iscore || totals);
    const bool want_c = has_t && (a.crps || totals);
    for (int i = tid; i < K; i += kThreads) bins[i] = 0u;             // (K = 0 without totals)

    const float nanv = __builtin_nanf("");
    const long long b = in ? e / O : 0;
    const int o = (int)(e - b * O);
    const float* p = a.out + b * a.ldp + o;
    const float* q = a.log_var + b * a.lv_ld + o;
    const long long ms = a.m_stride, ls = a.lv_ms;
    const float y = (in && has_t) ? a.target[b * a.ldt + o] : nanv;
    const bool tvalid = in && has_t && isfinite(y);

    // every wave: is the element finite, and the quantiles' bracket [min_s (m_s - 8 sd_s), max_s (m_s + 8 sd_s)]
    bool fin = in;
    float blo = INFINITY, bhi = -INFINITY;
    if (in) {
        for (int m = 0; m < S; m += 4) {
            float v[4], u[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long s = min(m + k, S - 1);
                v[k] = p[s * ms];
                u[k] = q[s * ls];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (m + k >= S) break;
                fin = fin && isfinite(v[k]) && fabsf(u[k]) <= kMaxAbsLv;  // (a NaN log-variance fails the comparison)
                const float sd = sqrtf(expf(u[k]));
                blo = fminf(blo, v[k] - 8.f * sd);
                bhi = fmaxf(bhi, v[k] + 8.f * sd);
            }
        }
    }

    // wave w: quantiles w and w + kWaves of the mixture CDF F(x) = (1 / S) sum_s Phi((x - m_s) hs_s) -- pit's expression, member
    // order.  Quantile i = 2 l is level l's (1 - p_l) / 2 one, i = 2 l + 1 its (1 + p_l) / 2 one.  F < target moves the lower end up.
    if (want_q && w < nq) {
        const bool two = w + kWaves < nq;
        const int i0 = w, i1 = two ? w + kWaves : w;
        const float lev0 = a.levels[i0 >> 1], lev1 = a.levels[i1 >> 1];
        const float pt0 = (i0 & 1) ? 0.5f * (1.f + lev0) : 0.5f * (1.f - lev0);
        const float pt1 = (i1 & 1) ? 0.5f * (1.f + lev1) : 0.5f * (1.f - lev1);
        float r0 = nanv, r1 = nanv;
        if (fin) {
            float lo0 = blo, hi0 = bhi, lo1 = blo, hi1 = bhi;
            for (int it = 0; it < kBisect; ++it) {
                const float mid0 = 0.5f * (lo0 + hi0), mid1 = 0.5f * (lo1 + hi1);
                float F0 = 0.f, F1 = 0.f;
                for (int s = 0; s < S; ++s) {
                    const float x = p[(long long)s * ms], hs = expf(-0.5f * q[(long long)s * ls]);
                    const float ph0 = 0.5f * erfcf(-(((mid0 - x) * hs) * kRsqrt2));
                    F0 = (s == 0) ? ph0 : F0 + ph0;
                    if (two) {
                        const float ph1 = 0.5f * erfcf(-(((mid1 - x) * hs) * kRsqrt2));
                        F1 = (s == 0) ? ph1 : F1 + ph1;
                    }
                }
                if (F0 / (float)S < pt0) lo0 = mid0; else hi0 = mid0;
                if (two) {
                    if (F1 / (float)S < pt1) lo1 = mid1; else hi1 = mid1;
                }
            }
            r0 = 0.5f * (lo0 + hi0);
            r1 = 0.5f * (lo1 + hi1);
        }
        qs[i0][lane] = r0;
        if (two) qs[i1][lane] = r1;
    }

    // the last wave: sum_{s,t} A(m_s - m_t, v_s + v_t) = sum_s [A(0, 2 v_s) + 2 sum_{t<s} A(m_s - m_t, v_s + v_t)], s, t ascending
    if (w == kWaves - 1) {
        double c2 = 0.0;
        if (want_c && fin && tvalid) {
            for (int s = 0; s < S; ++s) {
                const float xs = p[(long long)s * ms], vs = expf(q[(long long)s * ls]);
                c2 += (double)a_term(0.f, vs + vs);
                for (int t = 0; t < s; ++t) {
                    const float xt = p[(long long)t * ms], vt = ls ? expf(q[(long long)t * ls]) : vs;
                    c2 += 2.0 * (double)a_term(xs - xt, vs + vt);
                }
            }
        }
        c2s[lane] = c2;
    }

    // wave 0: the member pass with a log-variance per member, and the CRPS's first sum
    float pm = nanv, ev = nanv, av = nanv, tv = nanv, sq = nanv, ab = 0.f, ld = nanv, pit = nanv, pmsq = 0.f;
    double c1 = 0.0;
    if (w == 0 && fin) {
        const MemberPass r = member_pass<true, true>(p, ms, q, ls, S, y);
        pm = r.pm; ev = r.ev; av = r.av; c1 = r.c1;
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
    }
    __syncthreads();                                               // qs, c2s and the zeroed bins are there

    // wave 0 finishes its elements, writes them and leaves the workgroup's columns in LDS
    if (w == 0) {
        float crps = nanv;
        float ql[kMaxLevels], qu[kMaxLevels], wd[kMaxLevels], is[kMaxLevels];
        bool inside[kMaxLevels];
        if (fin && tvalid && want_c) {
            const double dS = (double)S;
            crps = (float)(c1 / dS - c2s[lane] / (2.0 * dS * dS));
        }
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) {
            ql[l] = qu[l] = wd[l] = is[l] = nanv;
            inside[l] = false;
            if (l < L && want_q && fin) {
                ql[l] = qs[2 * l][lane];
                qu[l] = qs[2 * l + 1][lane];
                wd[l] = qu[l] - ql[l];
                if (tvalid) {
                    is[l] = wd[l] + (2.f / (1.f - a.levels[l])) * (fmaxf(ql[l] - y, 0.f) + fmaxf(y - qu[l], 0.f));
                    inside[l] = ql[l] <= y && y <= qu[l];
                }
            }
        }
        if (in) {
            if (a.pred_mean) a.pred_mean[e] = pm;
            if (a.epistemic) a.epistemic[e] = ev;
            if (a.aleatoric) a.aleatoric[e] = av;
            if (a.total_std) a.total_std[e] = sqrtf(tv);
            if (a.sq_err) a.sq_err[e] = sq;
            if (a.log_density) a.log_density[e] = ld;
            if (a.pit) a.pit[e] = pit;
            if (a.crps) a.crps[e] = crps;
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l) {
                if (l < L) {
                    const long long at = (long long)l * a.n + e;
                    if (a.lower) a.lower[at] = ql[l];
                    if (a.upper) a.upper[at] = qu[l];
                    if (a.iscore) a.iscore[at] = is[l];
                }
            }
        }
        if (totals) {
            const bool scored = fin && tvalid;
            bool flags[kCounts] = {in, tvalid, in && has_t && !tvalid, in && !fin, scored};
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l) flags[kInside + l] = scored && inside[l];
            count_flags(flags, a.counts);                           // one wave holds the whole workgroup's elements: no LDS stage
            if (scored) atomicAdd(&bins[bin_of(pit, (float)K, K)], 1u);
            flagv[lane] = (fin ? kInFinite : 0) | (scored ? kInScored : 0);
            colv[kSumSq][lane] = sq; colv[kSumAbs][lane] = ab; colv[kSumLogDensity][lane] = ld; colv[kSumEpistemic][lane] = ev;
            colv[kSumTotalVar][lane] = tv; colv[kSumY][lane] = y; colv[kSumY2][lane] = y * y; colv[kSumPmSq][lane] = pmsq;
            colv[kSumAleatoric][lane] = av; colv[kSumCrps][lane] = crps;
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l) {
                colv[kSumWidth + l][lane] = l < L ? wd[l] : 0.f;
                colv[kSumIScore + l][lane] = l < L ? is[l] : 0.f;
            }
        }
    }
    if (!totals) return;                                           // (uniform over the grid)
    __syncthreads();
    flush_counters(bins, K, a.hist);
    if (tid < kSums)
        column_partial<kElems>(tid, colv[tid], flagv,
                               (tid == kSumEpistemic || tid == kSumTotalVar || tid == kSumAleatoric) ? kInFinite : kInScored,
                               a.partials, a.nblk);
}

long long workgroups(long long n) { return (n + kElems - 1) / kElems; }

}  // namespace

extern "C" int64_t lbbnn_eval_regression_scores_work_bytes(int S, int B, int O, int levels) {
    if (S < 1 || S > LBBNN_SCORE_MAX_MEMBERS || O < 1 || O > 16 || B < 0 || levels < 0 || levels > kMaxLevels) return 0;
    const long long nblk = workgroups((long long)B * O);
    return (int64_t)sizeof(double) * kSums * (nblk > 0 ? nblk : 1);
}

extern "C" int lbbnn_eval_regression_scores(const lbbnn_eval_scores_args_t* a, void* stream) {
    if (!a || !a->out || !a->log_var) return LBBNN_E_NULL;
    const int given = totals_given({a->counts, a->sums, a->pit_hist}, a->work);
    if (given < 0) return LBBNN_E_NULL;
    const bool any = given > 0;
    if (check_member_block(a->S, LBBNN_SCORE_MAX_MEMBERS, a->B, a->O, 16, a->ldp, a->m_stride)) return LBBNN_E_SHAPE;
    if ((a->mean_out && a->ldm < a->O) || (a->target && a->ldt < a->O)) return LBBNN_E_SHAPE;
    if ((long long)a->B * a->O > 0x7FFFFFFFll) return LBBNN_E_SHAPE;
    // the log-variance operand: (0, 0) per unit, (0, ld) per element, (ms, ld) per member and element
    if (a->lv_ld != 0 && a->lv_ld < a->O) return LBBNN_E_SHAPE;
    if (a->lv_mstride < 0 || (a->lv_mstride != 0 && a->lv_ld == 0)) return LBBNN_E_SHAPE;
    if (a->lv_mstride != 0 && a->S > 1 && a->B > 0 && a->lv_mstride < (int64_t)(a->B - 1) * a->lv_ld + a->O) return LBBNN_E_SHAPE;
    if (a->n_levels < 0 || a->n_levels > kMaxLevels) return LBBNN_E_SHAPE;
    for (int l = 0; l < a->n_levels; ++l)
        if (!(a->levels[l] >= kMinLevel && a->levels[l] <= kMaxLevel)) return LBBNN_E_SHAPE;
    // the LDS counters are sized from pit_bins: 4 * 1024 B at most
    if (any && (a->pit_bins < 1 || a->pit_bins > kMaxPitBins)) return LBBNN_E_SHAPE;
    if (off(a->out, 4) || off(a->mean_out, 4) || off(a->target, 4) || off(a->log_var, 4) || off(a->pred_mean, 4) ||
        off(a->epistemic_var, 4) || off(a->aleatoric_var, 4) || off(a->total_std, 4) || off(a->sq_err, 4) ||
        off(a->log_density, 4) || off(a->pit, 4) || off(a->crps, 4) || off(a->lower, 4) || off(a->upper, 4) ||
        off(a->interval_score, 4) || off(a->counts, 8) || off(a->sums, 8) || off(a->pit_hist, 8) || off(a->work, 8))
        return LBBNN_E_ALIGN;
    if (a->B == 0) return 0;
    ScoreK k;
    k.out = a->out; k.m_stride = a->S > 1 ? a->m_stride : 0; k.ldp = a->ldp;
    k.mean_out = a->mean_out; k.ldm = a->ldm;
    k.target = a->target; k.ldt = a->ldt;
    k.log_var = a->log_var; k.lv_ms = a->S > 1 ? a->lv_mstride : 0; k.lv_ld = a->lv_ld;
    k.pred_mean = a->pred_mean; k.epistemic = a->epistemic_var; k.aleatoric = a->aleatoric_var; k.total_std = a->total_std;
    k.sq_err = a->sq_err; k.log_density = a->log_density; k.pit = a->pit; k.crps = a->crps;
    k.lower = a->lower; k.upper = a->upper; k.iscore = a->interval_score;
    k.counts = (unsigned long long*)a->counts; k.hist = (unsigned long long*)a->pit_hist;
    k.partials = (double*)a->work;
    k.n = (long long)a->B * a->O;
    k.nblk = workgroups(k.n);
    k.S = a->S; k.O = a->O; k.K = any ? a->pit_bins : 0; k.L = a->n_levels;
    for (int l = 0; l < kMaxLevels; ++l) k.levels[l] = l < a->n_levels ? a->levels[l] : 0.5f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(eval_scores_kernel, dim3((unsigned)k.nblk), dim3(kThreads), sizeof(unsigned) * (size_t)k.K, s, k);
    int rc = (int)hipGetLastError();
    if (rc || !any) return rc;
    return launch_column_sums(a->work, k.nblk, kSums, a->sums, s);
}
