// Uncertainty and calibration metrics of an ensemble (include/lbbnn.h: lbbnn_eval_uncertainty) from the (members, B, classes)
// block of log-probabilities lbbnn_eval_metrics reads, in ONE pass over the block plus a one-workgroup launch for the double sums:
// the predictive distribution of the Bayesian model average, its entropy split into the expected part and the mutual information,
// Brier and log score per row, and running totals for reliability tables and score histograms.
//
// Layout: eval_metrics_kernel's.  A row's classes sit on G = the power of two >= C neighbouring lanes (256 / G rows per 256-thread
// workgroup), every reduction over the classes is a segmented DPP butterfly, the members are a loop of independent loads issued
// four at a time.  Totals: DESIGN.md, "Evaluation totals", through eval_totals.h.  Particular here: the LDS counters are 3 * M
// reliability and 3 * K histogram ones (dynamic LDS, sized from the arguments); a slot is a row, whose leader lane leaves the
// row's numbers in LDS; the columns are the 6 sums and, 6 + m, the confidence of bin m's rows with a target.
#include "eval_totals.h"
#include "seg_reduce.h"

namespace {

using namespace lbbnn;

constexpr int kThreads = kEvalThreads;
constexpr int kMaxConfBins = 100, kMaxHistBins = 4096;

enum { kRows = 0, kRowsWithTarget, kBadTargets, kCorrectBma, kNonfiniteRows, kLogScoreNonfinite, kCounts };
static_assert(kCounts == LBBNN_UNC_COUNTS, "the header's count list");
enum { kSumTotal = 0, kSumExpected, kSumMi, kSumConf, kSumBrier, kSumLogScore, kSums };
static_assert(kSums == LBBNN_UNC_SUMS, "the header's sum list");
static_assert(kSums + kMaxConfBins <= kThreads, "one thread per column of double partials");
// row flags in LDS: which sums a row enters
enum { kInFinite = 1, kInTarget = 2, kInLogScore = 4 };

struct UncK {
    const float* logp; long long m_stride, ldp;
    const int64_t* target;
    float* probs; int64_t* pred; float* conf; float* total; float* expected; float* mi; float* brier; float* log_score;
    unsigned long long* counts; unsigned long long* bin_rows; unsigned long long* bin_rows_t; unsigned long long* bin_correct;
    unsigned long long* hist;
    double* partials;
    long long nblk;
    int S, B, C, M, K;
    float ent_scale;
};

template <int G>
__global__ __launch_bounds__(kThreads) void eval_uncertainty_kernel(const UncK a) {
    constexpr int RPW = 64 / G, R = kThreads / G;                 // rows per wave / per workgroup
    extern __shared__ __attribute__((aligned(16))) unsigned bins[];   // [3 * M reliability counters | 3 * K histogram counters]
    __shared__ unsigned cnt[kCounts];
    __shared__ float rowv[kSums][R];
    __shared__ int rowbin[R], rowflag[R];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane / G, c = lane % G;
    const int S = a.S, C = a.C, M = a.M, K = a.K;
    const long long b = ((long long)blockIdx.x * (kThreads / 64) + w) * RPW + g;
    const bool rowok = b < a.B, cok = c < C;
    const long long bb = rowok ? b : (long long)a.B - 1;          // rows / classes past the end re-read the last one (masked below)
    const int cc = cok ? c : C - 1;
    const bool totals = a.counts != nullptr, has_t = a.target != nullptr;
    const long long t = has_t ? (long long)a.target[bb] : -1;
    const bool tvalid = rowok && has_t && t >= 0 && t < C;        // t is an index only behind this
    const bool leader = rowok && c == 0;
    const int nbins = 3 * M + 3 * K;
    if (totals) {
        if (tid < kCounts) cnt[tid] = 0u;
        for (int i = tid; i < nbins; i += kThreads) bins[i] = 0u;
        __syncthreads();
    }

    const float* p = a.logp + bb * a.ldp + cc;
    float acc = 0.f, hacc = 0.f;                                   // sum of expf(l) of this class / of the members' entropies
    float mx = -INFINITY, ssum = 0.f;                              // streaming logsumexp over the members of this lane's class
    for (int m = 0; m < S; m += 4) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p[(long long)min(m + k, S - 1) * a.m_stride];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (m + k >= S) break;
            const float x = v[k];
            const float e = cok ? expf(x) : 0.f;
            acc = (m + k == 0) ? e : acc + e;                     // the stated order: expf(logp[0]), then += expf(logp[m])
            const float h = -seg_sum<G>(e == 0.f ? 0.f : e * x);
            hacc = (m + k == 0) ? h : hacc + h;
            if (x > mx) {
                ssum = ssum * expf(mx - x) + 1.f;
                mx = x;
            } else if (x != -INFINITY) {
                ssum += expf(x - mx);                             // (a NaN member arrives here and stays)
            }
        }
    }

    const float pbar = acc / (float)S;                             // IEEE division (hipcc's default)
    if (a.probs && rowok && cok) a.probs[b * C + c] = pbar;
    const int pe = seg_argmax<G>(pbar, c, cok);
    const float conf = __shfl(pbar, lane - c + pe);                // the stored value of the winning class
    const float expd = hacc / (float)S;
    // one member: pbar = expf(l) exactly, so log pbar is l itself and H[pbar] the member's entropy -- taken as such, which makes
    // the mutual information of a single member exactly 0 instead of the rounding of logf(expf(l)) - l
    const float tot = S == 1 ? expd : -seg_sum<G>((!cok || pbar == 0.f) ? 0.f : pbar * logf(pbar));
    const float d = tot - expd;
    const float mi = d < 0.f ? 0.f : d;                            // NaN < 0 is false: a NaN stays
    const float nanv = __builtin_nanf("");
    const float dev = pbar - ((tvalid && c == (int)t) ? 1.f : 0.f);
    const float br = seg_sum<G>(cok ? dev * dev : 0.f);
    const float ls_own = -((mx + logf(ssum)) - logf((float)S));    // of this lane's class; the row wants its target's
    const float ls = __shfl(ls_own, lane - c + (tvalid ? (int)t : 0));
    if (leader) {
        if (a.pred) a.pred[b] = pe;
        if (a.conf) a.conf[b] = conf;
        if (a.total) a.total[b] = tot;
        if (a.expected) a.expected[b] = expd;
        if (a.mi) a.mi[b] = mi;
        if (a.brier) a.brier[b] = tvalid ? br : nanv;
        if (a.log_score) a.log_score[b] = tvalid ? ls : nanv;
    }
    if (!totals) return;

    // a bin index is taken from finite values only
    const bool fin = __builtin_isfinite(conf) && __builtin_isfinite(tot) && __builtin_isfinite(expd) && __builtin_isfinite(mi);
    const bool ls_fin = __builtin_isfinite(ls);
    const bool hit = tvalid && pe == (int)t;
    const bool flags[kCounts] = {leader, leader && tvalid, leader && has_t && !tvalid, leader && hit, leader && !fin,
                                 leader && fin && tvalid && !ls_fin};
    count_flags(flags, cnt);
    const int r = w * RPW + g;                                     // this row's slot in the workgroup, < R
    if (c == 0) {                                                  // one lane per slot, rows past the end included (flag 0)
        int mb = 0, flag = 0;
        if (rowok && fin) {
            mb = bin_of(conf, (float)M, M);
            flag = kInFinite | (tvalid ? kInTarget : 0) | ((tvalid && ls_fin) ? kInLogScore : 0);
            atomicAdd(&bins[mb], 1u);
            if (tvalid) atomicAdd(&bins[M + mb], 1u);
            if (hit) atomicAdd(&bins[2 * M + mb], 1u);
            atomicAdd(&bins[3 * M + bin_of(tot, a.ent_scale, K)], 1u);
            atomicAdd(&bins[3 * M + K + bin_of(mi, a.ent_scale, K)], 1u);
            atomicAdd(&bins[3 * M + 2 * K + bin_of(1.0f - conf, (float)K, K)], 1u);
        }
        rowbin[r] = mb;
        rowflag[r] = flag;
        rowv[kSumTotal][r] = tot; rowv[kSumExpected][r] = expd; rowv[kSumMi][r] = mi; rowv[kSumConf][r] = conf;
        rowv[kSumBrier][r] = br; rowv[kSumLogScore][r] = ls;
    }
    __syncthreads();
    flush_counters(cnt, kCounts, a.counts);
    flush_counters(bins, M, a.bin_rows);
    flush_counters(bins + M, M, a.bin_rows_t);
    flush_counters(bins + 2 * M, M, a.bin_correct);
    flush_counters(bins + 3 * M, 3 * K, a.hist);
    // column j < 6: a sum; 6 + m: the confidence of bin m's rows with a target
    if (tid < kSums + M) {
        const int need = tid < kSumBrier ? kInFinite : tid == kSumBrier ? (kInFinite | kInTarget)
                       : tid == kSumLogScore ? (kInFinite | kInLogScore) : (kInFinite | kInTarget);
        column_partial<R>(tid, rowv[tid < kSums ? tid : kSumConf], rowflag, need, a.partials, a.nblk, rowbin, tid - kSums);
    }
}

}  // namespace

extern "C" int64_t lbbnn_eval_uncertainty_work_bytes(int S, int B, int C, int conf_bins) {
    (void)S;
    if (C < 1 || C > 64 || B < 0 || conf_bins < 1 || conf_bins > kMaxConfBins) return 0;
    const long long nblk = row_workgroups(B, C);
    return (int64_t)sizeof(double) * (kSums + conf_bins) * (nblk > 0 ? nblk : 1);
}

extern "C" int lbbnn_eval_uncertainty(const lbbnn_eval_uncertainty_args_t* a, void* stream) {
    if (!a || !a->logp) return LBBNN_E_NULL;
    const int given = totals_given({a->counts, a->sums, a->bin_rows, a->bin_rows_with_target, a->bin_correct, a->bin_conf_sum, a->hist},
                                   a->work);
    if (given < 0) return LBBNN_E_NULL;
    const bool any = given > 0;
    if (check_member_block(a->S, 65535, a->B, a->C, 64, a->ldp, a->m_stride)) return LBBNN_E_SHAPE;
    if (row_workgroups(a->B, a->C) > 0x7FFFFFFFll) return LBBNN_E_SHAPE;
    if (any) {
        // the LDS counters are sized from these two: 4 * (3 * 100 + 3 * 4096) B at most, inside the 64 KiB a workgroup may ask for
        if (a->conf_bins < 1 || a->conf_bins > kMaxConfBins || a->hist_bins < 1 || a->hist_bins > kMaxHistBins) return LBBNN_E_SHAPE;
        if (!(a->ent_scale >= 0.f) || !(a->ent_scale <= 3.0e38f)) return LBBNN_E_SHAPE;      // (a NaN fails both)
    }
    if (off(a->logp, 4) || off(a->bma_probs, 4) || off(a->confidence, 4) || off(a->total_entropy, 4) ||
        off(a->expected_entropy, 4) || off(a->mutual_information, 4) || off(a->brier, 4) || off(a->log_score, 4) ||
        off(a->target, 8) || off(a->pred_bma, 8) || off(a->counts, 8) || off(a->sums, 8) || off(a->bin_rows, 8) ||
        off(a->bin_rows_with_target, 8) || off(a->bin_correct, 8) || off(a->bin_conf_sum, 8) || off(a->hist, 8) || off(a->work, 8))
        return LBBNN_E_ALIGN;
    if (a->B == 0) return 0;
    UncK k;
    k.logp = a->logp; k.m_stride = a->m_stride; k.ldp = a->ldp;
    k.target = a->target;
    k.probs = a->bma_probs; k.pred = a->pred_bma; k.conf = a->confidence; k.total = a->total_entropy;
    k.expected = a->expected_entropy; k.mi = a->mutual_information; k.brier = a->brier; k.log_score = a->log_score;
    k.counts = (unsigned long long*)a->counts; k.bin_rows = (unsigned long long*)a->bin_rows;
    k.bin_rows_t = (unsigned long long*)a->bin_rows_with_target; k.bin_correct = (unsigned long long*)a->bin_correct;
    k.hist = (unsigned long long*)a->hist;
    k.partials = (double*)a->work;
    k.nblk = row_workgroups(a->B, a->C);
    k.S = a->S; k.B = a->B; k.C = a->C;
    k.M = any ? a->conf_bins : 0; k.K = any ? a->hist_bins : 0;
    k.ent_scale = a->ent_scale;
    const size_t lds = sizeof(unsigned) * (size_t)(3 * k.M + 3 * k.K);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_lanes_per_row(a->C, [&](auto G) {
        hipLaunchKernelGGL(eval_uncertainty_kernel<decltype(G)::value>, dim3((unsigned)k.nblk), dim3(kThreads), lds, s, k);
    });
    int rc = (int)hipGetLastError();
    if (rc || !any) return rc;
    return launch_column_sums(a->work, k.nblk, kSums + k.M, a->sums, s, kSums, a->bin_conf_sum);
}
