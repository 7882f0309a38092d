// Ensemble evaluation metrics (include/lbbnn.h: lbbnn_eval_metrics): everything the reference's evaluation loops compute from a
// (members, B, classes) block of log-probabilities, in ONE pass over the block plus a one-workgroup launch for the double sums.
//
//   test_ensemble   LBBNN-GP-MF-MNF.py:312-323   mean over members, argmax, posterior-mean argmax, two correct counts
//   outofsample     LBBNN-GP-MF-MNF.py:370-392   per member sigmoid / row sum, member mean, -sum p log p, per-member corrects
//   VD validation   variational_dropout.py:160-176   member mean, nll_loss(sum), correct count, confusion[target][prediction]
//
// Layout: a row's classes sit on G = the power of two >= C neighbouring lanes, so a wave holds 64 / G rows and a 256-thread
// workgroup 256 / G; every reduction over the classes is a segmented DPP butterfly (no LDS), the members are a loop of
// independent loads issued four at a time.  Totals: DESIGN.md, "Evaluation totals"; the integer ones go through eval_totals.h,
// the two double sums keep a layout of their own (below): each workgroup's block sum is one partial in `work`.
#include "eval_totals.h"
#include "seg_reduce.h"

namespace {

using namespace lbbnn;

constexpr int kThreads = kEvalThreads;
constexpr int kMemberChunk = 1024;     // per-member correct counts held in LDS at a time

struct EvalK {
    const float* logp; long long m_stride, ldp;
    const float* mean_logp; long long ldm;
    const int64_t* target;
    float* ens; int64_t* pred_ens; int64_t* pred_mean; float* entropy;
    unsigned long long* counts; unsigned long long* correct_member; unsigned long long* confusion;
    double* partials;
    int S, B, C;
};

enum { kRows = 0, kRowsWithTarget, kBadTargets, kCorrectEnsemble, kCorrectPosteriorMean, kEntropyNonfinite, kCounts };
static_assert(kCounts == LBBNN_EVAL_COUNTS, "the header's count list");

template <int G>
__global__ __launch_bounds__(kThreads) void eval_metrics_kernel(const EvalK a) {
    constexpr int RPW = 64 / G;
    __shared__ unsigned hist[G * G];
    __shared__ unsigned mcount[kMemberChunk];
    __shared__ unsigned cnt[kCounts];
    __shared__ double scratch[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane / G, c = lane % G;
    const int S = a.S, C = a.C;
    const long long b = ((long long)blockIdx.x * (kThreads / 64) + w) * RPW + g;
    const bool rowok = b < a.B, cok = c < C;
    const long long bb = rowok ? b : (long long)a.B - 1;          // rows / classes past the end re-read the last one (masked below)
    const int cc = cok ? c : C - 1;
    const bool totals = a.counts != nullptr, has_t = a.target != nullptr;
    const long long t = has_t ? (long long)a.target[bb] : -1;
    const bool tvalid = rowok && has_t && t >= 0 && t < C;
    const bool leader = rowok && c == 0;
    const bool want_member = totals && has_t;
    if (totals) {
        if (tid < kCounts) cnt[tid] = 0u;
        for (int i = tid; i < C * C; i += kThreads) hist[i] = 0u;
        __syncthreads();
    }

    const float* p = a.logp + bb * a.ldp + cc;
    float acc = 0.f, pacc = 0.f;
    for (int m0 = 0; m0 < S; m0 += kMemberChunk) {
        const int mend = min(S, m0 + kMemberChunk);
        if (want_member) {
            for (int i = tid; i < mend - m0; i += kThreads) mcount[i] = 0u;
            __syncthreads();
        }
        for (int m = m0; m < mend; m += 4) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = p[(long long)min(m + k, mend - 1) * a.m_stride];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (m + k >= mend) break;
                const float x = v[k];
                acc = (m + k == 0) ? x : acc + x;                 // the stated order: logp[0], then += logp[m], m ascending
                const float sg = cok ? 1.0f / (1.0f + expf(-x)) : 0.f;
                pacc += sg / seg_sum<G>(sg);
                if (want_member) {
                    const int pm = seg_argmax<G>(x, c, cok);
                    const unsigned long long hit = __ballot(tvalid && c == 0 && pm == (int)t);
                    if (lane == 0 && hit) atomicAdd(&mcount[m + k - m0], (unsigned)__popcll(hit));
                }
            }
        }
        if (want_member) {
            __syncthreads();
            for (int i = tid; i < mend - m0; i += kThreads)
                if (mcount[i]) atomicAdd(&a.correct_member[m0 + i], (unsigned long long)mcount[i]);
            __syncthreads();
        }
    }

    const float ens = acc / (float)S;                              // IEEE division (hipcc's default)
    if (a.ens && rowok && cok) a.ens[b * C + c] = ens;
    const int pe = seg_argmax<G>(ens, c, cok);
    const float pbar = pacc / (float)S;
    const float ent = -seg_sum<G>(cok ? pbar * logf(pbar) : 0.f);
    int pq = -1;
    if (a.mean_logp) pq = seg_argmax<G>(a.mean_logp[bb * a.ldm + cc], c, cok);
    if (leader) {
        if (a.pred_ens) a.pred_ens[b] = pe;
        if (a.pred_mean) a.pred_mean[b] = pq;
        if (a.entropy) a.entropy[b] = ent;
    }
    if (!totals) return;

    const bool fin = __builtin_isfinite(ent);
    const bool flags[kCounts] = {leader, leader && tvalid, leader && has_t && !tvalid, leader && tvalid && pe == (int)t,
                                 leader && tvalid && a.mean_logp != nullptr && pq == (int)t, leader && !fin};
    count_flags(flags, cnt);
    if (leader && tvalid) atomicAdd(&hist[(int)t * C + pe], 1u);   // rows: the true label
    double nll = (tvalid && cok && c == (int)t) ? -(double)ens : 0.0;
    double es = (leader && fin) ? (double)ent : 0.0;
    nll = block_sum<double, kThreads / 64>(nll, scratch);          // fixed order: the wave butterfly, then the 4 waves
    es = block_sum<double, kThreads / 64>(es, scratch);
    flush_counters(cnt, kCounts, a.counts);
    flush_counters(hist, C * C, a.confusion);
    if (tid == 0) {
        a.partials[2 * (size_t)blockIdx.x] = nll;
        a.partials[2 * (size_t)blockIdx.x + 1] = es;
    }
}

// sums[0] += the workgroups' nll partials, sums[1] += their entropy partials: thread t adds partials t, t + 256, ... in
// ascending order, then the fixed block sum.
__global__ __launch_bounds__(kThreads) void eval_metrics_sums_kernel(const double* __restrict__ partials, long long nblk, double* sums) {
    __shared__ double scratch[kThreads / 64];
    double s0 = 0.0, s1 = 0.0;
    for (long long i = threadIdx.x; i < nblk; i += kThreads) {
        s0 += partials[2 * i];
        s1 += partials[2 * i + 1];
    }
    s0 = block_sum<double, kThreads / 64>(s0, scratch);
    s1 = block_sum<double, kThreads / 64>(s1, scratch);
    if (threadIdx.x == 0) {
        sums[0] += s0;
        sums[1] += s1;
    }
}

}  // namespace

extern "C" int64_t lbbnn_eval_metrics_work_bytes(int S, int B, int C) {
    (void)S;
    if (C < 1 || C > 64 || B < 0) return 0;
    const long long nblk = row_workgroups(B, C);
    return (int64_t)(2 * sizeof(double)) * (nblk > 0 ? nblk : 1);
}

extern "C" int lbbnn_eval_metrics(const lbbnn_eval_metrics_args_t* a, void* stream) {
    if (!a || !a->logp) return LBBNN_E_NULL;
    const int given = totals_given({a->counts, a->correct_member, a->confusion, a->sums}, a->work);
    if (given < 0) return LBBNN_E_NULL;
    const bool any = given > 0;
    if (a->pred_mean && !a->mean_logp) return LBBNN_E_NULL;
    if (check_member_block(a->S, 65535, a->B, a->C, 64, a->ldp, a->m_stride)) return LBBNN_E_SHAPE;
    if (a->mean_logp && a->ldm < a->C) return LBBNN_E_SHAPE;
    if (row_workgroups(a->B, a->C) > 0x7FFFFFFFll) return LBBNN_E_SHAPE;
    if (off(a->logp, 4) || off(a->mean_logp, 4) || off(a->ens_logp, 4) || off(a->entropy, 4) || off(a->target, 8) ||
        off(a->pred_ensemble, 8) || off(a->pred_mean, 8) || off(a->counts, 8) || off(a->correct_member, 8) ||
        off(a->confusion, 8) || off(a->sums, 8) || off(a->work, 8))
        return LBBNN_E_ALIGN;
    if (a->B == 0) return 0;
    EvalK k;
    k.logp = a->logp; k.m_stride = a->m_stride; k.ldp = a->ldp;
    k.mean_logp = a->mean_logp; k.ldm = a->ldm;
    k.target = a->target;
    k.ens = a->ens_logp; k.pred_ens = a->pred_ensemble; k.pred_mean = a->pred_mean; k.entropy = a->entropy;
    k.counts = (unsigned long long*)a->counts; k.correct_member = (unsigned long long*)a->correct_member;
    k.confusion = (unsigned long long*)a->confusion;
    k.partials = (double*)a->work;
    k.S = a->S; k.B = a->B; k.C = a->C;
    const long long nblk = row_workgroups(a->B, a->C);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_lanes_per_row(a->C, [&](auto G) {
        hipLaunchKernelGGL(eval_metrics_kernel<decltype(G)::value>, dim3((unsigned)nblk), dim3(kThreads), 0, s, k);
    });
    int rc = (int)hipGetLastError();
    if (rc || !any) return rc;
    hipLaunchKernelGGL(eval_metrics_sums_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)a->work, nblk, a->sums);
    return (int)hipGetLastError();
}
