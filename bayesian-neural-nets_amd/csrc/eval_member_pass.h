// The pass over an element's S members that eval_regression.hip and eval_scores.hip share: the mean in the stated order, the
// streaming logsumexp of the members' normal densities at the target, the PIT sum, then the variance about the mean; for the
// scores also the mean of the members' variances and the CRPS's first sum.  The per-member values are the single fp32
// operations include/lbbnn.h documents: no contraction, here or in the including file.
#pragma once
#include "lbbnn_device.h"

#pragma clang fp contract(off)

namespace lbbnn {

constexpr float kLog2Pi = 1.8378770664093453f;
constexpr float kRsqrt2 = 0.70710678118654752f;
constexpr float kRsqrt2Pi = 0.39894228040143268f;

// A(m, v) = 2 sqrt(v) phi(m / sqrt v) + m (2 Phi(m / sqrt v) - 1) = E|N(m, v)|, as 2 sd phi(z) + |m| erf(z / sqrt 2) with
// z = |m| / sd: both terms non-negative, and no 0 * inf (z * z may overflow: expf(-inf) = 0).  sd > 0 is the caller's.
__device__ __forceinline__ float a_term(float m, float v) {
    const float sd = sqrtf(v), am = fabsf(m), z = am / sd;
    return (2.f * sd) * (kRsqrt2Pi * expf(-0.5f * (z * z))) + am * erff(z * kRsqrt2);
}

struct MemberPass {
    float pm, ev, av;          // predictive mean, variance of the members about it, (mean) noise variance
    float ld, pit;             // log density of the mixture at y and its CDF there (meaningful for a finite y)
    double c1;                 // sum_s A(y - m_s, v_s) (Crps only)
    bool finite;               // every member finite
};

// Members p[s * ms] with log-variance q[s * ls] (LvPerMember), or q[0] for all of them: then its three exponentials are taken
// once, and av is expf(lv) itself, not a mean.
template <bool LvPerMember, bool Crps>
__device__ __forceinline__ MemberPass member_pass(const float* p, long long ms, const float* q, long long ls, int S, float y) {
    MemberPass r;
    r.c1 = 0.0;
    r.finite = true;
    float lv = 0.f, var = 0.f, iv = 0.f, hs = 0.f;
    if (!LvPerMember) {
        lv = q[0];
        iv = expf(-lv), hs = expf(-0.5f * lv);
        var = expf(lv);
    }
    float acc = 0.f, pacc = 0.f, vacc = 0.f;
    float mx = -INFINITY, ssum = 0.f;                              // streaming logsumexp over the members
    for (int m = 0; m < S; m += 4) {
        float v[4], u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long s = min(m + k, S - 1);
            v[k] = p[s * ms];
            if (LvPerMember) u[k] = q[s * ls];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (m + k >= S) break;
            const float x = v[k];
            r.finite = r.finite && isfinite(x);
            acc = (m + k == 0) ? x : acc + x;                      // the stated order: m_0, then += m_s
            if (LvPerMember) {
                lv = u[k];
                var = expf(lv), iv = expf(-lv), hs = expf(-0.5f * lv);
                vacc = (m + k == 0) ? var : vacc + var;
            }
            const float d = y - x;
            const float t = -0.5f * ((kLog2Pi + lv) + (d * d) * iv);
            if (t > mx) {
                ssum = ssum * expf(mx - t) + 1.f;
                mx = t;
            } else if (t != -INFINITY) {
                ssum += expf(t - mx);                              // (a NaN term arrives here and stays)
            }
            const float ph = 0.5f * erfcf(-((d * hs) * kRsqrt2));
            pacc = (m + k == 0) ? ph : pacc + ph;
            if (Crps) r.c1 += (double)a_term(d, var);
        }
    }
    r.pm = acc / (float)S;                                         // IEEE division (hipcc's default)
    float acc2 = 0.f;
    for (int m = 0; m < S; m += 4) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p[(long long)min(m + k, S - 1) * ms];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (m + k >= S) break;
            const float d = v[k] - r.pm;
            acc2 = (m + k == 0) ? d * d : acc2 + d * d;
        }
    }
    r.ev = acc2 / (float)S;
    r.av = LvPerMember ? vacc / (float)S : var;
    r.ld = (mx + logf(ssum)) - logf((float)S);
    r.pit = pacc / (float)S;
    return r;
}

}  // namespace lbbnn
