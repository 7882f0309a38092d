// The element backward of the fused weight pass: the gradients of one weight (mu, rho, lambda) and its contributions to the
// three column sums (dz_fwd, dz_kl, dr0_c).  Shared by weight_pass_bwd.hip (K1b) and the MNF replicates of lrt_study.hip.
#pragma once
#include "lbbnn_device.h"

namespace lbbnn {

struct ElemConsts { float mp, inv_sp2, log_sp, log_ap, log_1map, gk; };

// gradients of one weight; returns dmu, drho, dlam and the three column-sum contributions
__device__ __forceinline__ void elem_bwd(float mu, float rho, float lam, float gWm, float gWv, float zf, float zk, float rc,
                                         float dam, float dav, const ElemConsts& c, bool has_kl, bool has_act,
                                         float& dmu, float& drho, float& dlam, float& czf, float& czk, float& crc) {
    // the forward's own forms (lbbnn_device.h k1_*: raw v_exp / v_rcp / v_log, no denormal scaling, no cancellation)
    const float ex = k1_exp_raw(-lam);
    const float ope = 1.f + ex;
    const float alpha = __builtin_amdgcn_rcpf(ope);
    const float er = k1_exp_acc(rho);
    const float sigma = k1_sigma_of(er);
    const float dsig = er * __builtin_amdgcn_rcpf(1.f + er);  // d softplus / d rho = sigmoid(rho)
    const float a2 = alpha * alpha, s2 = sigma * sigma;
    float Gmu = gWm * alpha * zf;
    float Gsig = gWv * 2.f * sigma * a2;
    float Gal = gWm * mu * zf + gWv * 2.f * s2 * alpha;
    czf = gWm * mu * alpha;
    czk = 0.f; crc = 0.f;
    if (has_kl) {
        const float d = mu * zk - c.mp;
        const float la = -0.6931471805599453f * __builtin_amdgcn_logf(ope);       // log(alpha) = -log(1 + exp(-lambda))
        const float T = (c.log_sp - k1_log_sigma_of(rho, er, sigma)) - 0.5f + (la - c.log_ap) + (s2 + d * d) * 0.5f * c.inv_sp2;
        Gmu += c.gk * alpha * d * zk * c.inv_sp2;
        Gsig += c.gk * alpha * (sigma * c.inv_sp2 - __builtin_amdgcn_rcpf(sigma));
        Gal += c.gk * (T - ((la - lam) - c.log_1map));                             // log(1 - alpha) = log(alpha) - lambda
        czk = c.gk * alpha * d * mu * c.inv_sp2;
    }
    if (has_act) {
        const float ma = mu * alpha;
        Gmu += dam * rc * zk * alpha;
        Gal += dam * rc * zk * mu + dav * rc * rc * 2.f * s2 * alpha;
        Gsig += dav * rc * rc * 2.f * sigma * a2;
        czk += dam * rc * ma;
        crc = dam * zk * ma + dav * 2.f * rc * s2 * a2;
    }
    dmu = Gmu;
    drho = Gsig * dsig;
    dlam = Gal * alpha * (1.f - alpha);
}

}  // namespace lbbnn
