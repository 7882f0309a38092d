// K6 (baseline LBBNN gate x Gaussian weight sampling + Monte-Carlo log-probabilities) and
// K7 (variational-dropout operand pass) -- see include/lbbnn.h.  Both are one-pass HBM-bound kernels
// that feed the same dual-moment GEMM.  What they store goes out in the one operand layout of operand_store.h, which also
// holds the scalar bf16 split (bf16_hi_lo), uniform24 and gate_draw that the frozen baseline model (base_frozen.hip) shares.
#include <climits>
#include <cmath>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "operand_store.h"

namespace {

using namespace lbbnn;

// store one operand value at [o][i] either as fp32 or in the split bf16 hi|lo layout
// split: 0 = fp32, 1 = bf16 hi|lo (LBBNN_F_SPLIT16), 2 = fp16 in the hi unit, zero lo (LBBNN_F_HALF16: the single-product
// fp16 form of the variational-dropout operands)
__device__ __forceinline__ void store_operand(void* base, int split, size_t O, int ld, int o, int i, float v) {
    if (!split) { static_cast<float*>(base)[(size_t)o * ld + i] = v; return; }
    uint16_t* const w = static_cast<uint16_t*>(base);           // split hi|lo layout (lbbnn_device.h)
    const size_t at = split_hi_index((size_t)o, i, ld);
    if (split == 2) {
        const _Float16 h16 = (_Float16)v;                       // RNE; subnormals kept (the f16 MFMA honours them)
        w[at] = __builtin_bit_cast(uint16_t, h16);
        w[at + kSplitLoOffset] = 0;
        (void)O;
        return;
    }
    const uint32_t hl = bf16_hi_lo(v);
    w[at] = (uint16_t)hl;
    w[at + kSplitLoOffset] = (uint16_t)(hl >> 16);
    (void)O;
}


// ------------------------------------------------------------------------------------------------ in-kernel draws of K6 / K6b
// (lbbnn_gate_sample_draw / lbbnn_gate_backward_draw, include/lbbnn.h)
__device__ __forceinline__ float gate_u(uint64_t seed, uint64_t offs, uint32_t layer, int o, int i) {
    const Philox4 r = philox_bits4(seed, offs, LBBNN_STREAM_GATE * 64u + layer, (uint64_t)o, (uint32_t)(i >> 2));
    const uint32_t b = (i & 3) == 0 ? r.x : (i & 3) == 1 ? r.y : (i & 3) == 2 ? r.z : r.w;
    return uniform24(b);
}

// Standard Gamma(a) of element `e` (Marsaglia & Tsang, ACM TOMS 26(3), 2000): attempt k uses Philox counter (e, k) -- one
// normal (Box-Muller on words x, y, the same hardware forms as philox_normal4), the acceptance uniform (z) and, for a < 1,
// the boost uniform U^(1/a) of the accepted attempt (w).  At most LBBNN_GAMMA_MAX_ATTEMPTS attempts (one is rejected with
// probability < 0.05 for every a, so the bound is never reached in practice; if it were, the draw would be the mode-like
// d = a' - 1/3).  NaN, non-positive or infinite a: NaN.
__device__ __forceinline__ float std_gamma_draw(float a, uint64_t seed, uint64_t offs, uint32_t stream, uint64_t e) {
    if (!(a > 0.f) || !(a < INFINITY)) return __builtin_nanf("");
    const bool boost = a < 1.f;
    const float ap = boost ? a + 1.f : a;
    const float d = ap - 0.33333334f, c = 1.f / sqrtf(9.f * d);
    float x = d, ub = 1.f;
    for (int k = 0; k < LBBNN_GAMMA_MAX_ATTEMPTS; ++k) {
        const Philox4 r = philox_bits4(seed, offs, stream, e, (uint32_t)k);
        const float u0 = ((float)r.x + 1.0f) * 2.3283064365386963e-10f, u1 = (float)r.y * 2.3283064365386963e-10f;
        const float n = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u0)) * __builtin_amdgcn_cosf(u1);
        const float w = c * n;
        if (w <= -1.f) continue;
        const float v = (1.f + w) * (1.f + w) * (1.f + w);
        if (logf(uniform24(r.z)) < 0.5f * n * n + d * ((1.f - v) + 3.f * log1pf(w))) {
            x = d * v;
            ub = uniform24(r.w);
            break;
        }
    }
    if (boost) x *= expf(logf(ub) / a);
    return x;
}
// Gamma(a, rate) as torch's Gamma.rsample returns it: standard draw / rate, clamped below at FLT_MIN (NaN stays NaN)
__device__ __forceinline__ float gamma_rate_draw(float a, float rate, uint64_t seed, uint64_t offs, uint32_t stream, uint64_t e) {
    const float t = std_gamma_draw(a, seed, offs, stream, e) / rate;
    return (t < kTiny) ? kTiny : t;
}

__device__ __forceinline__ double digamma_d(double x) {
    double r = 0.0;
    for (int k = 0; k < 16 && x < 10.0; ++k) { r -= 1.0 / x; x += 1.0; }
    const double i = 1.0 / x, i2 = i * i;
    return r + log(x) - 0.5 * i - i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132)))));
}
// g(x, a) = dx/da of the standard Gamma draw = -(dP(a, x)/da) / f(x; a).  From P(a, x) = e^-x sum_n x^(a+n) / Gamma(a+n+1):
// dP/da = e^-x sum_n x^(a+n) / Gamma(a+n+1) (log x - psi(a+n+1)), and the n-th term over f is (x/a) s_n with s_0 = 1,
// s_n = s_(n-1) x / (a+n) -- no exp / lgamma, no underflow.  fp64; the terms change sign once, so the relative error is about
// 1e-16 / Q(a, x) (Q = 1 - P): far-right-tail x lose digits, x with Q > 1e-9 keep at least seven.
__device__ __forceinline__ float gamma_grad_one(float xf, float af) {
    if (!(af > 0.f) || !(af < INFINITY) || xf != xf) return __builtin_nanf("");
    if (!(xf > 0.f)) return 0.f;
    const double x = xf, a = af, lx = log(x);
    double psi = digamma_d(a + 1.0), s = 1.0;
    double sum = lx - psi, mag = fabs(sum);
    for (int n = 1; n < 8192; ++n) {
        psi += 1.0 / (a + n);
        s *= x / (a + n);
        const double t = s * (lx - psi);
        sum += t;
        mag += fabs(t);
        if (x < a + n && fabs(t) <= 1e-17 * mag) break;
    }
    return (float)(-(x / a) * sum);
}

// ------------------------------------------------------------------------------------------------ K6
// One workgroup per output row; rows[0..3][o] = row sums of
//   0: GaussGamma weight integrand (without the scalar C*gamma part folded: kept exact as the reference sums it)
//   1: BetaBinomial integrand      2: Gaussian.full_log_prob integrand     3: Bernoulli.log_prob integrand
template <bool DRAW>
__global__ __launch_bounds__(256) void gate_sample_kernel(const lbbnn_gate_draw_args_t dr, const uint64_t* rng) {
    const lbbnn_gate_args_t& a = dr.g;
    __shared__ double red[4][4];
    const int o = blockIdx.x, tid = threadIdx.x;
    const size_t ro = (size_t)o * a.I;
    const int split = (a.flags & LBBNN_F_SPLIT16) ? 1 : 0;
    uint64_t seed = 0, offs = 0;
    if (DRAW || (a.mode == LBBNN_MODE_SAMPLE && !a.eps_w)) { seed = rng[0]; offs = rng[1]; }
    float C = 0.f, cbb = 0.f, pa = 0.f, pb = 0.f, tau = 0.f;
    if (a.want_lp) {
        const float wa = a.weight_a[0], wb = a.weight_b[0];
        if (DRAW) {
            // every workgroup draws the same tau_w (a deterministic function of the state): no launch ahead of this one
            tau = gamma_rate_draw(wa, wb, seed, offs, LBBNN_STREAM_GAMMA_W * 64u + a.layer_id, 0);
            if (o == 0 && tid == 0) dr.tau_w[0] = tau;
        } else {
            tau = a.tau_w[0];
        }
        // a*log(b) + (a-0.5)*tau - b*tau - lgamma(a) - 0.5*log(2*pi)      LBBNN-GP-MF.py:144-145
        C = wa * logf(wb) + (wa - 0.5f) * tau - wb * tau - lgammaf(wa) - 0.5f * 1.8378770664093453f;
        pa = a.pa[0]; pb = a.pb[0];
        // lgamma(1) + lgamma(pa+pb) - lgamma(1+pa+pb) - lgamma(pa) - lgamma(pb)   (the g-independent terms of :167-173)
        cbb = lgammaf(pa + pb) - lgammaf(1.f + pa + pb) - lgammaf(pa) - lgammaf(pb);
    }
    double s_gg = 0.0, s_bb = 0.0, s_fq = 0.0, s_be = 0.0;
    for (int i = tid; i < a.ld; i += 256) {
        float w = 0.f;
        if (i < a.I) {
            const float mu = a.mu[ro + i];
            float g, al = 0.f;
            if (DRAW) {
                al = sigmoid_ref(dr.lambdal[ro + i]);
                float dcda;
                g = gate_draw(al, gate_u(seed, offs, a.layer_id, o, i), dr.temperature, (a.exact & 8) != 0, &dcda);
                dr.gammas[ro + i] = g;
                if (dr.alpha) dr.alpha[ro + i] = al;
            } else {
                g = a.cgamma ? a.cgamma[ro + i] : 1.f;
            }
            float sigma = 0.f;
            if (a.mode == LBBNN_MODE_SAMPLE) {
                float e;
                if (a.eps_w) e = a.eps_w[ro + i];
                else { float n[4]; philox_normal4(seed, offs, LBBNN_STREAM_EPS_W * 64u + a.layer_id, (uint64_t)o, (uint32_t)(i >> 2), n); e = n[i & 3]; }
                sigma = softplus_ref(a.rho[ro + i]);
                w = g * (mu + sigma * e);                                          // :232-233
            } else if (a.mode == LBBNN_MODE_MEDIMEAN) {
                w = g * mu;                                                        // :237
            } else {
                w = a.alpha_attr[ro + i] * mu;                                     // :241
            }
            if (a.want_lp) {
                if (a.mode != LBBNN_MODE_SAMPLE) sigma = softplus_ref(a.rho[ro + i]);
                const float g_wp = (a.exact & 1) ? rintf(g) : g;
                s_gg += (double)(g_wp * C - tau * (w * w) + (1.f - g_wp) + 1e-8f);                  // :144-150
                const float g_bb = (a.exact & 4) ? rintf(g) : g;
                s_bb += (double)(cbb + lgammaf(1.f + pb - g_bb) - lgammaf(2.f - g_bb));              // :167-173
                const float d = w - mu;
                const float lp = -0.9189385332046727f - logf(sigma) - (d * d) / (2.f * sigma * sigma);   // :94-97
                s_fq += (double)logf(g * expf(lp) + (1.f - g) + 1e-8f);                              // :99-101
                if (!DRAW) al = a.gamma_alpha[ro + i];
                const float g_be = (a.exact & 8) ? rintf(g) : g;
                s_be += (double)(g_be * logf(al + 1e-8f) + (1.f - g_be) * logf(1.f - al + 1e-8f));   // :125-127
            }
        }
        if (a.w_out) store_operand(a.w_out, split, a.O, a.ld, o, i, w);
    }
    if (a.want_lp) {
        s_gg = wave_sum(s_gg); s_bb = wave_sum(s_bb); s_fq = wave_sum(s_fq); s_be = wave_sum(s_be);
        const int lane = tid & 63, wv = tid >> 6;
        if (lane == 0) { red[0][wv] = s_gg; red[1][wv] = s_bb; red[2][wv] = s_fq; red[3][wv] = s_be; }
        __syncthreads();
        if (tid < 4) a.rows[(size_t)tid * a.O + o] = (float)((red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]));
    }
}

// bias sample + bias log-probabilities + final scalars (single workgroup)
template <bool DRAW>
__global__ __launch_bounds__(256) void gate_finalize_kernel(const lbbnn_gate_draw_args_t dr, const uint64_t* rng) {
    const lbbnn_gate_args_t& a = dr.g;
    __shared__ double scratch[4];
    const int tid = threadIdx.x;
    uint64_t seed = 0, offs = 0;
    if (DRAW || (a.mode == LBBNN_MODE_SAMPLE && !a.eps_b)) { seed = rng[0]; offs = rng[1]; }
    double r0 = 0, r1 = 0, r2 = 0, r3 = 0, gb = 0, qb = 0;
    for (int o = tid; o < a.O; o += 256) {
        const float sb = softplus_ref(a.bias_rho[o]);
        float b = a.bias_mu[o];
        if (a.mode == LBBNN_MODE_SAMPLE) {
            float e;
            if (a.eps_b) e = a.eps_b[o];
            else { float n[4]; philox_normal4(seed, offs, LBBNN_STREAM_EPS_B * 64u + a.layer_id, (uint64_t)(o >> 2), 0u, n); e = n[o & 3]; }
            b = a.bias_mu[o] + sb * e;                                                                // :234
        }
        a.bias_out[o] = b;
        if (a.want_lp) {
            r0 += (double)a.rows[o]; r1 += (double)a.rows[(size_t)a.O + o];
            r2 += (double)a.rows[2 * (size_t)a.O + o]; r3 += (double)a.rows[3 * (size_t)a.O + o];
            const float ba = a.bias_a[o], bb = a.bias_b[o];
            float tb;
            if (DRAW) { tb = gamma_rate_draw(ba, bb, seed, offs, LBBNN_STREAM_GAMMA_B * 64u + a.layer_id, (uint64_t)o); dr.tau_b[o] = tb; }
            else tb = a.tau_b[o];
            const float Cb = ba * logf(bb) + (ba - 0.5f) * tb - bb * tb - lgammaf(ba) - 0.5f * 1.8378770664093453f;
            gb += (double)(Cb - tb * (b * b) + 0.f + 1e-8f);                                          // GaussGamma(bias, 1)
            const float d = b - a.bias_mu[o];
            qb += (double)(-0.9189385332046727f - logf(sb) - (d * d) / (2.f * sb * sb));              // Gaussian.log_prob :89-92
        }
    }
    if (!a.want_lp) return;
    r0 = block_sum<double, 4>(r0, scratch); r1 = block_sum<double, 4>(r1, scratch);
    r2 = block_sum<double, 4>(r2, scratch); r3 = block_sum<double, 4>(r3, scratch);
    gb = block_sum<double, 4>(gb, scratch); qb = block_sum<double, 4>(qb, scratch);
    if (tid == 0) {
        *a.log_prior = (float)(r0 + gb + r1);          // :247-249
        *a.log_q = (float)(r2 + r3 + qb);              // :250-251
    }
}

// ------------------------------------------------------------------------------------------------ K6b
// Backward of the sampled baseline layer (LBBNN-GP-MF.py:228-255 under loss.backward(), :331-337): one pass over (O,I)
// turns the upstream gradients -- dW = G^T x of F.linear (:255), and the scalars g_lp = dL/dlog_prior, g_lq = dL/dlog_q --
// into d weight_mu, d weight_rho, d cgamma, d gamma.alpha and the row sums the scalar parameters need; a single-workgroup
// tail adds those up (weight_a, weight_b, tau_w, pa, pb) and does the (O)-sized bias chain.  Also rewrites the sampled
// weight W as a dense fp32 (O,I) matrix for the dX product.  eps_w / eps_b are re-created from the forward's Philox state.
// psi = digamma by upward recurrence to x >= 6 and the asymptotic series (|error| < 1e-6 for x >= 0.5).
__device__ __forceinline__ float digammaf_pos(float x) {
    float r = 0.f;
#pragma unroll 1
    while (x < 6.f) { r -= 1.f / x; x += 1.f; }
    const float i = 1.f / x, i2 = i * i;
    return r + logf(x) - 0.5f * i - i2 * (0.083333333f - i2 * (0.0083333333f - i2 * 0.003968254f));
}

struct GateScal { float C, tau, pa, pb, glp, glq; };

template <bool DRAW>
__global__ __launch_bounds__(256) void gate_backward_kernel(const lbbnn_gate_bwd_draw_args_t dr, const uint64_t* rng) {
    const lbbnn_gate_bwd_args_t& a = dr.g;
    __shared__ double red[3][4];
    const int o = blockIdx.x, tid = threadIdx.x;
    const size_t ro = (size_t)o * a.I;
    uint64_t seed = 0, offs = 0;
    if (DRAW || !a.eps_w) { seed = rng[0]; offs = rng[1]; }
    const float wa = a.weight_a[0], wb = a.weight_b[0], tau = a.tau_w[0], pb = a.pb[0];
    const float C = wa * logf(wb) + (wa - 0.5f) * tau - wb * tau - lgammaf(wa) - 0.5f * 1.8378770664093453f;
    const float glp = a.g_lp ? a.g_lp[0] : 0.f, glq = a.g_lq ? a.g_lq[0] : 0.f;
    double s_c = 0.0, s_w2 = 0.0, s_psi = 0.0;
    for (int i = tid; i < a.I; i += 256) {
        const float mu = a.mu[ro + i];
        float g, al, dcda = 0.f;
        if (DRAW) {
            al = sigmoid_ref(dr.lambdal[ro + i]);                 // the forward's alpha and gate, bit for bit
            g = gate_draw(al, gate_u(seed, offs, a.layer_id, o, i), dr.temperature, (a.exact & 8) != 0, &dcda);
        } else {
            g = a.cgamma[ro + i];
            al = a.gamma_alpha[ro + i];
        }
        float e;
        if (a.eps_w) e = a.eps_w[ro + i];
        else { float n[4]; philox_normal4(seed, offs, LBBNN_STREAM_EPS_W * 64u + a.layer_id, (uint64_t)o, (uint32_t)(i >> 2), n); e = n[i & 3]; }
        const float rho = a.rho[ro + i];
        const float sigma = softplus_ref(rho);
        const float ws = mu + sigma * e, w = g * ws;
        if (a.w_out) a.w_out[ro + i] = w;
        const float d = w - mu, is2 = 1.f / (sigma * sigma);
        const float lp = -0.9189385332046727f - logf(sigma) - (d * d) * 0.5f * is2;
        const float E = expf(lp), D = g * E + (1.f - g) + 1e-8f;
        const float q = glq * (g * E / D);                         // g_lq * d full_log_prob / d lp
        const float A = (a.dW ? a.dW[ro + i] : 0.f) + glp * (-2.f * tau * w) + q * (-d * is2);       // dL/dW
        const float g_wp = (a.exact & 1) ? rintf(g) : g, g_bb = (a.exact & 4) ? rintf(g) : g, g_be = (a.exact & 8) ? rintf(g) : g;
        float dg = A * ws + glq * ((E - 1.f) / D);
        if (!(a.exact & 1)) dg += glp * (C - 1.f);
        const float psi1 = digammaf_pos(1.f + pb - g_bb);
        if (!(a.exact & 4)) dg += glp * (-psi1 + digammaf_pos(2.f - g_bb));
        if (!(a.exact & 8)) dg += glq * (logf(al + 1e-8f) - logf(1.f - al + 1e-8f));
        const float dws = A * g;
        a.d_mu[ro + i] = dws + q * (d * is2);
        const float dsig = dws * e + q * (-1.f / sigma + (d * d) * is2 / sigma);
        a.d_rho[ro + i] = dsig / (1.f + expf(-rho));
        const float dal = glq * (g_be / (al + 1e-8f) - (1.f - g_be) / (1.f - al + 1e-8f));
        if (DRAW) {
            dr.d_lambdal[ro + i] = (al * (1.f - al)) * (dal + dg * dcda);   // alpha = sigmoid(lambdal) feeds both
        } else {
            a.d_cgamma[ro + i] = dg;
            a.d_alpha[ro + i] = dal;
        }
        s_c += (double)g_wp; s_w2 += (double)(w * w); s_psi += (double)psi1;
    }
    s_c = wave_sum(s_c); s_w2 = wave_sum(s_w2); s_psi = wave_sum(s_psi);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) { red[0][wv] = s_c; red[1][wv] = s_w2; red[2][wv] = s_psi; }
    __syncthreads();
    if (tid < 3) a.rows[(size_t)tid * a.O + o] = (float)((red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]));
}

template <bool DRAW>
__global__ __launch_bounds__(256) void gate_backward_tail_kernel(const lbbnn_gate_bwd_draw_args_t dr, const uint64_t* rng) {
    const lbbnn_gate_bwd_args_t& a = dr.g;
    __shared__ double scratch[4];
    const int tid = threadIdx.x;
    uint64_t seed = 0, offs = 0;
    if (!a.eps_b) { seed = rng[0]; offs = rng[1]; }
    const float glp = a.g_lp ? a.g_lp[0] : 0.f, glq = a.g_lq ? a.g_lq[0] : 0.f;
    double r0 = 0, r1 = 0, r2 = 0;
    for (int o = tid; o < a.O; o += 256) {
        r0 += (double)a.rows[o]; r1 += (double)a.rows[(size_t)a.O + o]; r2 += (double)a.rows[2 * (size_t)a.O + o];
        const float rho = a.bias_rho[o], sb = softplus_ref(rho), bm = a.bias_mu[o];
        float e;
        if (a.eps_b) e = a.eps_b[o];
        else { float n[4]; philox_normal4(seed, offs, LBBNN_STREAM_EPS_B * 64u + a.layer_id, (uint64_t)(o >> 2), 0u, n); e = n[o & 3]; }
        const float b = bm + sb * e, d = b - bm, is2 = 1.f / (sb * sb);
        const float ba = a.bias_a[o], bb = a.bias_b[o], tb = a.tau_b[o];
        const float db = (a.g_sum ? a.g_sum[o] : 0.f) + glp * (-2.f * tb * b) + glq * (-d * is2);      // dL/db
        a.d_bias_mu[o] = db + glq * (d * is2);
        a.d_bias_rho[o] = (db * e + glq * (-1.f / sb + (d * d) * is2 / sb)) / (1.f + expf(-rho));
        const float dtb = glp * ((ba - 0.5f) - bb - b * b);
        if (DRAW) {
            // tau_b = x / b with x ~ Gamma(a, 1): d tau / d a = g(x, a) / b, d tau / d b = -tau / b
            a.d_bias_a[o] = glp * (logf(bb) + tb - digammaf_pos(ba)) + dtb * (gamma_grad_one(tb * bb, ba) / bb);
            a.d_bias_b[o] = glp * (ba / bb - tb) - dtb * (tb / bb);
            if (a.d_tau_b) a.d_tau_b[o] = dtb;
        } else {
            a.d_bias_a[o] = glp * (logf(bb) + tb - digammaf_pos(ba));
            a.d_bias_b[o] = glp * (ba / bb - tb);
            a.d_tau_b[o] = dtb;
        }
    }
    r0 = block_sum<double, 4>(r0, scratch); r1 = block_sum<double, 4>(r1, scratch); r2 = block_sum<double, 4>(r2, scratch);
    if (tid == 0) {
        const float wa = a.weight_a[0], wb = a.weight_b[0], tau = a.tau_w[0], pa = a.pa[0], pb = a.pb[0];
        const double N = (double)a.O * (double)a.I;
        const float dtw = glp * (float)(r0 * (double)((wa - 0.5f) - wb) - r1);                         // d tau_w
        a.d_scalars[0] = glp * (float)(r0 * (double)(logf(wb) + tau - digammaf_pos(wa)));             // d weight_a
        a.d_scalars[1] = glp * (float)(r0 * (double)(wa / wb - tau));                                 // d weight_b
        if (DRAW) {
            a.d_scalars[0] += dtw * (gamma_grad_one(tau * wb, wa) / wb);
            a.d_scalars[1] -= dtw * (tau / wb);
        }
        a.d_scalars[2] = dtw;
        const float common = digammaf_pos(pa + pb) - digammaf_pos(1.f + pa + pb);
        a.d_scalars[3] = glp * (float)(N * (double)(common - digammaf_pos(pa)));                      // d pa
        a.d_scalars[4] = glp * (float)(r2 + N * (double)(common - digammaf_pos(pb)));                 // d pb
    }
}

// ------------------------------------------------------------------------------------------------ K6e
// lbbnn_gate_members (include/lbbnn.h): the sampled operands of every layer and every ensemble member in one launch.  One
// workgroup per output row (rows of all layers concatenated); a thread owns up to kGmGroups groups of 8 consecutive k, keeps
// mu, sigma and alpha of them in registers, then loops over the members.  Per member and group: two Philox calls for the four
// normals of each quad (the training kernel computes four and uses one), two for the gate uniforms (SAMPLE), and 32 B of
// operand written as two float4 (fp32) or one 16-B hi unit + one 16-B lo unit (split layout, lbbnn_device.h).  The
// expressions are those of gate_sample_kernel<true> / gate_finalize_kernel<true>, so the operands are bitwise theirs.
// G (template): groups per thread, the smallest of 1, 2, 4 that covers the widest layer (register footprint ~ 24 G floats)
constexpr int kGmThreads = 128;
constexpr int kGmMaxLd = kGmThreads * 4 * 8;   // 4096

struct GateMembersLaunch {
    lbbnn_gate_member_desc_t l[LBBNN_MAX_LAYERS];
    int row0[LBBNN_MAX_LAYERS], row_end[LBBNN_MAX_LAYERS];   // blockIdx.x range of each layer (unused layers: INT_MAX)
    int vec[LBBNN_MAX_LAYERS];                               // (O,I) inputs readable as float4
    int members, gates;
    float temperature;
    uint64_t member_advance;
};

template <int kGmGroups>
__global__ __launch_bounds__(kGmThreads) void gate_members_kernel(const GateMembersLaunch ga, const uint64_t* rng) {
    __shared__ float red[2][kGmThreads / 64];
    const int bx = blockIdx.x;
    const int li = (bx >= ga.row_end[0]) + (bx >= ga.row_end[1]) + (bx >= ga.row_end[2]);
    lbbnn_gate_member_desc_t L;
    LBBNN_SELECT_LAYER(L, ga.l, li);
    int row0, vec;
    LBBNN_SELECT_LAYER(row0, ga.row0, li);
    LBBNN_SELECT_LAYER(vec, ga.vec, li);
    const int o = bx - row0, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t ro = (size_t)o * L.I;
    const bool sample = ga.gates == LBBNN_GATES_SAMPLE, hard = (L.exact & 8) != 0;
    const uint64_t seed = rng[0], off0 = rng[1];
    const uint32_t s_gate = LBBNN_STREAM_GATE * 64u + L.layer_id, s_w = LBBNN_STREAM_EPS_W * 64u + L.layer_id;

    float mu[kGmGroups][8], sg[kGmGroups][8], al[kGmGroups][8];
#pragma unroll
    for (int gi = 0; gi < kGmGroups; ++gi) {
        const int i0 = 8 * (tid + gi * kGmThreads);
        float r[8], lam[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { mu[gi][e] = 0.f; r[e] = 0.f; lam[e] = 0.f; }
        if (i0 < L.I) {
            if (vec) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if (i0 + 4 * q >= L.I) continue;                      // I % 4 == 0: a quad is wholly in or out
                    const float4 m4 = *reinterpret_cast<const float4*>(L.mu + ro + i0 + 4 * q);
                    const float4 r4 = *reinterpret_cast<const float4*>(L.rho + ro + i0 + 4 * q);
                    const float4 l4 = *reinterpret_cast<const float4*>(L.lambdal + ro + i0 + 4 * q);
                    mu[gi][4 * q] = m4.x; mu[gi][4 * q + 1] = m4.y; mu[gi][4 * q + 2] = m4.z; mu[gi][4 * q + 3] = m4.w;
                    r[4 * q] = r4.x; r[4 * q + 1] = r4.y; r[4 * q + 2] = r4.z; r[4 * q + 3] = r4.w;
                    lam[4 * q] = l4.x; lam[4 * q + 1] = l4.y; lam[4 * q + 2] = l4.z; lam[4 * q + 3] = l4.w;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (i0 + e < L.I) { mu[gi][e] = L.mu[ro + i0 + e]; r[e] = L.rho[ro + i0 + e]; lam[e] = L.lambdal[ro + i0 + e]; }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { sg[gi][e] = softplus_ref(r[e]); al[gi][e] = sigmoid_ref(lam[e]); }
    }

    // the member biases: thread t draws those of members t, t + kGmThreads, ...
    if (tid < ga.members) {
        const float sb = softplus_ref(L.bias_rho[o]), bm = L.bias_mu[o];
        for (int m = tid; m < ga.members; m += kGmThreads) {
            float n[4];
            philox_normal4(seed, off0 + (uint64_t)m * ga.member_advance, LBBNN_STREAM_EPS_B * 64u + L.layer_id,
                           (uint64_t)(o >> 2), 0u, n);
            const float e = n[o & 3];
            L.bias_out[(size_t)m * L.O + o] = bm + sb * e;                                   // :234
        }
    }

    const size_t w_ms = (size_t)L.O * L.ld;                  // member stride in 4-byte units (fp32 and split rows alike)
    for (int m = 0; m < ga.members; ++m) {
        const uint64_t offs = off0 + (uint64_t)m * ga.member_advance;
        float gsum = 0.f;
#pragma unroll
        for (int gi = 0; gi < kGmGroups; ++gi) {
            const int i0 = 8 * (tid + gi * kGmThreads);
            if (i0 >= L.ld) continue;
            float w[8], c[8];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int iq = i0 + 4 * q;
                if (iq >= L.I) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { w[4 * q + e] = 0.f; c[4 * q + e] = 0.f; }
                    continue;
                }
                float n[4], u[4] = {0.f, 0.f, 0.f, 0.f};
                philox_normal4(seed, offs, s_w, (uint64_t)o, (uint32_t)(iq >> 2), n);
                if (sample) {
                    const Philox4 r = philox_bits4(seed, offs, s_gate, (uint64_t)o, (uint32_t)(iq >> 2));
                    u[0] = uniform24(r.x); u[1] = uniform24(r.y); u[2] = uniform24(r.z); u[3] = uniform24(r.w);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * q + e;
                    float g = 0.f, v = 0.f;
                    if (iq + e < L.I) {
                        float dcda;
                        g = sample ? gate_draw(al[gi][k], u[e], ga.temperature, hard, &dcda) : (al[gi][k] > 0.5f ? 1.f : 0.f);
                        const float sigma = sg[gi][k], mu_k = mu[gi][k], ek = n[e];
                        v = g * (mu_k + sigma * ek);                                            // :232-233
                    }
                    w[k] = v; c[k] = g;
                    gsum += g;
                }
            }
            // store8_operand of operand_store.h at member m, spelled out: through the call the kernel does not compile to the
            // same instructions (it runs in every live ensemble)
            if (L.flags & LBBNN_F_SPLIT16) {
                uint32_t hl[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) hl[k] = bf16_hi_lo(w[k]);
                uint16_t* const p = static_cast<uint16_t*>(L.w_out) + 2 * (m * w_ms) + split_hi_index((size_t)o, i0, L.ld);
                *reinterpret_cast<uint4*>(p) = make_uint4((hl[0] & 0xFFFFu) | (hl[1] << 16), (hl[2] & 0xFFFFu) | (hl[3] << 16),
                                                          (hl[4] & 0xFFFFu) | (hl[5] << 16), (hl[6] & 0xFFFFu) | (hl[7] << 16));
                *reinterpret_cast<uint4*>(p + kSplitLoOffset) =
                    make_uint4((hl[0] >> 16) | (hl[1] & 0xFFFF0000u), (hl[2] >> 16) | (hl[3] & 0xFFFF0000u),
                               (hl[4] >> 16) | (hl[5] & 0xFFFF0000u), (hl[6] >> 16) | (hl[7] & 0xFFFF0000u));
            } else {
                float* const p = static_cast<float*>(L.w_out) + m * w_ms + (size_t)o * L.ld + i0;
                *reinterpret_cast<float4*>(p) = make_float4(w[0], w[1], w[2], w[3]);
                *reinterpret_cast<float4*>(p + 4) = make_float4(w[4], w[5], w[6], w[7]);
            }
            if (L.gates) {
                float* const p = L.gates + (size_t)m * L.O * L.I + ro;
#pragma unroll
                for (int k = 0; k < 8; ++k) if (i0 + k < L.I) p[i0 + k] = c[k];
            }
        }
        if (L.gate_rows) {                                    // uniform: per-member row sum, fixed order (lanes, then waves)
            const float s = wave_sum(gsum);
            if (lane == 0) red[m & 1][wv] = s;
            __syncthreads();                                  // (double buffer: one barrier per member)
            if (tid == 0) L.gate_rows[(size_t)m * L.O + o] = red[m & 1][0] + red[m & 1][1];
        }
    }
}

// ------------------------------------------------------------------------------------------------ K7
// 32x32 tiles of theta (I,O) through LDS: coalesced reads along O, coalesced writes along I.
__global__ __launch_bounds__(256) void vd_operands_kernel(const float* __restrict__ theta, void* e_w, void* var_w,
                                                          int ld, int I, int O, int split) {
    __shared__ float tile[32][33];
    const int i0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty + 8 * r, o = o0 + tx;
        tile[ty + 8 * r][tx] = (i < I && o < O) ? theta[(size_t)i * O + o] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + ty + 8 * r, i = i0 + tx;
        if (o < O && i < ld) {
            const float t = tile[tx][ty + 8 * r];                // zero for i >= I: keeps the operand tail zero-filled
            store_operand(e_w, split, O, ld, o, i, t);
            store_operand(var_w, split, O, ld, o, i, t * t);
        }
    }
}

// Backward operands of a Bayesian layer in ONE pass over its parameters: (e_w)^T = (mu * alpha * z)^T and
// (var_w)^T = (sigma^2 alpha^2)^T as GEMM operands [I][ld(O)] (the dX products contract over O) -- instead of the weight
// pass (fp32 operands) followed by two transposes.  Same tiling as K7; same elementwise forms as the weight pass.
__global__ __launch_bounds__(256) void weight_operands_t_kernel(const float* __restrict__ mu, const float* __restrict__ rho,
                                                                const float* __restrict__ lam, const float* __restrict__ z,
                                                                void* e_t, void* v_t, int ld, int O, int I, int split) {
    __shared__ float te[32][33], tv[32][33];
    const int o0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + ty + 8 * r, i = i0 + tx;
        float e = 0.f, v = 0.f;
        if (o < O && i < I) {
            const size_t k = (size_t)o * I + i;
            const float alpha = k1_alpha(lam[k]);
            e = (mu[k] * alpha) * (z ? z[i] : 1.f);                                  // same association as the weight pass
            if (v_t) { const float sg = k1_sigma(rho[k]); v = (sg * sg) * (alpha * alpha); }
        }
        te[ty + 8 * r][tx] = e; tv[ty + 8 * r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty + 8 * r, o = o0 + tx;
        if (i < I && o < ld) {                                   // zero for o >= O: keeps the operand tail zero-filled
            store_operand(e_t, split, I, ld, i, o, te[tx][ty + 8 * r]);
            if (v_t) store_operand(v_t, split, I, ld, i, o, tv[tx][ty + 8 * r]);
        }
    }
}

// generic (R,C) -> operand [C][ld] transpose, optional square (same tiling as K7)
__global__ __launch_bounds__(256) void transpose_operand_kernel(const float* __restrict__ src, int R, int C, int lds_src,
                                                                void* dst, int ld, int square, int split) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        float v = (r < R && c < C) ? src[(size_t)r * lds_src + c] : 0.f;
        tile[ty + 8 * k][tx] = square ? v * v : v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, r = r0 + tx;
        if (c < C && r < ld) store_operand(dst, split, C, ld, c, r, tile[tx][ty + 8 * k]);
    }
}

}  // namespace

// (R,C) -> operand [R][ld] without a transpose: row r of dst = row r of src (squared if asked), zero tail, fp32 or split.
// The input-gradient operands of a variational-dropout layer: theta (n,m) IS W^T for dX = G . theta^T.
__global__ __launch_bounds__(256) void format_operand_kernel(const float* __restrict__ src, int R, int C, int lds_src,
                                                             void* dst, int ld, int square, int split) {
    const int r = blockIdx.y;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < ld; c += gridDim.x * 256) {
        float v = c < C ? src[(size_t)r * lds_src + c] : 0.f;
        if (square) v *= v;
        store_operand(dst, split, R, ld, r, c, v);
    }
}

extern "C" int lbbnn_format_operand(const float* src, int R, int C, int lds_src, void* dst, int ld, int square, int flags,
                                    void* stream) {
    if (!src || !dst) return LBBNN_E_NULL;
    if (R <= 0 || C <= 0 || lds_src < C) return LBBNN_E_SHAPE;
    if (ld < C || (ld & 31)) return LBBNN_E_ALIGN;
    if (flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
    hipLaunchKernelGGL(format_operand_kernel, dim3((ld + 1023) / 1024, R), dim3(256), 0, static_cast<hipStream_t>(stream), src, R,
                       C, lds_src, dst, ld, square ? 1 : 0, (flags & LBBNN_F_SPLIT16) ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_transpose_operand(const float* src, int R, int C, int lds_src, void* dst, int ld,
                                       int square, int flags, void* stream) {
    if (!src || !dst) return LBBNN_E_NULL;
    if (R <= 0 || C <= 0 || lds_src < C) return LBBNN_E_SHAPE;
    if (ld < R || (ld & 31)) return LBBNN_E_ALIGN;
    if (flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
    hipLaunchKernelGGL(transpose_operand_kernel, dim3((ld + 31) / 32, (C + 31) / 32), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, R, C, lds_src, dst, ld, square ? 1 : 0,
                       (flags & LBBNN_F_SPLIT16) ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_weight_operands_t(const float* mu, const float* rho, const float* lambdal, const float* z,
                                       void* e_t, void* v_t, int ld, int O, int I, int flags, void* stream) {
    if (!mu || !lambdal || !e_t || (v_t && !rho)) return LBBNN_E_NULL;
    if (O <= 0 || I <= 0) return LBBNN_E_SHAPE;
    if (ld < O || (ld & 31)) return LBBNN_E_ALIGN;
    if (flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
    hipLaunchKernelGGL(weight_operands_t_kernel, dim3((ld + 31) / 32, (I + 31) / 32), dim3(256), 0,
                       static_cast<hipStream_t>(stream), mu, rho, lambdal, z, e_t, v_t, ld, O, I, (flags & LBBNN_F_SPLIT16) ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_gate_sample(const lbbnn_gate_args_t* p, const uint64_t* rng, void* stream) {
    if (!p) return LBBNN_E_NULL;
    const lbbnn_gate_args_t& a = *p;
    if (!a.mu || !a.bias_mu || !a.bias_out) return LBBNN_E_NULL;
    if (a.O <= 0 || a.I <= 0) return LBBNN_E_SHAPE;
    if (a.mode < 0 || a.mode > 2) return LBBNN_E_FLAGS;
    if (a.flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
    if (a.w_out && (a.ld < a.I || (a.ld & 31))) return LBBNN_E_ALIGN;
    if (a.mode == LBBNN_MODE_SAMPLE && (!a.rho || !a.bias_rho)) return LBBNN_E_NULL;
    if (a.mode != LBBNN_MODE_MEAN && !a.cgamma) return LBBNN_E_NULL;
    if (a.mode == LBBNN_MODE_MEAN && !a.alpha_attr) return LBBNN_E_NULL;
    if (a.mode == LBBNN_MODE_SAMPLE && (!a.eps_w || !a.eps_b) && !rng) return LBBNN_E_NOISE;
    if (a.want_lp && (!a.rho || !a.bias_rho || !a.cgamma || !a.gamma_alpha || !a.weight_a || !a.weight_b || !a.tau_w ||
                      !a.pa || !a.pb || !a.bias_a || !a.bias_b || !a.tau_b || !a.rows || !a.log_prior || !a.log_q))
        return LBBNN_E_NULL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    lbbnn_gate_draw_args_t d{};
    d.g = a;
    hipLaunchKernelGGL(gate_sample_kernel<false>, dim3(a.O), dim3(256), 0, s, d, rng);
    hipLaunchKernelGGL(gate_finalize_kernel<false>, dim3(1), dim3(256), 0, s, d, rng);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_gate_sample_draw(const lbbnn_gate_draw_args_t* p, const uint64_t* rng, void* stream) {
    if (!p) return LBBNN_E_NULL;
    const lbbnn_gate_draw_args_t& d = *p;
    const lbbnn_gate_args_t& a = d.g;
    if (!a.mu || !a.rho || !a.bias_mu || !a.bias_rho || !a.bias_out || !d.lambdal || !d.gammas || !d.tau_w || !d.tau_b)
        return LBBNN_E_NULL;
    if (!a.weight_a || !a.weight_b || !a.pa || !a.pb || !a.bias_a || !a.bias_b || !a.rows || !a.log_prior || !a.log_q)
        return LBBNN_E_NULL;
    if (a.O <= 0 || a.I <= 0) return LBBNN_E_SHAPE;
    if (a.mode != LBBNN_MODE_SAMPLE || !a.want_lp) return LBBNN_E_FLAGS;
    if (a.flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
    if (!(d.temperature > 0.f)) return LBBNN_E_FLAGS;
    if (a.w_out && (a.ld < a.I || (a.ld & 31))) return LBBNN_E_ALIGN;
    if (!rng) return LBBNN_E_NOISE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gate_sample_kernel<true>, dim3(a.O), dim3(256), 0, s, d, rng);
    hipLaunchKernelGGL(gate_finalize_kernel<true>, dim3(1), dim3(256), 0, s, d, rng);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_gate_backward(const lbbnn_gate_bwd_args_t* p, const uint64_t* rng, void* stream) {
    if (!p) return LBBNN_E_NULL;
    const lbbnn_gate_bwd_args_t& a = *p;
    if (!a.mu || !a.rho || !a.gamma_alpha || !a.cgamma || !a.bias_mu || !a.bias_rho || !a.bias_a || !a.bias_b || !a.tau_b ||
        !a.weight_a || !a.weight_b || !a.tau_w || !a.pa || !a.pb) return LBBNN_E_NULL;
    if (!a.d_mu || !a.d_rho || !a.d_cgamma || !a.d_alpha || !a.d_bias_mu || !a.d_bias_rho || !a.d_bias_a || !a.d_bias_b ||
        !a.d_tau_b || !a.d_scalars || !a.rows) return LBBNN_E_NULL;
    if ((!a.eps_w || !a.eps_b) && !rng) return LBBNN_E_NOISE;
    if (a.O <= 0 || a.I <= 0) return LBBNN_E_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    lbbnn_gate_bwd_draw_args_t d{};
    d.g = a;
    hipLaunchKernelGGL(gate_backward_kernel<false>, dim3(a.O), dim3(256), 0, s, d, rng);
    hipLaunchKernelGGL(gate_backward_tail_kernel<false>, dim3(1), dim3(256), 0, s, d, rng);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_gate_backward_draw(const lbbnn_gate_bwd_draw_args_t* p, const uint64_t* rng, void* stream) {
    if (!p) return LBBNN_E_NULL;
    const lbbnn_gate_bwd_draw_args_t& d = *p;
    const lbbnn_gate_bwd_args_t& a = d.g;
    if (!a.mu || !a.rho || !d.lambdal || !a.bias_mu || !a.bias_rho || !a.bias_a || !a.bias_b || !a.tau_b ||
        !a.weight_a || !a.weight_b || !a.tau_w || !a.pa || !a.pb) return LBBNN_E_NULL;
    if (!a.d_mu || !a.d_rho || !d.d_lambdal || !a.d_bias_mu || !a.d_bias_rho || !a.d_bias_a || !a.d_bias_b ||
        !a.d_scalars || !a.rows) return LBBNN_E_NULL;
    if (!rng) return LBBNN_E_NOISE;
    if (a.O <= 0 || a.I <= 0) return LBBNN_E_SHAPE;
    if (!(d.temperature > 0.f)) return LBBNN_E_FLAGS;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gate_backward_kernel<true>, dim3(a.O), dim3(256), 0, s, d, rng);
    hipLaunchKernelGGL(gate_backward_tail_kernel<true>, dim3(1), dim3(256), 0, s, d, rng);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_gate_members(const lbbnn_gate_member_desc_t* layers, int n, int members, int gates, float temperature,
                                  const uint64_t* rng, uint64_t member_advance, void* stream) {
    if (!layers) return LBBNN_E_NULL;
    if (n < 1 || n > LBBNN_MAX_LAYERS || members < 1 || members > 65535) return LBBNN_E_SHAPE;
    if (gates != LBBNN_GATES_SAMPLE && gates != LBBNN_GATES_MPM) return LBBNN_E_FLAGS;
    if (gates == LBBNN_GATES_SAMPLE && !(temperature > 0.f)) return LBBNN_E_FLAGS;
    GateMembersLaunch ga{};
    long long rows = 0;
    int max_ld = 0;
    for (int l = 0; l < LBBNN_MAX_LAYERS; ++l) { ga.row0[l] = INT_MAX; ga.row_end[l] = INT_MAX; }
    for (int l = 0; l < n; ++l) {
        const lbbnn_gate_member_desc_t& d = layers[l];
        if (!d.mu || !d.rho || !d.lambdal || !d.bias_mu || !d.bias_rho || !d.w_out || !d.bias_out) return LBBNN_E_NULL;
        if (d.O <= 0 || d.I <= 0 || d.ld > kGmMaxLd) return LBBNN_E_SHAPE;
        if (d.ld < d.I || (d.ld & 31) || (reinterpret_cast<uintptr_t>(d.w_out) & 15u)) return LBBNN_E_ALIGN;
        if (d.flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
        ga.l[l] = d;
        max_ld = d.ld > max_ld ? d.ld : max_ld;
        ga.vec[l] = (d.I % 4) == 0 &&
                    ((reinterpret_cast<uintptr_t>(d.mu) | reinterpret_cast<uintptr_t>(d.rho) | reinterpret_cast<uintptr_t>(d.lambdal)) & 15u) == 0;
        ga.row0[l] = (int)rows;
        rows += d.O;
        if (rows > INT_MAX) return LBBNN_E_SHAPE;
        ga.row_end[l] = (int)rows;
    }
    if (!rng) return LBBNN_E_NOISE;
    ga.members = members; ga.gates = gates; ga.temperature = temperature; ga.member_advance = member_advance;
    const dim3 grid((unsigned)rows), block(kGmThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (max_ld <= kGmThreads * 8) hipLaunchKernelGGL(gate_members_kernel<1>, grid, block, 0, s, ga, rng);
    else if (max_ld <= kGmThreads * 16) hipLaunchKernelGGL(gate_members_kernel<2>, grid, block, 0, s, ga, rng);
    else hipLaunchKernelGGL(gate_members_kernel<4>, grid, block, 0, s, ga, rng);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ test entry points
__global__ __launch_bounds__(256) void philox_uniform_kernel(const uint64_t* rng, uint32_t stream, long long row_base,
                                                             long long rows, long long cols, float* out) {
    const long long gpr = (cols + 3) / 4;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= gpr * rows) return;
    const long long r = g / gpr, cg = g % gpr;
    const Philox4 b = philox_bits4(rng[0], rng[1], stream, (uint64_t)(row_base + r), (uint32_t)cg);
    const uint32_t w[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) if (cg * 4 + k < cols) out[r * cols + cg * 4 + k] = uniform24(w[k]);
}

__global__ __launch_bounds__(256) void philox_std_gamma_kernel(const uint64_t* rng, uint32_t stream, const float* a,
                                                               const float* rate, long long n, float* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = rate ? gamma_rate_draw(a[i], rate[i], rng[0], rng[1], stream, (uint64_t)i)
                  : gamma_rate_draw(a[i], 1.f, rng[0], rng[1], stream, (uint64_t)i);
}

__global__ __launch_bounds__(256) void gamma_grad_kernel(const float* x, const float* a, long long n, float* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = gamma_grad_one(x[i], a[i]);
}

extern "C" int lbbnn_philox_uniform(const uint64_t* rng, uint32_t rng_stream, int64_t row_base, int64_t rows, int64_t cols,
                                    float* out, void* stream) {
    if (!rng || !out) return LBBNN_E_NULL;
    if (rows <= 0 || cols <= 0) return LBBNN_E_SHAPE;
    const long long groups = ((cols + 3) / 4) * rows;
    hipLaunchKernelGGL(philox_uniform_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), rng, rng_stream, (long long)row_base, (long long)rows, (long long)cols, out);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_philox_std_gamma(const uint64_t* rng, uint32_t rng_stream, const float* a, const float* rate, int64_t n,
                                      float* out, void* stream) {
    if (!rng || !a || !out) return LBBNN_E_NULL;
    if (n <= 0) return LBBNN_E_SHAPE;
    hipLaunchKernelGGL(philox_std_gamma_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), rng, rng_stream, a, rate, (long long)n, out);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_gamma_grad(const float* x, const float* a, int64_t n, float* out, void* stream) {
    if (!x || !a || !out) return LBBNN_E_NULL;
    if (n <= 0) return LBBNN_E_SHAPE;
    hipLaunchKernelGGL(gamma_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, a, (long long)n, out);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_vd_operands(const float* theta, void* e_w, void* var_w, int ld, int I, int O, int flags, void* stream) {
    if (!theta || !e_w || !var_w) return LBBNN_E_NULL;
    if (I <= 0 || O <= 0) return LBBNN_E_SHAPE;
    if (ld < I || (ld & 31)) return LBBNN_E_ALIGN;
    if (flags & ~(LBBNN_F_SPLIT16 | LBBNN_F_HALF16)) return LBBNN_E_FLAGS;
    if ((flags & LBBNN_F_HALF16) && !(flags & LBBNN_F_SPLIT16)) return LBBNN_E_FLAGS;
    hipLaunchKernelGGL(vd_operands_kernel, dim3((ld + 31) / 32, (O + 31) / 32), dim3(256), 0,
                       static_cast<hipStream_t>(stream), theta, e_w, var_w, ld, I, O,
                       (flags & LBBNN_F_HALF16) ? 2 : ((flags & LBBNN_F_SPLIT16) ? 1 : 0));
    return (int)hipGetLastError();
}
