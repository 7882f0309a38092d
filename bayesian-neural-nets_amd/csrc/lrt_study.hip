// lbbnn_lrt_study_fit: R independent one-layer LRT networks with a sigmoid head, trained in ONE launch (include/lbbnn.h;
// DESIGN.md 9.5).  The simulation study is many small fits: a 20 -> 1 layer is a few hundred floats of state, so a replicate is
// ONE workgroup of 256 threads that loads its parameters, Adam moments, step counter and Philox state once, loops over the
// epochs and batches itself, and stores them once.  Grid = R workgroups.  A workgroup reads and writes its own replicate's
// slices only; there is no communication between workgroups -- no atomics, no flags, no spinning -- and every loop bound is a
// host-passed count, so a workgroup waits on nothing but its own loads and the barriers of its own 256 threads.
//
// Elements.  The layer is laid out as O rows of I + 1 entries: entry (o, i < I) is weight (o, i), entry (o, I) is the bias of
// unit o, whose "input" is 1.  Element e = o (I + 1) + i belongs to thread e % 256, slot e / 256 (at most 5 slots: O I <= 1024,
// O <= 16).  The owner keeps the element's parameters (mu, rho, lambda | bias_mu, bias_rho) and their moments in registers for
// the whole launch.
//
// One step:
//   prepare   owners: alpha, sigma -> e_w, var_w (bias: bias_mu, sigma_b^2) into LDS; the element's KL term
//   forward   item (b, o) of a tile of rows: mean / variance products over x and x^2, eps_out from Philox, the logit, the
//             probability, the BCE term and counts (binary_head.hip's formulas), g = d loss / d logit and g_v = g eps / (2 std)
//             into LDS
//   backward  element (o, i): Sum_b g x and Sum_b g_v x^2 over the tile's rows (the bias entries: Sum_b g, Sum_b g_v)
//   reduce    nll, counts and KL by block_sum (wave sums, then the four waves in index order)
//   update    owners: the chain through alpha, sigma and the KL (weight_pass_bwd.hip's elem_bwd with z = 1, the bias terms of
//             vector_bwd.hip's bias_backward_kernel), then Adam (adam.hip's update, expression for expression)
// Fixed orders: with fewer than 256 elements the threads form G = 256 / elements row groups; group g adds rows g, g + G, ...
// of every tile in rising order and the owner adds the G partials in index order.  With 256 elements or more one thread adds
// all rows of its element in rising order.  Nothing depends on scheduling or on another replicate: a replicate's bits are a
// function of its own inputs.
//
// Guard.  A step is skipped -- no parameter, moment or step counter changes; it is counted -- when its fp32 loss is not finite
// OR a probability of the batch is not finite.  The second condition is this kernel's own: the BCE term of binary_head.hip costs
// a NaN probability a finite 100 (fmax returns its number), while the gradient of that element is NaN.
#include <cmath>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"

namespace {

using namespace lbbnn;
constexpr int NT = 256;                 // threads per replicate
constexpr int NS = 5;                   // element slots per thread: 16 * 65 = 1040 <= 5 * 256
constexpr int MAXE = 1040;              // O (I + 1) at the limits
constexpr int GT = 4096;                // (row, unit) items per tile: rows per tile = GT / O >= 256

__device__ __forceinline__ bool target_ok(float y) { return y >= 0.f && y <= 1.f; }      // false for NaN

struct PriorConsts { float mp, inv_sp2, log_sp, log_ap, log_1map, bmp, bsp, binv; };

__global__ __launch_bounds__(NT) void lrt_study_kernel(const lbbnn_study_args_t a) {
    __shared__ float ew[MAXE], vw[MAXE];                // operands of the step, rows of I + 1
    __shared__ float gl[GT], gvl[GT];                   // g, g_v of the tile's items
    __shared__ float redm[NT], redv[NT];                // row-group partials (G * elements <= 256)
    __shared__ double scratch[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int I = a.I, O = a.O, I1 = I + 1, OI = O * I, ET = O * I1, P = 3 * OI + 2 * O;
    const int G = ET < NT ? NT / ET : 1;                // row groups
    const int rg = ET < NT ? tid / ET : 0;
    float* const pr = a.params + (size_t)r * P;
    float* const mr = a.exp_avg + (size_t)r * P;
    float* const vr = a.exp_avg_sq + (size_t)r * P;
    const float* const xg = a.x + (size_t)r * a.x_rstride;
    const float* const yg = a.y + (size_t)r * a.y_rstride;

    // ---- elements of this thread: own[j] (state, update) and acc[j] (the backward sums; = own[j] unless row groups are on)
    int own[NS], acc[NS], eo[NS], ei[NS];
    float Pp[NS][3], Mm[NS][3], Vv[NS][3];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + NT * j;
        own[j] = e < ET ? e : -1;
        acc[j] = ET < NT ? ((j == 0 && rg < G) ? tid - rg * ET : -1) : own[j];
        const int ae = acc[j] >= 0 ? acc[j] : 0;
        eo[j] = ae / I1;
        ei[j] = ae - eo[j] * I1;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            Pp[j][q] = 0.f; Mm[j][q] = 0.f; Vv[j][q] = 0.f;
            if (own[j] >= 0) {
                const int idx = ei[j] < I ? q * OI + eo[j] * I + ei[j] : (q < 2 ? 3 * OI + q * O + eo[j] : -1);
                if (idx >= 0) { Pp[j][q] = pr[idx]; Mm[j][q] = mr[idx]; Vv[j][q] = vr[idx]; }
            }
        }
    }
    const lbbnn_priors_t pri = a.priors[(size_t)r * a.priors_rstride];
    PriorConsts c;
    c.mp = pri.mu_prior; c.inv_sp2 = 1.f / (pri.sigma_prior * pri.sigma_prior);
    c.log_sp = logf(pri.sigma_prior); c.log_ap = logf(pri.alpha_prior); c.log_1map = logf(1.f - pri.alpha_prior);
    c.bmp = pri.bias_mu_prior; c.bsp = pri.bias_sigma_prior; c.binv = 1.f / (pri.bias_sigma_prior * pri.bias_sigma_prior);
    const lbbnn_adam_hyper_t h = a.hyper[r];
    const float b1 = h.beta1, b2 = h.beta2, eps_adam = h.eps, wd = h.weight_decay;
    float step_f = a.step[r];
    const uint64_t seed = a.rng[2 * (size_t)r];
    uint64_t offs = a.rng[2 * (size_t)r + 1];
    long long skipped = a.skipped[r];
    const int N = a.N, batch = a.batch;
    const int nb = (int)(((long long)N + batch - 1) / batch);
    const float kl_scale = (float)((double)batch / (double)N);          // 1 / NUM_BATCHES with the script's float NUM_BATCHES
    const int TB = GT / O;

    for (int ep = a.first_epoch; ep < a.first_epoch + a.n_epochs; ++ep) {
        bool restart = false;
        for (int k = 0; k < a.n_restarts; ++k) restart |= a.restarts[k] == ep;
        if (restart) {                                                  // a fresh optim.Adam: moments and step counter
            step_f = 0.f;
#pragma unroll
            for (int j = 0; j < NS; ++j)
#pragma unroll
                for (int q = 0; q < 3; ++q) { Mm[j][q] = 0.f; Vv[j][q] = 0.f; }
        }
        const float lr = a.lr[(size_t)r * a.lr_rstride + ep];
        double h_loss = 0.0, h_nll = 0.0, h_ok = 0.0, h_n = 0.0, last_loss = 0.0, last_nll = 0.0;
        long long h_fin = 0, h_skip = 0;

        for (int k = 0; k < nb; ++k) {
            const long long row0 = (long long)k * batch;
            const int Bt = (int)((long long)N - row0 < batch ? (long long)N - row0 : batch);
            // ---- prepare: the step's operands and the KL
            float klt = 0.f;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (own[j] < 0) continue;
                if (ei[j] < I) {
                    const float mu = Pp[j][0], rho = Pp[j][1], lam = Pp[j][2];
                    const float alpha = k1_alpha(lam), sigma = k1_sigma(rho);
                    const float ope = 1.f + k1_exp_raw(-lam), er = k1_exp_acc(rho);          // their inner values, for the KL
                    const float s2 = sigma * sigma;
                    ew[own[j]] = mu * alpha;
                    vw[own[j]] = s2 * (alpha * alpha);
                    const float d = mu - c.mp;
                    const float la = -0.6931471805599453f * __builtin_amdgcn_logf(ope);       // log(alpha)
                    const float T = (c.log_sp - k1_log_sigma_of(rho, er, sigma)) - 0.5f + (la - c.log_ap) + (s2 + d * d) * 0.5f * c.inv_sp2;
                    klt += alpha * T + (1.f - alpha) * ((la - lam) - c.log_1map);             // LBBNN-GP-MF-LRT.py:189-192
                } else {
                    const float sb = softplus_ref(Pp[j][1]);
                    const float d = Pp[j][0] - c.bmp;
                    ew[own[j]] = Pp[j][0];
                    vw[own[j]] = sb * sb;
                    klt += logf(c.bsp / sb) - 0.5f + (sb * sb + d * d) / (2.f * c.bsp * c.bsp);   // :185-186
                }
            }
            const float kl = (float)block_sum<double, 4>((double)klt, scratch);              // (its barriers publish ew / vw)

            // ---- forward and the row sums of the backward, tile by tile
            double s_nll = 0.0;
            int c_ok = 0, c_bad = 0, c_nf = 0;
            float am[NS], av[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) { am[j] = 0.f; av[j] = 0.f; }
            for (int t0 = 0; t0 < Bt; t0 += TB) {
                const int nr = Bt - t0 < TB ? Bt - t0 : TB;
                for (int idx = tid; idx < nr * O; idx += NT) {
                    const int bl = idx / O, o = idx - bl * O, b = t0 + bl;
                    const float* __restrict__ xr = xg + (size_t)(row0 + b) * I;
                    const float* we = ew + o * I1;
                    const float* wv = vw + o * I1;
                    float sm = 0.f, sv = 0.f;
                    for (int i = 0; i < I; ++i) {
                        const float xv = xr[i];
                        sm = __builtin_fmaf(xv, we[i], sm);
                        sv = __builtin_fmaf(xv * xv, wv[i], sv);
                    }
                    const float sd = sqrt_hw(sv + wv[I]);
                    float e4[4];
                    philox_normal4(seed, offs, LBBNN_STREAM_EPS_OUT * 64u, (uint64_t)b, (uint32_t)(o >> 2), e4);
                    const int oq = o & 3;
                    const float e = oq == 0 ? e4[0] : oq == 1 ? e4[1] : oq == 2 ? e4[2] : e4[3];
                    const float logit = (sm + we[I]) + sd * e;
                    const float p = sigmoid_ref(logit);
                    const float yv = yg[(size_t)(row0 + b) * O + o];
                    if (!isfinite(p)) ++c_nf;
                    float gm = 0.f, gv = 0.f;
                    if (!target_ok(yv)) {
                        ++c_bad;
                    } else {
                        const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
                        s_nll += (double)((yv - 1.f) * lq - yv * lp);
                        if ((p > 0.5f) == (yv > 0.5f)) ++c_ok;
                        const float d = (1.f - p) * p;
                        gm = ((p - yv) / fmaxf(d, 1e-12f)) * d;
                        gv = gm * e / (2.f * sd);
                    }
                    gl[idx] = gm; gvl[idx] = gv;
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    if (acc[j] < 0) continue;
                    const int o = eo[j], i = ei[j];
                    const float* __restrict__ xc = xg + (size_t)(row0 + t0) * I + (i < I ? i : 0);
                    float sm = am[j], sv = av[j];
                    for (int bl = rg; bl < nr; bl += G) {
                        const float xv = i < I ? xc[(size_t)bl * I] : 1.f;
                        sm = __builtin_fmaf(gl[bl * O + o], xv, sm);
                        sv = __builtin_fmaf(gvl[bl * O + o], xv * xv, sv);
                    }
                    am[j] = sm; av[j] = sv;
                }
                __syncthreads();
            }
            const double nll = block_sum<double, 4>(s_nll, scratch);
            const double n_ok = block_sum<double, 4>((double)c_ok, scratch);
            const double n_nf = block_sum<double, 4>((double)c_nf, scratch);
            (void)c_bad;
            if (G > 1) {                                                 // the row groups' partials, in index order
                if (acc[0] >= 0) { redm[rg * ET + acc[0]] = am[0]; redv[rg * ET + acc[0]] = av[0]; }
                __syncthreads();
                if (own[0] >= 0) {
                    float sm = redm[own[0]], sv = redv[own[0]];
                    for (int g = 1; g < G; ++g) { sm += redm[g * ET + own[0]]; sv += redv[g * ET + own[0]]; }
                    am[0] = sm; av[0] = sv;
                }
            }
            // ---- the step's loss and its guard (the same values in every thread)
            const double kl_term = (double)kl * (double)kl_scale;
            const float lf = (float)(nll + kl_term);
            const bool finite = isfinite(lf) && n_nf == 0.0;
            if (finite) {
                const float t = step_f + 1.f;
                const float bc1 = 1.f - powf(b1, t), bc2s = sqrtf(1.f - powf(b2, t));
                const float step_size = lr / bc1;
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    if (own[j] < 0) continue;
                    float g3[3] = {0.f, 0.f, 0.f};
                    int nq = 3;
                    if (ei[j] < I) {                                    // weight_pass_bwd.hip elem_bwd with z = 1, g_kl = kl_scale
                        const float mu = Pp[j][0], rho = Pp[j][1], lam = Pp[j][2], gWm = am[j], gWv = av[j];
                        const float ope = 1.f + k1_exp_raw(-lam);
                        const float alpha = __builtin_amdgcn_rcpf(ope);
                        const float er = k1_exp_acc(rho);
                        const float sigma = k1_sigma_of(er);
                        const float dsig = er * __builtin_amdgcn_rcpf(1.f + er);
                        const float a2 = alpha * alpha, s2 = sigma * sigma;
                        const float d = mu - c.mp;
                        const float la = -0.6931471805599453f * __builtin_amdgcn_logf(ope);
                        const float T = (c.log_sp - k1_log_sigma_of(rho, er, sigma)) - 0.5f + (la - c.log_ap) + (s2 + d * d) * 0.5f * c.inv_sp2;
                        const float Gmu = gWm * alpha + kl_scale * alpha * d * c.inv_sp2;
                        const float Gsig = gWv * 2.f * sigma * a2 + kl_scale * alpha * (sigma * c.inv_sp2 - __builtin_amdgcn_rcpf(sigma));
                        const float Gal = gWm * mu + gWv * 2.f * s2 * alpha + kl_scale * (T - ((la - lam) - c.log_1map));
                        g3[0] = Gmu; g3[1] = Gsig * dsig; g3[2] = Gal * alpha * (1.f - alpha);
                    } else {                                            // vector_bwd.hip bias_backward_kernel
                        const float er = expf(Pp[j][1]);
                        const float sb = log1pf(er), dsig = er / (1.f + er);
                        g3[0] = am[j] + kl_scale * (Pp[j][0] - c.bmp) * c.binv;
                        g3[1] = (av[j] * 2.f * sb + kl_scale * (sb * c.binv - 1.f / sb)) * dsig;
                        nq = 2;
                    }
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        if (q >= nq) continue;
                        const float gq = g3[q] + wd * Pp[j][q];         // adam.hip's update
                        Mm[j][q] = b1 * Mm[j][q] + (1.f - b1) * gq;
                        Vv[j][q] = b2 * Vv[j][q] + (1.f - b2) * gq * gq;
                        const float denom = sqrtf(Vv[j][q]) / bc2s + eps_adam;
                        Pp[j][q] = Pp[j][q] - step_size * (Mm[j][q] / denom);
                    }
                }
                step_f += 1.f;
                h_loss += nll + kl_term; h_nll += nll; ++h_fin;
            } else {
                ++skipped; ++h_skip;
            }
            offs += 1;                                                  // the forward drew: skipped steps advance too
            h_ok += n_ok; h_n += (double)Bt * O;
            last_loss = (double)lf; last_nll = nll;
        }
        if (tid == 0) {
            double* hr = a.history + ((size_t)r * a.epochs + ep) * 6;
            hr[0] = h_loss / (double)h_fin; hr[1] = h_nll / (double)h_fin; hr[2] = h_ok / h_n;
            hr[3] = last_loss; hr[4] = last_nll; hr[5] = (double)h_skip;
        }
    }

    // ---- the state goes back once
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        if (own[j] < 0) continue;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int idx = ei[j] < I ? q * OI + eo[j] * I + ei[j] : (q < 2 ? 3 * OI + q * O + eo[j] : -1);
            if (idx >= 0) { pr[idx] = Pp[j][q]; mr[idx] = Mm[j][q]; vr[idx] = Vv[j][q]; }
        }
    }
    if (tid == 0) { a.step[r] = step_f; a.rng[2 * (size_t)r + 1] = offs; a.skipped[r] = skipped; }
}

inline bool off4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }
inline bool off8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

}  // namespace

extern "C" int lbbnn_lrt_study_fit(const lbbnn_study_args_t* p, void* stream) {
    if (!p) return LBBNN_E_NULL;
    const lbbnn_study_args_t& a = *p;
    if (!a.params || !a.exp_avg || !a.exp_avg_sq || !a.step || !a.rng || !a.skipped || !a.x || !a.y || !a.priors || !a.hyper ||
        !a.lr || !a.history || (a.n_restarts > 0 && !a.restarts))
        return LBBNN_E_NULL;
    if (a.I < 1 || a.I > LBBNN_STUDY_MAX_I || a.O < 1 || a.O > LBBNN_STUDY_MAX_O || a.O * a.I > LBBNN_STUDY_MAX_WEIGHTS)
        return LBBNN_E_SHAPE;
    if (a.batch < 1 || a.batch > LBBNN_STUDY_MAX_BATCH || a.N < 1 || a.R < 1 || a.R > 65535) return LBBNN_E_SHAPE;
    if (a.n_epochs < 0 || a.first_epoch < 0 || a.epochs < 1 || (long long)a.first_epoch + a.n_epochs > a.epochs || a.n_restarts < 0)
        return LBBNN_E_SHAPE;
    if ((a.x_rstride != 0 && a.x_rstride < (int64_t)a.N * a.I) || (a.y_rstride != 0 && a.y_rstride < (int64_t)a.N * a.O) ||
        (a.priors_rstride != 0 && a.priors_rstride != 1) || (a.lr_rstride != 0 && a.lr_rstride < a.epochs))
        return LBBNN_E_SHAPE;
    if (off4(a.params) || off4(a.exp_avg) || off4(a.exp_avg_sq) || off4(a.step) || off8(a.rng) || off8(a.skipped) || off4(a.x) ||
        off4(a.y) || off4(a.priors) || off4(a.hyper) || off4(a.lr) || off4(a.restarts) || off8(a.history))
        return LBBNN_E_ALIGN;
    if (a.n_epochs == 0) return 0;
    hipLaunchKernelGGL(lrt_study_kernel, dim3((unsigned)a.R), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
