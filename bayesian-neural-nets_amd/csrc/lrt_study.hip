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
//
// lbbnn_mnf_study_fit: the same kernel, instantiated for one-layer planar-MNF networks.  An LRT replicate is an
// MNF replicate with z == 1 and without the flow terms of the KL, so the prepare step, the tiled forward, the head, the row
// sums, the guard, Adam and the history below exist once; `if constexpr (MNF)` adds
//   vectors   thread i < I owns element i of q0_mean, q0_log_var, r0_c, r0_b1, r0_b2 and of every transform's u and w, with
//             their moments, in registers; the transforms' biases are held (and updated identically) by every thread
//   flows     z_fwd, z_kl (+ log-dets, log_q0) and the r flow transform by transform (mnf_flow.hip's planar_apply on both
//             draws): one fixed-order block sum of three values per transform; z_fwd, z_kl, r0_c go to LDS for the elements
//   KL tail   act_mu / act_var: the owners' terms through LDS, unit o adds its row in index order; m, log_rb (mnf_flow.hip K5)
//   backward  vector_bwd.hip V1 (da_mu, da_var), elem_bwd.h with the real z_fwd / z_kl / r0_c, the three column sums in unit
//             order through LDS, vector_bwd.hip V2 (flow_planar_backward_body) with the work vectors in registers
//   update    Adam with the rate of the tensor's group: 0 the ten named tensors, 1 z_flow, 2 r_flow
// As V1 of the ordinary step, da_var divides by sqrt(act_var): a unit whose act_var is exactly 0 (r0_c all zero -- not reachable
// from the seeded initialisation) gives a NaN gradient that the guard on the loss does not see.
// The LRT instantiation compiles the expressions it had before the template.
#include <cmath>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "elem_bwd.h"

namespace {

using namespace lbbnn;
constexpr int NT = 256;                 // threads per replicate
constexpr int NS = 5;                   // element slots per thread: 16 * 65 = 1040 <= 5 * 256
constexpr int MAXE = 1040;              // O (I + 1) at the limits
constexpr int GT = 4096;                // (row, unit) items per tile: rows per tile = GT / O >= 256
static_assert(GT >= 3 * MAXE, "the MNF step parks its three column terms of MAXE floats each in the tile buffer gl");

__device__ __forceinline__ bool target_ok(float y) { return y >= 0.f && y <= 1.f; }      // false for NaN

struct PriorConsts { float mp, inv_sp2, log_sp, log_ap, log_1map, bmp, bsp, binv; };

constexpr int MT = LBBNN_STUDY_MAX_TRANSFORMS;
struct PMV { float p, m, v; };           // a vector element (or a transform's bias) with its Adam moments
__device__ __forceinline__ int flow_T(const lbbnn_study_args_t&, int) { return 0; }
__device__ __forceinline__ int flow_T(const lbbnn_mnf_study_args_t& a, int r_flow) { return r_flow ? a.Tr : a.Tz; }

// three block sums behind one pair of barriers: wave sums, then the four waves in index order (block_sum's order)
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double* scr) {
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { scr[w] = a; scr[4 + w] = b; scr[8 + w] = c; }
    __syncthreads();
    a = ((scr[0] + scr[1]) + scr[2]) + scr[3];
    b = ((scr[4] + scr[5]) + scr[6]) + scr[7];
    c = ((scr[8] + scr[9]) + scr[10]) + scr[11];
}

template <bool MNF, typename Args>
__global__ __launch_bounds__(NT) void study_kernel(const Args a) {
    __shared__ float ew[MAXE], vw[MAXE];                // operands of the step, rows of I + 1
    __shared__ float gl[GT], gvl[GT];                   // g, g_v of the tile's items
    __shared__ float redm[NT], redv[NT];                // row-group partials (G * elements <= 256)
    __shared__ double scratch[4];
    __shared__ double scr3[MNF ? 12 : 1];
    __shared__ float zfs[MNF ? NT : 1], zks[MNF ? NT : 1], rcs[MNF ? NT : 1];       // z_fwd, z_kl, r0_c of the step
    __shared__ float dams[MNF ? LBBNN_STUDY_MAX_O : 1], davs[MNF ? LBBNN_STUDY_MAX_O : 1], s_zb[1];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int Tz = flow_T(a, 0), Tr = flow_T(a, 1);
    const int I = a.I, O = a.O, I1 = I + 1, OI = O * I, ET = O * I1, P0 = 3 * OI + 2 * O;
    const int P = MNF ? P0 + 5 * I + (Tz + Tr) * (2 * I + 1) : P0;
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
    // ---- MNF: the vectors of thread i = tid < I, the transforms' biases in every thread
    const bool vi = MNF && tid < I;
    PMV Vn[5], Zu[MT], Zw[MT], Zb[MT], Ru[MT], Rw[MT], Rb[MT];
    const auto ld_pmv = [&](PMV& s, int idx, bool on) {
        s.p = 0.f; s.m = 0.f; s.v = 0.f;
        if (on) { s.p = pr[idx]; s.m = mr[idx]; s.v = vr[idx]; }
    };
    const auto st_pmv = [&](const PMV& s, int idx) { pr[idx] = s.p; mr[idx] = s.m; vr[idx] = s.v; };
    if constexpr (MNF) {
#pragma unroll
        for (int q = 0; q < 5; ++q) ld_pmv(Vn[q], P0 + q * I + tid, vi);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int zo = P0 + 5 * I + t * (2 * I + 1), ro = P0 + 5 * I + (Tz + t) * (2 * I + 1);
            ld_pmv(Zu[t], zo + tid, vi && t < Tz); ld_pmv(Zw[t], zo + I + tid, vi && t < Tz); ld_pmv(Zb[t], zo + 2 * I, t < Tz);
            ld_pmv(Ru[t], ro + tid, vi && t < Tr); ld_pmv(Rw[t], ro + I + tid, vi && t < Tr); ld_pmv(Rb[t], ro + 2 * I, t < Tr);
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
    ElemConsts ce;                                                      // elem_bwd.h's view of the priors, g_kl = kl_scale
    ce.mp = c.mp; ce.inv_sp2 = c.inv_sp2; ce.log_sp = c.log_sp; ce.log_ap = c.log_ap; ce.log_1map = c.log_1map; ce.gk = kl_scale;

    for (int ep = a.first_epoch; ep < a.first_epoch + a.n_epochs; ++ep) {
        bool restart = false;
        for (int k = 0; k < a.n_restarts; ++k) restart |= a.restarts[k] == ep;
        if (restart) {                                                  // a fresh optim.Adam: moments and step counter
            step_f = 0.f;
#pragma unroll
            for (int j = 0; j < NS; ++j)
#pragma unroll
                for (int q = 0; q < 3; ++q) { Mm[j][q] = 0.f; Vv[j][q] = 0.f; }
            if constexpr (MNF) {
#pragma unroll
                for (int q = 0; q < 5; ++q) { Vn[q].m = 0.f; Vn[q].v = 0.f; }
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    Zu[t].m = Zu[t].v = Zw[t].m = Zw[t].v = Zb[t].m = Zb[t].v = 0.f;
                    Ru[t].m = Ru[t].v = Rw[t].m = Rw[t].v = Rb[t].m = Rb[t].v = 0.f;
                }
            }
        }
        const size_t lr_at = (size_t)r * a.lr_rstride + ep;
        const float lr = MNF ? a.lr[lr_at * 3] : a.lr[lr_at];
        const float lr_z = MNF ? a.lr[lr_at * 3 + 1] : 0.f, lr_r = MNF ? a.lr[lr_at * 3 + 2] : 0.f;
        double h_loss = 0.0, h_nll = 0.0, h_ok = 0.0, h_n = 0.0, last_loss = 0.0, last_nll = 0.0;
        long long h_fin = 0, h_skip = 0;

        for (int k = 0; k < nb; ++k) {
            const long long row0 = (long long)k * batch;
            const int Bt = (int)((long long)N - row0 < batch ? (long long)N - row0 : batch);
            // ---- MNF: the draws and the flows (mnf_flow.hip planar_apply on both draws; vector_bwd.hip keeps the same values)
            float ef = 0.f, ek = 0.f, sd0 = 0.f, zfc = 0.f, zkc = 0.f, rrc = 0.f, ldq = 0.f, ldr = 0.f;
            float ZF[MT], ZK[MT], RR[MT], thF[MT], thK[MT], uwZ[MT], thR[MT], uwR[MT];   // ZF / ZK / RR[t]: transform t's input
            double lq0 = 0.0;
            if constexpr (MNF) {
                if (vi) {
                    float n4[4];
                    const int w4 = tid & 3;
                    philox_normal4(seed, offs, LBBNN_STREAM_EPS_Z * 64u, (uint64_t)(tid >> 2), 0u, n4);
                    ef = w4 == 0 ? n4[0] : w4 == 1 ? n4[1] : w4 == 2 ? n4[2] : n4[3];
                    philox_normal4(seed, offs, LBBNN_STREAM_EPS_Z2 * 64u, (uint64_t)(tid >> 2), 0u, n4);
                    ek = w4 == 0 ? n4[0] : w4 == 1 ? n4[1] : w4 == 2 ? n4[2] : n4[3];
                    const float qm = Vn[0].p, lv = Vn[1].p;
                    sd0 = expf(0.5f * lv);
                    zfc = qm + sd0 * ef;                                 // LBBNN-GP-MF-MNF.py:183-185
                    zkc = qm + sd0 * ek;
                    const float d = zkc - qm;
                    lq0 = (double)(-0.5f * 1.1447298858494002f - 0.5f * lv - 0.5f * ((d * d) / expf(lv)));   // :213-214
                }
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    ZF[t] = zfc; ZK[t] = zkc; thF[t] = 0.f; thK[t] = 0.f; uwZ[t] = 0.f;
                    if (t < Tz) {                                        // uniform
                        double sf = (double)(Zw[t].p * zfc), sk = (double)(Zw[t].p * zkc), uw = (double)(Zu[t].p * Zw[t].p);
                        block_sum3(sf, sk, uw, scr3);
                        const float tf = tanhf((float)sf + Zb[t].p), tk = tanhf((float)sk + Zb[t].p);   // flows2.py:87
                        thF[t] = tf; thK[t] = tk; uwZ[t] = (float)uw;
                        zfc += Zu[t].p * tf; zkc += Zu[t].p * tk;       // :88
                        ldq += logf(fabsf(1.f + (1.f - tk * tk) * (float)uw));                          // :89, :95
                    }
                }
                rrc = zkc;
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    RR[t] = rrc; thR[t] = 0.f; uwR[t] = 0.f;
                    if (t < Tr) {
                        double sr = (double)(Rw[t].p * rrc), uw = (double)(Ru[t].p * Rw[t].p), z0 = 0.0;
                        block_sum3(sr, uw, z0, scr3);
                        const float th = tanhf((float)sr + Rb[t].p);
                        thR[t] = th; uwR[t] = (float)uw;
                        rrc += Ru[t].p * th;
                        ldr += logf(fabsf(1.f + (1.f - th * th) * (float)uw));
                    }
                }
                if (vi) { zfs[tid] = zfc; zks[tid] = zkc; rcs[tid] = Vn[2].p; }
                if (tid == I - 1) s_zb[0] = rrc;                         // z_b[-1]: the LAST element (:224)
                lq0 = block_sum<double, 4>(lq0, scratch);                // (its barriers publish zfs / zks / rcs / s_zb)
            }
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
                    float d = mu - c.mp;
                    if constexpr (MNF) {                                 // kl_weight(mu z_kl); the terms of act_mu / act_var
                        const float zk = zks[ei[j]], rc = rcs[ei[j]];
                        d = mu * zk - c.mp;
                        gl[own[j]] = rc * zk * (mu * alpha);             // LBBNN-GP-MF-MNF.py:211, :216
                        gvl[own[j]] = (rc * rc) * (s2 * (alpha * alpha));                     // :212, :217
                    }
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
            const double kl_sum = block_sum<double, 4>((double)klt, scratch);                // (its barriers publish ew / vw)
            float kl = (float)kl_sum;
            // ---- MNF: the KL tail (mnf_flow.hip K5) and what vector_bwd.hip's V1 / V2 take from the same sweep
            float act = 0.f, e_act = 0.f, sd_act = 0.f, m_act = 0.f, zb = 0.f, eb = 0.f, dlt = 0.f;
            double S_aux = 0.0, S_zb = 0.0;
            if constexpr (MNF) {
                if (tid < O) {                                           // unit o = tid adds its row's terms in index order
                    float smu = 0.f, svar = 0.f;
                    for (int i = 0; i < I; ++i) { smu += gl[tid * I1 + i]; svar += gvl[tid * I1 + i]; }
                    float n4[4];
                    const int w4 = tid & 3;
                    philox_normal4(seed, offs, LBBNN_STREAM_EPS_ACT * 64u, (uint64_t)(tid >> 2), 0u, n4);
                    e_act = w4 == 0 ? n4[0] : w4 == 1 ? n4[1] : w4 == 2 ? n4[2] : n4[3];
                    sd_act = sqrtf(svar);
                    act = tanhf(smu + sd_act * e_act);                   // :218-219
                }
                const double s_act = block_sum<double, 4>((double)act, scratch);             // (act = 0 beyond O)
                m_act = (float)(s_act / (double)O);                      // outer(b, act).mean(-1) = b * mean(act)   :220-221
                zb = s_zb[0];
                double s_rb = 0.0;
                if (vi) {
                    const float b1v = Vn[3].p, b2v = Vn[4].p;
                    const float lvr = b2v * m_act;
                    dlt = zb - b1v * m_act;
                    s_rb = (double)(-0.5f * 1.1447298858494002f - 0.5f * lvr - 0.5f * ((dlt * dlt) / expf(lvr)));   // :223-224
                    eb = expf(-b2v * m_act);
                    S_aux = (double)(-0.5f * b2v + dlt * b1v * eb + 0.5f * dlt * dlt * b2v * eb);   // d log_rb / d m (V1 negates it)
                    S_zb = (double)(dlt * eb);
                }
                block_sum3(s_rb, S_aux, S_zb, scr3);                     // (... and gl / gvl are free for the tiles)
                kl = (float)(kl_sum + ((-(double)ldq + (double)(float)lq0) - ((double)ldr + s_rb)));   // :215, :225, :235
            }

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
                        if constexpr (MNF) sm = __builtin_fmaf(xv * zfs[i], we[i], sm);      // x * z_k   :197
                        else sm = __builtin_fmaf(xv, we[i], sm);
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
                if constexpr (MNF) {                                    // vector_bwd.hip V1: d loss / d act_mu, d act_var
                    if (tid < O) {
                        const float cm = kl_scale * (float)(-S_aux) / (float)O;             // kl = ... - log_rb
                        const float d = cm * (1.f - act * act);
                        dams[tid] = d;
                        davs[tid] = d * e_act / (2.f * sd_act);
                    }
                    __syncthreads();
                }
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    if (own[j] < 0) continue;
                    float g3[3] = {0.f, 0.f, 0.f};
                    int nq = 3;
                    if (MNF && ei[j] < I) {                             // elem_bwd.h with the step's z_fwd, z_kl, r0_c
                        float czf, czk, crc;
                        elem_bwd(Pp[j][0], Pp[j][1], Pp[j][2], am[j], av[j], zfs[ei[j]], zks[ei[j]], rcs[ei[j]], dams[eo[j]],
                                 davs[eo[j]], ce, true, true, g3[0], g3[1], g3[2], czf, czk, crc);
                        gl[own[j]] = czf; gl[MAXE + own[j]] = czk; gl[2 * MAXE + own[j]] = crc;
                    } else if (ei[j] < I) {                             // weight_pass_bwd.hip elem_bwd with z = 1, g_kl = kl_scale
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
                if constexpr (MNF) {
                    __syncthreads();                                    // the elements' column terms are in gl
                    const float G = kl_scale;
                    float dzf = 0.f, dzk = 0.f, drc = 0.f;
                    if (vi)
                        for (int o = 0; o < O; ++o) {                   // unit order
                            dzf += gl[o * I1 + tid]; dzk += gl[MAXE + o * I1 + tid]; drc += gl[2 * MAXE + o * I1 + tid];
                        }
                    // ---- vector_bwd.hip V2 (flow_planar_backward_body), the work vectors in registers
                    float gV[5], gZu[MT], gZw[MT], gZb[MT], gRu[MT], gRw[MT], gRb[MT];
                    gV[2] = drc;
                    gV[3] = -G * dlt * m_act * eb;                                           // log_rb: r0_b1, r0_b2
                    gV[4] = -G * (-0.5f * m_act + 0.5f * dlt * dlt * m_act * eb);
                    float DK = tid == I - 1 ? G * (float)S_zb : 0.f;                         // -G * dlog_rb / dzb
#pragma unroll
                    for (int t = MT - 1; t >= 0; --t) {                 // r flow backward (multiplier on log_det_r is -G)
                        gRu[t] = 0.f; gRw[t] = 0.f; gRb[t] = 0.f;
                        if (t < Tr) {
                            double d1 = (double)(DK * Ru[t].p), z0 = 0.0, z1 = 0.0;
                            block_sum3(d1, z0, z1, scr3);
                            const float th = thR[t], psi = 1.f - th * th, uw = uwR[t], D = 1.f + psi * uw;
                            const float dth = (float)d1 + (-G) * (-2.f * th * uw) / D;
                            const float din = dth * psi, cc = (-G) * psi / D;
                            gRu[t] = DK * th + cc * Rw[t].p;
                            gRw[t] = din * RR[t] + cc * Ru[t].p;
                            DK = DK + din * Rw[t].p;
                            gRb[t] = din;
                        }
                    }
                    DK += dzk;
                    float DF = dzf;
#pragma unroll
                    for (int t = MT - 1; t >= 0; --t) {                 // z flow backward on both draws (log_det_q: -G)
                        gZu[t] = 0.f; gZw[t] = 0.f; gZb[t] = 0.f;
                        if (t < Tz) {
                            double dk = (double)(DK * Zu[t].p), df = (double)(DF * Zu[t].p), z0 = 0.0;
                            block_sum3(dk, df, z0, scr3);
                            const float uw = uwZ[t];
                            const float tk = thK[t], psik = 1.f - tk * tk, Dk = 1.f + psik * uw;
                            const float dthk = (float)dk + (-G) * (-2.f * tk * uw) / Dk;
                            const float dink = dthk * psik, ck = (-G) * psik / Dk;
                            const float tf = thF[t], dinf = (float)df * (1.f - tf * tf);
                            gZu[t] = DK * tk + ck * Zw[t].p + DF * tf;
                            gZw[t] = dink * ZK[t] + ck * Zu[t].p + dinf * ZF[t];
                            DK = DK + dink * Zw[t].p;
                            DF = DF + dinf * Zw[t].p;
                            gZb[t] = dink + dinf;
                        }
                    }
                    gV[0] = DK + DF;                                    // q0: dlog_q0 / dlog_var = -1/2 exactly
                    gV[1] = 0.5f * sd0 * (DK * ek + DF * ef) - 0.5f * G;
                    const auto adam = [&](PMV& s, float g, float rate) {                     // adam.hip's update
                        const float gq = g + wd * s.p;
                        s.m = b1 * s.m + (1.f - b1) * gq;
                        s.v = b2 * s.v + (1.f - b2) * gq * gq;
                        const float denom = sqrtf(s.v) / bc2s + eps_adam;
                        s.p = s.p - (rate / bc1) * (s.m / denom);
                    };
                    if (vi) {
#pragma unroll
                        for (int q = 0; q < 5; ++q) adam(Vn[q], gV[q], lr);
                    }
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        if (t < Tz) { if (vi) { adam(Zu[t], gZu[t], lr_z); adam(Zw[t], gZw[t], lr_z); } adam(Zb[t], gZb[t], lr_z); }
                        if (t < Tr) { if (vi) { adam(Ru[t], gRu[t], lr_r); adam(Rw[t], gRw[t], lr_r); } adam(Rb[t], gRb[t], lr_r); }
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
    if constexpr (MNF) {
        if (vi) {
#pragma unroll
            for (int q = 0; q < 5; ++q) st_pmv(Vn[q], P0 + q * I + tid);
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int zo = P0 + 5 * I + t * (2 * I + 1), ro = P0 + 5 * I + (Tz + t) * (2 * I + 1);
            if (t < Tz) { if (vi) { st_pmv(Zu[t], zo + tid); st_pmv(Zw[t], zo + I + tid); } if (tid == 0) st_pmv(Zb[t], zo + 2 * I); }
            if (t < Tr) { if (vi) { st_pmv(Ru[t], ro + tid); st_pmv(Rw[t], ro + I + tid); } if (tid == 0) st_pmv(Rb[t], ro + 2 * I); }
        }
    }
    if (tid == 0) { a.step[r] = step_f; a.rng[2 * (size_t)r + 1] = offs; a.skipped[r] = skipped; }
}

inline bool off4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }
inline bool off8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

// the checks both entries make, in their order: NULL, shape, alignment; 1: nothing to launch
template <typename Args>
int check_args(const Args* p, int Tz, int Tr) {
    if (!p) return LBBNN_E_NULL;
    const Args& a = *p;
    if (!a.params || !a.exp_avg || !a.exp_avg_sq || !a.step || !a.rng || !a.skipped || !a.x || !a.y || !a.priors || !a.hyper ||
        !a.lr || !a.history || (a.n_restarts > 0 && !a.restarts))
        return LBBNN_E_NULL;
    if (a.I < 1 || a.I > LBBNN_STUDY_MAX_I || a.O < 1 || a.O > LBBNN_STUDY_MAX_O || a.O * a.I > LBBNN_STUDY_MAX_WEIGHTS)
        return LBBNN_E_SHAPE;
    if (Tz < 0 || Tz > LBBNN_STUDY_MAX_TRANSFORMS || Tr < 0 || Tr > LBBNN_STUDY_MAX_TRANSFORMS) return LBBNN_E_SHAPE;
    if (a.batch < 1 || a.batch > LBBNN_STUDY_MAX_BATCH || a.N < 1 || a.R < 1 || a.R > 65535) return LBBNN_E_SHAPE;
    if (a.n_epochs < 0 || a.first_epoch < 0 || a.epochs < 1 || (long long)a.first_epoch + a.n_epochs > a.epochs || a.n_restarts < 0)
        return LBBNN_E_SHAPE;
    if ((a.x_rstride != 0 && a.x_rstride < (int64_t)a.N * a.I) || (a.y_rstride != 0 && a.y_rstride < (int64_t)a.N * a.O) ||
        (a.priors_rstride != 0 && a.priors_rstride != 1) || (a.lr_rstride != 0 && a.lr_rstride < a.epochs))
        return LBBNN_E_SHAPE;
    if (off4(a.params) || off4(a.exp_avg) || off4(a.exp_avg_sq) || off4(a.step) || off8(a.rng) || off8(a.skipped) || off4(a.x) ||
        off4(a.y) || off4(a.priors) || off4(a.hyper) || off4(a.lr) || off4(a.restarts) || off8(a.history))
        return LBBNN_E_ALIGN;
    return a.n_epochs == 0 ? 1 : 0;
}

}  // namespace

extern "C" int lbbnn_lrt_study_fit(const lbbnn_study_args_t* p, void* stream) {
    const int rc = check_args(p, 0, 0);
    if (rc != 0) return rc < 0 ? rc : 0;
    hipLaunchKernelGGL((study_kernel<false, lbbnn_study_args_t>), dim3((unsigned)p->R), dim3(NT), 0, static_cast<hipStream_t>(stream), *p);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_mnf_study_fit(const lbbnn_mnf_study_args_t* p, void* stream) {
    const int rc = check_args(p, p ? p->Tz : 0, p ? p->Tr : 0);
    if (rc != 0) return rc < 0 ? rc : 0;
    hipLaunchKernelGGL((study_kernel<true, lbbnn_mnf_study_args_t>), dim3((unsigned)p->R), dim3(NT), 0, static_cast<hipStream_t>(stream), *p);
    return (int)hipGetLastError();
}
