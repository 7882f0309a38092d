// Frozen evaluation model of a baseline LBBNN network (gfx950), see include/lbbnn.h: the snapshot planes taken once
// (lbbnn_base_frozen_operands) and every member's weights and biases drawn from them (lbbnn_base_frozen_members).  Both take an
// optional compact map (sorted rows / cols of the full layer, evaluate.live_structure); without one the map is the identity.
//
// Work split of both kernels: ONE WAVE PER (COMPACT) OUTPUT ROW, kBfRows rows per workgroup, the rows of all layers
// concatenated on gridDim.x.  A lane owns the groups of EIGHT consecutive compact columns lane, lane + 64, ... of its row: a
// group is two float4 of every fp32 plane, or one 16-B hi unit and one 16-B lo unit of the split layout (lbbnn_device.h) -- the
// store8 / store8_operand of operand_store.h (the store shapes of gate_members_kernel, gate_vd.hip), no exchange between lanes.
// No LDS, no atomics; row sums are DPP wave sums.
//
//   base_frozen_operands_kernel -- sources gathered at (rows[o'], cols[j']) (float4 loads when there is no map and the rows
//     allow it), sigma / alpha by softplus_ref / sigmoid_ref: the functions, hence the bits, of gate_members_kernel.
//   base_frozen_members_kernel -- gridDim.y strides over the members; per group the planes and the column indices are read
//     once and every member of the stride is drawn from them.  The Philox counter of compact column j' is the FULL one,
//     (rows[o'], cols[j'] / 4): sorted cols keep the columns of one full quad adjacent, so a new evaluation is made only when
//     the quad changes (identity map: one per float4, as gate_members_kernel).  MPM mode: a float4 whose w_mu and w_sigma are
//     all zero draws nothing.
// The draw (gate_draw, uniform24), the scalar bf16 split, layer_of and map_index are operand_store.h's: the ones the live
// kernels and frozen.hip use.
#include <climits>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "operand_store.h"

namespace {

using namespace lbbnn;

constexpr int kBfRows = 4;                 // rows (= waves) per workgroup
constexpr int kBfNT = 64 * kBfRows;
constexpr int kBfMaxLd = 4096;             // GATE_MEMBERS_MAX_LD: the widest row of lbbnn_gate_members

struct BfLayer {
    const float* mu; const float* rho; const float* lambdal; const float* bias_mu; const float* bias_rho;
    const int32_t* rows; const int32_t* cols;            // both NULL: the identity
    float* w_mu; float* w_sigma; float* alpha; void* e_w; float* b_mu; float* b_sigma;
    int32_t* kept_rows; float* alpha_rows; uint8_t* keep;
    void* w_out; float* bias_out; float* gate_rows;      // members call
    int O, I, ld, O_full, I_full, split, hard, vec;
    uint32_t layer_id;
};
struct BfBatch {
    BfLayer l[LBBNN_MAX_LAYERS];
    int wg_end[LBBNN_MAX_LAYERS];
    int n, mode, members;
    float threshold, temperature;
    uint64_t member_advance;
};

// element `k` (0..3) of a register quad without indexing memory
__device__ __forceinline__ float pick4(const float v[4], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3]; }
__device__ __forceinline__ uint32_t pick4(const Philox4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }


__global__ __launch_bounds__(kBfNT) void base_frozen_operands_kernel(const BfBatch bt_) {
    const LBBNN_CONST_AS BfBatch* bt = kernarg_as<BfBatch>();
    int wg0;
    const int li = layer_of(bt, wg0);
    const LBBNN_CONST_AS BfLayer& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kBfRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;                                                 // (whole waves leave: no barrier below)
    const int I = a.I, ld = a.ld, If = a.I_full;
    const bool mpm = bt->mode == LBBNN_GATES_MPM, split = a.split != 0, vec = a.vec != 0;
    const float thr = bt->threshold;
    const int r = map_index(a.rows, o, a.O_full);
    const size_t rowoff = (size_t)r * If;
    const float* mu_r = a.mu + rowoff; const float* rho_r = a.rho + rowoff; const float* lam_r = a.lambdal + rowoff;
    float asum = 0.f;
    int kept = 0;
    for (int i0 = 8 * lane; i0 < ld; i0 += 8 * 64) {
        float mu[8], rho[8], lam[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { mu[e] = 0.f; rho[e] = 0.f; lam[e] = 0.f; }
        if (vec) {                                                        // no map, I % 4 == 0: a float4 is wholly in or out
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (i0 + 4 * q >= I) continue;
                const float4 m4 = *reinterpret_cast<const float4*>(mu_r + i0 + 4 * q);
                const float4 r4 = *reinterpret_cast<const float4*>(rho_r + i0 + 4 * q);
                const float4 l4 = *reinterpret_cast<const float4*>(lam_r + i0 + 4 * q);
                mu[4 * q] = m4.x; mu[4 * q + 1] = m4.y; mu[4 * q + 2] = m4.z; mu[4 * q + 3] = m4.w;
                rho[4 * q] = r4.x; rho[4 * q + 1] = r4.y; rho[4 * q + 2] = r4.z; rho[4 * q + 3] = r4.w;
                lam[4 * q] = l4.x; lam[4 * q + 1] = l4.y; lam[4 * q + 2] = l4.z; lam[4 * q + 3] = l4.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (i0 + e < I) {
                    const int c = map_index(a.cols, i0 + e, If);
                    mu[e] = mu_r[c]; rho[e] = rho_r[c]; lam[e] = lam_r[c];
                }
            }
        }
        float wm[8], ws[8], al[8], ew[8];
        uint32_t kbits = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool in = i0 + e < I;
            const float sigma = softplus_ref(rho[e]), alpha = sigmoid_ref(lam[e]);
            const bool keep = in && (alpha > thr);                        // fp32; NaN is never kept
            al[e] = in ? alpha : 0.f;
            wm[e] = in && (!mpm || keep) ? mu[e] : 0.f;
            ws[e] = in && (!mpm || keep) ? sigma : 0.f;
            ew[e] = mpm ? wm[e] : al[e] * mu[e];                          // medimean :236-238 / the mode-2 mean alpha * mu
            asum += al[e];
            kept += keep ? 1 : 0;
            kbits |= keep ? (1u << e) : 0u;
        }
        if (a.w_mu) store8(a.w_mu, o, i0, ld, wm);
        if (a.w_sigma) store8(a.w_sigma, o, i0, ld, ws);
        if (a.alpha) store8(a.alpha, o, i0, ld, al);
        if (a.e_w) store8_operand(a.e_w, split, (size_t)o, i0, ld, ew);
        if (a.keep) {                                                     // identity map: row r = o, column = i0 + e
            uint8_t* const kp = a.keep + rowoff;
#pragma unroll
            for (int e = 0; e < 8; ++e) if (i0 + e < I) kp[i0 + e] = (uint8_t)((kbits >> e) & 1u);
        }
    }
    const float atot = wave_sum(asum);
    const int ktot = (int)wave_sum((float)kept);                          // per-lane counts are < 2^24: their float sum is exact
    if (lane == 0) {
        if (a.alpha_rows) a.alpha_rows[o] = atot;
        if (a.kept_rows) a.kept_rows[o] = ktot;
        if (a.b_mu) a.b_mu[o] = a.bias_mu[r];
        if (a.b_sigma) a.b_sigma[o] = softplus_ref(a.bias_rho[r]);
    }
}

__global__ __launch_bounds__(kBfNT) void base_frozen_members_kernel(const BfBatch bt_, const uint64_t* rng) {
    const LBBNN_CONST_AS BfBatch* bt = kernarg_as<BfBatch>();
    int wg0;
    const int li = layer_of(bt, wg0);
    const LBBNN_CONST_AS BfLayer& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kBfRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;
    const int I = a.I, ld = a.ld, If = a.I_full, members = bt->members;
    const int m0 = blockIdx.y, mstep = gridDim.y;
    const bool sample = bt->mode == LBBNN_GATES_SAMPLE, hard = a.hard != 0, split = a.split != 0;
    const float T = bt->temperature;
    const uint64_t seed = rng[0], off0 = rng[1], adv = bt->member_advance;
    const uint32_t lid = a.layer_id;
    const uint32_t s_gate = LBBNN_STREAM_GATE * 64u + lid, s_w = LBBNN_STREAM_EPS_W * 64u + lid;
    const int r = map_index(a.rows, o, a.O_full);

    // the member biases, at the full row's counter: lane t draws those of members t, t + 64, ... (first member stride only)
    if (m0 == 0) {
        const float bm = a.b_mu[o], sb = a.b_sigma[o];
        for (int m = lane; m < members; m += 64) {
            float n[4];
            philox_normal4(seed, off0 + (uint64_t)m * adv, LBBNN_STREAM_EPS_B * 64u + lid, (uint64_t)(r >> 2), 0u, n);
            a.bias_out[(size_t)m * a.O + o] = bm + sb * pick4(n, r & 3);                       // :234
        }
    }

    const int G = (ld + 511) >> 9;
    for (int gidx = 0; gidx < G; ++gidx) {                                // wave-uniform trip count: the row sum below is a wave op
        const int i0 = 8 * (lane + 64 * gidx);
        float wm[8], ws[8], al[8];
        int col[8];
        bool any[2] = {false, false};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 m4 = zero4, s4 = zero4, a4 = zero4;
            if (i0 + 4 * q < I) {                                         // the planes' tails are zeros: a float4 read is whole
                m4 = *reinterpret_cast<const float4*>(a.w_mu + (size_t)o * ld + i0 + 4 * q);
                s4 = *reinterpret_cast<const float4*>(a.w_sigma + (size_t)o * ld + i0 + 4 * q);
                if (sample) a4 = *reinterpret_cast<const float4*>(a.alpha + (size_t)o * ld + i0 + 4 * q);
            }
            wm[4 * q] = m4.x; wm[4 * q + 1] = m4.y; wm[4 * q + 2] = m4.z; wm[4 * q + 3] = m4.w;
            ws[4 * q] = s4.x; ws[4 * q + 1] = s4.y; ws[4 * q + 2] = s4.z; ws[4 * q + 3] = s4.w;
            al[4 * q] = a4.x; al[4 * q + 1] = a4.y; al[4 * q + 2] = a4.z; al[4 * q + 3] = a4.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * q + e;
                col[k] = (i0 + k < I) ? map_index(a.cols, i0 + k, If) : -1;
                any[q] = any[q] || (i0 + k < I && (sample || wm[k] != 0.f || ws[k] != 0.f));
            }
        }
        for (int m = m0; m < members; m += mstep) {
            const uint64_t offs = off0 + (uint64_t)m * adv;
            float w[8];
            float gsum = 0.f;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
#pragma unroll
                for (int e = 0; e < 4; ++e) w[4 * q + e] = 0.f;
                if (!any[q]) continue;                                    // past I, or (MPM) nothing kept: no draw, zeros
                float n[4] = {0.f, 0.f, 0.f, 0.f};
                Philox4 ub = {0u, 0u, 0u, 0u};
                int quad = -1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * q + e, c = col[k];
                    if (c < 0) continue;
                    if ((c >> 2) != quad) {                               // sorted cols: one evaluation per full quad touched
                        quad = c >> 2;
                        philox_normal4(seed, offs, s_w, (uint64_t)r, (uint32_t)quad, n);
                        if (sample) ub = philox_bits4(seed, offs, s_gate, (uint64_t)r, (uint32_t)quad);
                    }
                    const float ek = pick4(n, c & 3), sigma = ws[k], mu_k = wm[k];
                    if (sample) {
                        float dcda;                                       // (the derivative is the backward pass's)
                        const float g = gate_draw(al[k], uniform24(pick4(ub, c & 3)), T, hard, &dcda);
                        w[k] = g * (mu_k + sigma * ek);                                         // :232-233
                        gsum += g;
                    } else {
                        w[k] = mu_k + sigma * ek;
                    }
                }
            }
            if (i0 < ld) store8_operand(a.w_out, split, (size_t)m * a.O + o, i0, ld, w);
            if (a.gate_rows) {                                            // one wave owns the row: plain read-add-write, in order
                const float s = wave_sum(gsum);
                float* const p = a.gate_rows + (size_t)m * a.O + o;
                if (lane == 0) *p = gidx ? *p + s : s;
            }
        }
    }
}

// the shape, alignment and map checks both entry points make of a layer, and the fields both kernels read
int fill_layer(BfLayer& a, const lbbnn_base_frozen_desc_t& d, const lbbnn_compact_map_t* m) {
    if (d.O <= 0 || d.I <= 0 || d.ld < d.I || d.ld > kBfMaxLd) return LBBNN_E_SHAPE;
    if (d.ld & 31) return LBBNN_E_ALIGN;
    if (d.flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
    if (!aligned16(d.w_mu) || !aligned16(d.w_sigma) || !aligned16(d.alpha) || !aligned16(d.e_w)) return LBBNN_E_ALIGN;
    if (!aligned4(d.b_mu) || !aligned4(d.b_sigma) || !aligned4(d.kept_rows) || !aligned4(d.alpha_rows)) return LBBNN_E_ALIGN;
    a = BfLayer{};
    a.O = d.O; a.I = d.I; a.ld = d.ld; a.O_full = d.O; a.I_full = d.I;
    if (m) {
        if (!m->rows || !m->cols) return LBBNN_E_NULL;
        if (m->O_full <= 0 || m->I_full <= 0 || d.O > m->O_full || d.I > m->I_full) return LBBNN_E_SHAPE;
        if (!aligned4(m->rows) || !aligned4(m->cols)) return LBBNN_E_ALIGN;
        a.rows = m->rows; a.cols = m->cols; a.O_full = m->O_full; a.I_full = m->I_full;
    }
    a.w_mu = d.w_mu; a.w_sigma = d.w_sigma; a.alpha = d.alpha; a.e_w = d.e_w; a.b_mu = d.b_mu; a.b_sigma = d.b_sigma;
    a.split = (d.flags & LBBNN_F_SPLIT16) ? 1 : 0;
    a.hard = (d.exact & 8) ? 1 : 0;
    a.layer_id = d.layer_id;
    return 0;
}

}  // namespace

extern "C" int lbbnn_base_frozen_operands(const lbbnn_base_frozen_desc_t* L, const lbbnn_compact_map_t* M, int n, int mode,
                                          float threshold, void* stream) {
    if (!L) return LBBNN_E_NULL;
    if (n < 1 || n > LBBNN_MAX_LAYERS) return LBBNN_E_SHAPE;
    if (mode != LBBNN_GATES_SAMPLE && mode != LBBNN_GATES_MPM) return LBBNN_E_FLAGS;
    if (M && mode == LBBNN_GATES_SAMPLE) return LBBNN_E_FLAGS;            // alpha gates are never exactly zero: nothing to drop
    if (!(threshold > 0.f && threshold < 1.f)) return LBBNN_E_FLAGS;
    BfBatch bt = {};
    int wgs = 0;
    for (int i = 0; i < n; ++i) {
        const lbbnn_base_frozen_desc_t& d = L[i];
        if (!d.mu || !d.rho || !d.lambdal || !d.bias_mu || !d.bias_rho) return LBBNN_E_NULL;
        if (!d.w_mu && !d.w_sigma && !d.alpha && !d.e_w && !d.b_mu && !d.b_sigma && !d.kept_rows && !d.alpha_rows && !d.keep)
            return LBBNN_E_NULL;
        if (d.keep && M) return LBBNN_E_FLAGS;                            // the keep plane is the full layer's
        BfLayer& a = bt.l[i];
        const int rc = fill_layer(a, d, M ? &M[i] : nullptr);
        if (rc) return rc;
        if (!aligned4(d.mu) || !aligned4(d.rho) || !aligned4(d.lambdal) || !aligned4(d.bias_mu) || !aligned4(d.bias_rho))
            return LBBNN_E_ALIGN;
        a.mu = d.mu; a.rho = d.rho; a.lambdal = d.lambdal; a.bias_mu = d.bias_mu; a.bias_rho = d.bias_rho;
        a.kept_rows = d.kept_rows; a.alpha_rows = d.alpha_rows; a.keep = d.keep;
        a.vec = !M && (d.I % 4) == 0 && aligned16(d.mu) && aligned16(d.rho) && aligned16(d.lambdal);
        wgs += (d.O + kBfRows - 1) / kBfRows;
        bt.wg_end[i] = wgs;
    }
    bt.n = n; bt.mode = mode; bt.threshold = threshold;
    hipLaunchKernelGGL(base_frozen_operands_kernel, dim3(wgs), dim3(kBfNT), 0, static_cast<hipStream_t>(stream), bt);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_base_frozen_members(const lbbnn_base_frozen_desc_t* L, const lbbnn_compact_map_t* M, int n, int members,
                                         int mode, float temperature, void* w_out[], float* bias_out[], float* gate_rows[],
                                         const uint64_t* rng, uint64_t member_advance, void* stream) {
    if (!L || !w_out || !bias_out) return LBBNN_E_NULL;
    if (n < 1 || n > LBBNN_MAX_LAYERS || members < 1 || members > 65535) return LBBNN_E_SHAPE;
    if (mode != LBBNN_GATES_SAMPLE && mode != LBBNN_GATES_MPM) return LBBNN_E_FLAGS;
    if (mode == LBBNN_GATES_SAMPLE && (M || !(temperature > 0.f))) return LBBNN_E_FLAGS;
    if (mode == LBBNN_GATES_MPM && gate_rows) return LBBNN_E_FLAGS;       // the gates of an MPM model are its planes' zeros
    BfBatch bt = {};
    int wgs = 0;
    for (int i = 0; i < n; ++i) {
        const lbbnn_base_frozen_desc_t& d = L[i];
        if (!d.w_mu || !d.w_sigma || !d.b_mu || !d.b_sigma || !w_out[i] || !bias_out[i]) return LBBNN_E_NULL;
        if (mode == LBBNN_GATES_SAMPLE && !d.alpha) return LBBNN_E_NULL;
        BfLayer& a = bt.l[i];
        const int rc = fill_layer(a, d, M ? &M[i] : nullptr);
        if (rc) return rc;
        if (!aligned16(w_out[i]) || !aligned4(bias_out[i]) || (gate_rows && !aligned4(gate_rows[i]))) return LBBNN_E_ALIGN;
        a.w_out = w_out[i]; a.bias_out = bias_out[i]; a.gate_rows = gate_rows ? gate_rows[i] : nullptr;
        wgs += (d.O + kBfRows - 1) / kBfRows;
        bt.wg_end[i] = wgs;
    }
    if (!rng) return LBBNN_E_NOISE;
    bt.n = n; bt.mode = mode; bt.members = members; bt.temperature = temperature; bt.member_advance = member_advance;
    // members on gridDim.y while the rows alone leave compute units idle (about 8 workgroups per unit), looped inside beyond that
    int my = (2048 + wgs - 1) / wgs;
    my = my < 1 ? 1 : (my > members ? members : my);
    hipLaunchKernelGGL(base_frozen_members_kernel, dim3(wgs, my), dim3(kBfNT), 0, static_cast<hipStream_t>(stream), bt, rng);
    return (int)hipGetLastError();
}
