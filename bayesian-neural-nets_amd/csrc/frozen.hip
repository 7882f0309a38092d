// Frozen evaluation model (gfx950): the GEMM operands of a trained LRT / MNF network taken ONCE from its parameters, with
// the gates as trained (alpha) or thresholded (the median probability model), see include/lbbnn.h.  Both kernels exist in
// two instantiations: the full layer, and (kMap) the compact layer of the median probability model -- the full layer's rows
// `rows` and columns `cols` (sorted index lists built on the host side from the kept masks), gathered while loading;
// everything downstream runs the existing GEMMs at the smaller shape.  Operands leave through operand_store.h in the one
// layout every writer shares: 16-B vectors into padded rows, fp32 or the bf16 hi | lo units.
//
//   frozen_operands_kernel -- lbbnn_frozen_operands / lbbnn_frozen_operands_compact: one launch over the rows of up to
//     LBBNN_MAX_LAYERS layers.  ONE WAVE PER ROW (four rows per 256-thread workgroup): a lane owns the float4 column groups
//     lane, lane + 64, ... of the (compact) row.  Full: a wave-load covers 1 KiB contiguous of each of mu / rho / lambdal,
//     four groups per lane in flight together; per weight 12 B read, 12 B (fp32: e0, e_w, var_w) or 12 B (split: e0 4 B + two
//     hi | lo operands of 4 B each) written -- a streaming kernel whose bound is HBM.  Rows that are not whole aligned float4s
//     (I % 4 != 0, or parameters off a 16-B boundary) take scalar loads of the same groups (fp32 operands only there, as K1).
//     Compact: four column indices, then four scalar loads of each of mu / rho / lambdal at (rows[o'], cols[j']), two groups
//     (12 gathered loads each) in flight; median-probability gates only, a = [lambdal > cut], fixed at compile time.
//     The arithmetic of mode 0 is K1's (k1_alpha / k1_sigma of lbbnn_device.h, the products in K1's order), so the operands
//     are the values lbbnn_weight_pass writes.  The kept count of a row is accumulated per lane, reduced with DPP moves
//     (wave_sum) and stored by lane 0 with an ordinary store: no atomics, no LDS.
//   frozen_scale_kernel -- lbbnn_frozen_members / _compact: e_w_members[m] = operand(E0 * z_m) for every member (gridDim.y)
//     and MNF layer in one launch: 4 B read (e0, L2-resident across members) and 4 B written per weight and member.  Compact:
//     E0'[o'][j'] * z_m[cols[j']], the gather of the full-width z fused in: no compact z is ever stored.
//     lbbnn_frozen_members_dense is the same launch behind lbbnn_flow_dense_members (flow_dense_members.hip) instead of the
//     planar-flow launch: the z of RNVP / MNF-type z flows.  lbbnn_frozen_members_z is the planar-flow launch WITHOUT this
//     kernel: the z of a sparse model (sparse_members.hip), which scales inside its layer kernel.
//   gather_columns_kernel -- lbbnn_gather_columns: out[b][j] = x[b][idx[j]], one thread per float4 of the output.
#include <cstdlib>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "operand_store.h"

namespace {

using namespace lbbnn;

constexpr int kFzRows = 4;                 // rows (= waves) per workgroup
constexpr int kFzNT = 64 * kFzRows;
// float4 groups per lane loaded together: 1024 weights of a row per batch; compact: 2 (12 gathered loads each)
template <bool kMap> constexpr int kFzB = kMap ? 2 : 4;

struct FrozenLayer {
    const float* mu; const float* rho; const float* lambdal; const float* bias_rho;
    float* e0; float* e_w; float* var_w; float* bias_var; int32_t* kept_rows;
    int O, I, ld, vec, split, mode;
    float cut;
    const int32_t* rows; const int32_t* cols; int O_full, I_full;       // the compact map (kMap instantiation only)
};
struct FrozenBatch { FrozenLayer l[LBBNN_MAX_LAYERS]; int wg_end[LBBNN_MAX_LAYERS]; int n; };

struct ScaleLayer {
    const float* e0; const float* z; float* e_w_members;
    long long z_ms;
    int O, I, ld, split;
    const int32_t* cols; int I_full;                                    // the compact map (kMap instantiation only)
};
struct ScaleBatch { ScaleLayer l[LBBNN_MAX_LAYERS]; int wg_end[LBBNN_MAX_LAYERS]; int n; };

__device__ __forceinline__ float4 fz_ld4(const float* p, int j) { return reinterpret_cast<const float4*>(p)[j]; }
// columns 4j .. 4j+3 of a row that is not a whole aligned float4 sequence; elements at or past I read as 0
__device__ __forceinline__ float4 fz_ld4_scalar(const float* row, int j, int I) {
    const int k = 4 * j;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < I) v.x = row[k];
    if (k + 1 < I) v.y = row[k + 1];
    if (k + 2 < I) v.z = row[k + 2];
    if (k + 3 < I) v.w = row[k + 3];
    return v;
}
// compact columns 4j .. 4j+3 of three full-width rows (If elements): one column index, then one load of each row, per
// element; elements at or past I read as 0
__device__ __forceinline__ void fz_gather4(const float* mu_r, const float* rho_r, const float* lam_r, const int32_t* cols, int j,
                                           int I, int If, float4& mu, float4& rho, float4& lam) {
    float m[4], r[4], l[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        m[t] = 0.f; r[t] = 0.f; l[t] = 0.f;
        if (4 * j + t < I) {
            const int c = clamped_index(cols, 4 * j + t, If);
            m[t] = mu_r[c]; r[t] = rho_r[c]; l[t] = lam_r[c];
        }
    }
    mu = make_float4(m[0], m[1], m[2], m[3]); rho = make_float4(r[0], r[1], r[2], r[3]); lam = make_float4(l[0], l[1], l[2], l[3]);
}

struct FzElem { float e0, v; int kept; };
// mode 0: a = alpha (K1's operands: e_w = mu * alpha, var_w = sigma^2 * alpha^2, LBBNN-GP-MF-LRT.py:170-171);
// mode 1: a = [lambdal > cut] (outofsample(medimod=True)), compared in fp32 (NaN is never kept): e0 = mu or +0.0,
// V = sigma^2 or 0 (a^2 = a)
__device__ __forceinline__ FzElem fz_elem(float mu, float rho, float lam, int mode, float cut) {
    FzElem r;
    const bool kept = lam > cut;
    const float sigma = k1_sigma(rho);
    const float s2 = sigma * sigma;
    r.kept = kept ? 1 : 0;
    if (mode == 0) {
        const float alpha = k1_alpha(lam);
        r.e0 = mu * alpha;
        r.v = s2 * (alpha * alpha);
    } else {
        r.e0 = kept ? mu : 0.f;
        r.v = kept ? s2 : 0.f;
    }
    return r;
}

template <bool kMap>
__global__ __launch_bounds__(kFzNT) void frozen_operands_kernel(const FrozenBatch bt_) {
    constexpr int kB = kFzB<kMap>;
    const LBBNN_CONST_AS FrozenBatch* bt = kernarg_as<FrozenBatch>();
    int wg0;
    const int li = layer_of(bt, wg0);
    const LBBNN_CONST_AS FrozenLayer& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kFzRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;                                                 // (whole waves leave: no barrier below)
    const int I = a.I, P = a.ld, nq = P >> 2;
    const int iq = (I + 3) >> 2;                                          // groups holding at least one weight
    const int G = (nq + 63) >> 6;
    const bool vec = a.vec != 0, split = a.split != 0;
    const int mode = kMap ? LBBNN_FROZEN_MPM : a.mode;                    // compact: no alpha path is generated
    const float cut = a.cut;
    const int r = kMap ? clamped_index(a.rows, o, a.O_full) : o;              // the full layer's row
    const int If = kMap ? a.I_full : I;
    const size_t rowoff = (size_t)r * If;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int kept = 0;
    for (int g0 = 0; g0 < G; g0 += kB) {
        float4 mu[kB], rho[kB], lam[kB];
#pragma unroll
        for (int g = 0; g < kB; ++g) {
            const int j = lane + 64 * (g0 + g);
            mu[g] = zero4; rho[g] = zero4; lam[g] = zero4;
            if constexpr (kMap) {                                         // (guarded per element)
                fz_gather4(a.mu + rowoff, a.rho + rowoff, a.lambdal + rowoff, a.cols, j, I, If, mu[g], rho[g], lam[g]);
            } else if (j < iq) {
                if (vec) { mu[g] = fz_ld4(a.mu + rowoff, j); rho[g] = fz_ld4(a.rho + rowoff, j); lam[g] = fz_ld4(a.lambdal + rowoff, j); }
                else {
                    mu[g] = fz_ld4_scalar(a.mu + rowoff, j, I); rho[g] = fz_ld4_scalar(a.rho + rowoff, j, I);
                    lam[g] = fz_ld4_scalar(a.lambdal + rowoff, j, I);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < kB; ++g) {
            if (g0 + g >= G) break;                                       // wave-uniform
            const int j = lane + 64 * (g0 + g);
            float4 e0 = zero4, vw = zero4;
            if (j < iq) {
                const FzElem x = fz_elem(mu[g].x, rho[g].x, lam[g].x, mode, cut), y = fz_elem(mu[g].y, rho[g].y, lam[g].y, mode, cut);
                const FzElem z = fz_elem(mu[g].z, rho[g].z, lam[g].z, mode, cut), w = fz_elem(mu[g].w, rho[g].w, lam[g].w, mode, cut);
                // the zero tail of a partial group (I % 4 != 0): masked here, not by the loads' zeros -- with a negative
                // cut a zero-filled lambdal would count as kept
                const int k = 4 * j;
                const bool ky = k + 1 < I, kz = k + 2 < I, kw = k + 3 < I;
                e0 = make_float4(x.e0, ky ? y.e0 : 0.f, kz ? z.e0 : 0.f, kw ? w.e0 : 0.f);
                vw = make_float4(x.v, ky ? y.v : 0.f, kz ? z.v : 0.f, kw ? w.v : 0.f);
                kept += x.kept + (ky ? y.kept : 0) + (kz ? z.kept : 0) + (kw ? w.kept : 0);
            }
            const bool in = j < nq;
            if (in) reinterpret_cast<float4*>(a.e0 + (size_t)o * P)[j] = e0;
            store4_operand(a.e_w, o, j, P, split, in, e0);
            store4_operand(a.var_w, o, j, P, split, in, vw);
        }
    }
    // per-lane counts are < 2^24: their float sum is exact
    const int total = (int)wave_sum((float)kept);
    if (lane == 0) {
        a.kept_rows[o] = total;
        const float sb = softplus_ref(a.bias_rho[r]);
        a.bias_var[o] = sb * sb;                      // bias.sigma**2 of the full row, LBBNN-GP-MF-LRT.py:173 (never gated)
    }
}

template <bool kMap>
__global__ __launch_bounds__(kFzNT) void frozen_scale_kernel(const ScaleBatch bt_) {
    constexpr int kB = kFzB<kMap>;
    const LBBNN_CONST_AS ScaleBatch* bt = kernarg_as<ScaleBatch>();
    int wg0;
    const int li = layer_of(bt, wg0);
    const LBBNN_CONST_AS ScaleLayer& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kFzRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;
    const int mem = blockIdx.y;
    const int P = a.ld, nq = P >> 2, iq = a.I >> 2;                       // I % 4 == 0 (checked on the host)
    const int G = (nq + 63) >> 6;
    const bool split = a.split != 0;
    const float* z = a.z + (size_t)mem * a.z_ms;
    float* out = a.e_w_members + (size_t)mem * a.O * P;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g0 = 0; g0 < G; g0 += kB) {
        float4 e[kB], zz[kB];
#pragma unroll
        for (int g = 0; g < kB; ++g) {
            const int j = lane + 64 * (g0 + g);
            e[g] = zero4; zz[g] = zero4;
            if (j < iq) {
                e[g] = fz_ld4(a.e0 + (size_t)o * P, j);
                if constexpr (kMap) {
                    const int If = a.I_full;
                    zz[g] = make_float4(z[clamped_index(a.cols, 4 * j, If)], z[clamped_index(a.cols, 4 * j + 1, If)],
                                        z[clamped_index(a.cols, 4 * j + 2, If)], z[clamped_index(a.cols, 4 * j + 3, If)]);
                } else {
                    zz[g] = fz_ld4(z, j);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < kB; ++g) {
            if (g0 + g >= G) break;
            const int j = lane + 64 * (g0 + g);
            // (mu * a) * z_k: the mean operand of an MNF layer (LBBNN-GP-MF-MNF.py:195,197), K1's order of products
            const float4 w = make_float4(e[g].x * zz[g].x, e[g].y * zz[g].y, e[g].z * zz[g].z, e[g].w * zz[g].w);
            store4_operand(out, o, j, P, split, j < nq, w);
        }
    }
}

__global__ __launch_bounds__(256) void gather_columns_kernel(const float* __restrict__ x, int ldx, const int32_t* __restrict__ idx,
                                                             int n_idx, float* __restrict__ out, int ldo, long long items) {
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int nq = ldo >> 2;
    const long long b = it / nq;
    const int k = 4 * (int)(it - b * nq);
    const float* row = x + (size_t)b * ldx;
    float v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = (k + t < n_idx) ? row[clamped_index(idx, k + t, ldx)] : 0.f;   // zero tail [n_idx, ldo)
    reinterpret_cast<float4*>(out + (size_t)b * ldo)[k >> 2] = make_float4(v[0], v[1], v[2], v[3]);
}

// the checks the compact entry points make of a layer's map
inline int check_map(const lbbnn_compact_map_t& m, int O, int I) {
    if (!m.rows || !m.cols) return LBBNN_E_NULL;
    if (m.O_full <= 0 || m.I_full <= 0 || O > m.O_full || I > m.I_full) return LBBNN_E_SHAPE;
    if (!aligned4(m.rows) || !aligned4(m.cols)) return LBBNN_E_ALIGN;
    return 0;
}

// lbbnn_frozen_operands (M == NULL) and lbbnn_frozen_operands_compact (M: one map per layer)
int frozen_operands_impl(const lbbnn_frozen_desc_t* L, const lbbnn_compact_map_t* M, int n, void* stream) {
    if (!L) return LBBNN_E_NULL;
    if (n <= 0 || n > LBBNN_MAX_LAYERS) return LBBNN_E_SHAPE;
    FrozenBatch bt = {};
    int wgs = 0;
    for (int i = 0; i < n; ++i) {
        const lbbnn_frozen_desc_t& d = L[i];
        if (!d.weight_mu || !d.weight_rho || !d.lambdal || !d.bias_rho || !d.e0 || !d.e_w || !d.var_w || !d.bias_var ||
            !d.kept_rows) return LBBNN_E_NULL;
        if (d.O <= 0 || d.I <= 0 || d.ld < d.I) return LBBNN_E_SHAPE;
        if (d.ld & 31) return LBBNN_E_ALIGN;
        if (!aligned16(d.e0) || !aligned16(d.e_w) || !aligned16(d.var_w)) return LBBNN_E_ALIGN;
        if (!aligned4(d.weight_mu) || !aligned4(d.weight_rho) || !aligned4(d.lambdal) || !aligned4(d.bias_rho) ||
            !aligned4(d.bias_var) || !aligned4(d.kept_rows)) return LBBNN_E_ALIGN;
        if (d.flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
        // a compact model has median-probability gates only: alpha gates are never exactly zero, nothing to drop
        if (d.mode != LBBNN_FROZEN_MPM && (M || d.mode != LBBNN_FROZEN_ALPHA)) return LBBNN_E_FLAGS;
        FrozenLayer& a = bt.l[i];
        a.split = (d.flags & LBBNN_F_SPLIT16) ? 1 : 0;
        if (M) {
            const int rc = check_map(M[i], d.O, d.I);
            if (rc) return rc;
            if (a.split && (d.I & 7)) return LBBNN_E_ALIGN;             // the bf16 hi | lo kernels' rule (I % 8)
            a.rows = M[i].rows; a.cols = M[i].cols; a.O_full = M[i].O_full; a.I_full = M[i].I_full;
        } else {
            a.vec = (d.I % 4 == 0 && aligned16(d.weight_mu) && aligned16(d.weight_rho) && aligned16(d.lambdal)) ? 1 : 0;
            if (a.split && !a.vec) return LBBNN_E_ALIGN;                // split operands need whole aligned float4 rows, as K1
        }
        a.mu = d.weight_mu; a.rho = d.weight_rho; a.lambdal = d.lambdal; a.bias_rho = d.bias_rho;
        a.e0 = d.e0; a.e_w = static_cast<float*>(d.e_w); a.var_w = static_cast<float*>(d.var_w);
        a.bias_var = d.bias_var; a.kept_rows = d.kept_rows;
        a.O = d.O; a.I = d.I; a.ld = d.ld; a.mode = d.mode; a.cut = d.cut;
        wgs += (d.O + kFzRows - 1) / kFzRows;
        bt.wg_end[i] = wgs;
    }
    bt.n = n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (M) hipLaunchKernelGGL(frozen_operands_kernel<true>, dim3(wgs), dim3(kFzNT), 0, s, bt);
    else hipLaunchKernelGGL(frozen_operands_kernel<false>, dim3(wgs), dim3(kFzNT), 0, s, bt);
    return (int)hipGetLastError();
}

// the per-member part of a frozen model: the z flows of the MNF layers (planar: d.z_flow; dense: F, lbbnn_flow_dense_members),
// then frozen_scale_kernel.  M (optional): the layers are compact; the flow runs, and z lies, at the FULL width, so member m's
// z is the full model's, bit for bit.  z_only (lbbnn_frozen_members_z): the flow launch alone -- e0, e_w_members, ld and flags
// are neither checked nor read, and nothing is scaled.
int frozen_members_impl(const lbbnn_frozen_desc_t* L, const lbbnn_dense_members_t* F, bool dense, const lbbnn_compact_map_t* M,
                        int n, int members, const uint64_t* rng, uint64_t member_advance, void* stream, bool z_only = false) {
    if (!L || (dense && !F)) return LBBNN_E_NULL;
    if (n <= 0 || n > LBBNN_MAX_LAYERS || members < 1 || members > 65535) return LBBNN_E_SHAPE;
    FlowArgs fa[LBBNN_MAX_LAYERS];
    lbbnn_dense_members_t fd[LBBNN_MAX_LAYERS];
    ScaleBatch bt = {};
    int nf = 0, wgs = 0;
    bool one_stride = true;
    for (int i = 0; i < n; ++i) {
        const lbbnn_frozen_desc_t& d = L[i];
        if (!d.q0_mean) continue;                           // an LRT layer: its e_w is shared by every member
        if (!d.q0_log_var || !d.z_fwd || (!z_only && (!d.e0 || !d.e_w_members))) return LBBNN_E_NULL;
        if (!dense) {
            if (d.z_flow.T < 0 || d.z_flow.T > LBBNN_MAX_FLOW_T) return LBBNN_E_SHAPE;
            for (int t = 0; t < d.z_flow.T; ++t)
                if (!d.z_flow.u[t] || !d.z_flow.w[t] || !d.z_flow.b[t]) return LBBNN_E_NULL;
        }
        if (!rng) return LBBNN_E_NOISE;
        if (d.O <= 0 || d.I <= 0 || (!z_only && d.ld < d.I) || (!M && d.I > LBBNN_MAX_FLOW_DIM)) return LBBNN_E_SHAPE;
        int If = d.I;                                       // the width of the flow and of z
        if (M) {
            const int rc = check_map(M[i], d.O, d.I);
            if (rc) return rc;
            If = M[i].I_full;
            if (If > LBBNN_MAX_FLOW_DIM) return LBBNN_E_SHAPE;
        }
        if (d.z_mstride < If) return LBBNN_E_SHAPE;
        if ((!z_only && (d.ld & 31)) || (d.I & 3) || (If & 3) || (d.z_mstride & 3)) return LBBNN_E_ALIGN;
        if ((!z_only && (!aligned16(d.e0) || !aligned16(d.e_w_members))) || !aligned16(d.z_fwd)) return LBBNN_E_ALIGN;
        if (!z_only && (d.flags & ~LBBNN_F_SPLIT16)) return LBBNN_E_FLAGS;
        if (M && (d.flags & LBBNN_F_SPLIT16) && (d.I & 7)) return LBBNN_E_ALIGN;
        if (dense) {
            fd[nf] = F[i];
            fd[nf].z_fwd = d.z_fwd; fd[nf].z_mstride = d.z_mstride;
        } else {
            FlowArgs& f = fa[nf];
            f = FlowArgs{};
            f.q0_mean = d.q0_mean; f.q0_log_var = d.q0_log_var; f.rng = rng; f.z_fwd = d.z_fwd; f.zf = d.z_flow; f.rf.T = 0;
            f.I = If; f.want_kl = 0; f.layer = d.layer_id & 63u;
        }
        ScaleLayer& a = bt.l[nf];
        a.e0 = d.e0; a.z = d.z_fwd; a.e_w_members = static_cast<float*>(d.e_w_members); a.z_ms = (long long)d.z_mstride;
        a.O = d.O; a.I = d.I; a.ld = d.ld; a.split = (d.flags & LBBNN_F_SPLIT16) ? 1 : 0;
        if (M) { a.cols = M[i].cols; a.I_full = If; }
        wgs += (d.O + kFzRows - 1) / kFzRows;
        bt.wg_end[nf] = wgs;
        ++nf;
    }
    if (!nf) return 0;
    for (int k = 1; k < nf; ++k) one_stride = one_stride && bt.l[k].z_ms == bt.l[0].z_ms;
    bt.n = nf;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one flow launch serves every layer when they share the member stride of z (a caller lays the layers' z blocks out
    // side by side in one [members][stride] buffer); else one launch per layer (n <= 4), as lbbnn_ensemble_operands
    if (dense) {
        const int rc = lbbnn_flow_dense_members(fd, nf, members, rng, member_advance, stream);   // all layers, one launch
        if (rc) return rc;
    } else if (one_stride) {
        const int rc = launch_flow_planar(fa, nf, s, members, member_advance, bt.l[0].z_ms);
        if (rc) return rc;
    } else {
        for (int k = 0; k < nf; ++k) {
            const int rc = launch_flow_planar(&fa[k], 1, s, members, member_advance, bt.l[k].z_ms);
            if (rc) return rc;
        }
    }
    if (z_only) return 0;
    if (M) hipLaunchKernelGGL(frozen_scale_kernel<true>, dim3(wgs, members), dim3(kFzNT), 0, s, bt);
    else hipLaunchKernelGGL(frozen_scale_kernel<false>, dim3(wgs, members), dim3(kFzNT), 0, s, bt);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int lbbnn_frozen_operands(const lbbnn_frozen_desc_t* L, int n, void* stream) {
    return frozen_operands_impl(L, nullptr, n, stream);
}

extern "C" int lbbnn_frozen_operands_compact(const lbbnn_frozen_desc_t* L, const lbbnn_compact_map_t* M, int n, void* stream) {
    if (!L || !M) return LBBNN_E_NULL;
    return frozen_operands_impl(L, M, n, stream);
}

extern "C" int lbbnn_frozen_members(const lbbnn_frozen_desc_t* L, int n, int members, const uint64_t* rng,
                                    uint64_t member_advance, void* stream) {
    return frozen_members_impl(L, nullptr, false, nullptr, n, members, rng, member_advance, stream);
}

extern "C" int lbbnn_frozen_members_z(const lbbnn_frozen_desc_t* L, int n, int members, const uint64_t* rng,
                                      uint64_t member_advance, void* stream) {
    return frozen_members_impl(L, nullptr, false, nullptr, n, members, rng, member_advance, stream, true);
}

extern "C" int lbbnn_frozen_members_dense(const lbbnn_frozen_desc_t* L, const lbbnn_dense_members_t* F, int n, int members,
                                          const uint64_t* rng, uint64_t member_advance, void* stream) {
    return frozen_members_impl(L, F, true, nullptr, n, members, rng, member_advance, stream);
}

extern "C" int lbbnn_frozen_members_compact(const lbbnn_frozen_desc_t* L, const lbbnn_compact_map_t* M, int n, int members,
                                            const uint64_t* rng, uint64_t member_advance, void* stream) {
    if (!L || !M) return LBBNN_E_NULL;
    return frozen_members_impl(L, nullptr, false, M, n, members, rng, member_advance, stream);
}

extern "C" int lbbnn_gather_columns(const float* x, int ldx, const int32_t* idx, int n_idx, float* out, int ldo, int B,
                                    void* stream) {
    if (B < 0) return LBBNN_E_SHAPE;
    if (B == 0) return 0;
    if (!x || !idx || !out) return LBBNN_E_NULL;
    if (n_idx < 1 || ldo < n_idx || ldx < 1) return LBBNN_E_SHAPE;
    if ((ldo & 3) || !aligned16(out) || !aligned4(x) || !aligned4(idx)) return LBBNN_E_ALIGN;
    const long long items = (long long)B * (ldo >> 2);
    const long long blocks = (items + 255) / 256;
    if (blocks > 0x7FFFFFFFLL) return LBBNN_E_SHAPE;
    hipLaunchKernelGGL(gather_columns_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       x, ldx, idx, n_idx, out, ldo, items);
    return (int)hipGetLastError();
}
