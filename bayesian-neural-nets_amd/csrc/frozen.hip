// Frozen evaluation model (gfx950): the GEMM operands of a trained LRT / MNF network taken ONCE from its parameters, with
// the gates as trained (alpha) or thresholded (the median probability model), see include/lbbnn.h.
//
//   frozen_operands_kernel -- lbbnn_frozen_operands: one launch over the rows of up to LBBNN_MAX_LAYERS layers.  ONE WAVE
//     PER ROW (four rows per 256-thread workgroup): a lane owns the float4 column groups lane, lane + 64, ...; a wave-load
//     covers 1 KiB contiguous of each of mu / rho / lambdal, kFzB groups per lane in flight together.  Per weight 12 B
//     read, 12 B (fp32: e0, e_w, var_w) or 12 B (split: e0 4 B + two hi | lo operands of 4 B each) written -- a streaming
//     kernel whose bound is HBM.  The arithmetic of mode 0 is K1's (k1_alpha / k1_sigma of lbbnn_device.h, the products in
//     K1's order), so the operands are the values lbbnn_weight_pass writes.  The kept count of a row is accumulated per
//     lane, reduced with DPP moves (wave_sum) and stored by lane 0 with an ordinary store: no atomics.
//     Rows that are not whole aligned float4s (I % 4 != 0, or parameters off a 16-B boundary) take scalar loads of the
//     same groups; the stores are 16-B vectors into the padded rows either way (fp32 operands only there, as K1).
//   frozen_scale_kernel -- lbbnn_frozen_members: e_w_members[m] = operand(E0 * z_m) for every member (gridDim.y) and MNF
//     layer in one launch: 4 B read (e0, L2-resident across members) and 4 B written per weight and member.
//     lbbnn_frozen_members_dense is the same launch behind lbbnn_flow_dense_members (flow_dense_members.hip) instead of the
//     planar-flow launch: the z of RNVP / MNF-type z flows.
#include <cstdlib>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"

namespace {

using namespace lbbnn;

constexpr int kFzRows = 4;                 // rows (= waves) per workgroup
constexpr int kFzNT = 64 * kFzRows;
constexpr int kFzB = 4;                    // float4 groups per lane loaded together: 1024 weights of a row per batch

struct FrozenLayer {
    const float* mu; const float* rho; const float* lambdal; const float* bias_rho;
    float* e0; float* e_w; float* var_w; float* bias_var; int32_t* kept_rows;
    int O, I, ld, vec, split, mode;
    float cut;
};
struct FrozenBatch { FrozenLayer l[LBBNN_MAX_LAYERS]; int wg_end[LBBNN_MAX_LAYERS]; int n; };

struct ScaleLayer {
    const float* e0; const float* z; float* e_w_members;
    long long z_ms;
    int O, I, ld, split;
};
struct ScaleBatch { ScaleLayer l[LBBNN_MAX_LAYERS]; int wg_end[LBBNN_MAX_LAYERS]; int n; };

// w = hi + lo (both bf16, v_cvt_pk_bf16_f32: RNE), four elements as two uint2 -- the split of K1 (weight_pass.hip)
typedef __bf16 fz_bf16x2 __attribute__((ext_vector_type(2)));
typedef float fz_floatx2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t fz_cvt_pk(float a, float b) {
    const fz_floatx2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, fz_bf16x2));
}
__device__ __forceinline__ void fz_split4(const float4 w, uint2& hi, uint2& lo) {
    const uint32_t h0 = fz_cvt_pk(w.x, w.y), h1 = fz_cvt_pk(w.z, w.w);
    hi = make_uint2(h0, h1);
    lo = make_uint2(fz_cvt_pk(w.x - __uint_as_float(h0 << 16), w.y - __uint_as_float(h0 & 0xFFFF0000u)),
                    fz_cvt_pk(w.z - __uint_as_float(h1 << 16), w.w - __uint_as_float(h1 & 0xFFFF0000u)));
}
__device__ __forceinline__ uint32_t fz_xor1(uint32_t v) { return (uint32_t)dpp_mov<0xB1>((int)v); }   // lane ^ 1

// One operand group (columns 4j .. 4j+3 of row o) to memory.  fp32: the float4 itself.  Split: 16-B units (lbbnn_device.h) --
// the even lane of a pair holds k = 8m..8m+3, the odd lane k = 8m+4..8m+7; the even lane stores the hi unit (its hi half |
// the partner's), the odd lane the lo unit next to it.  EVERY lane of the wave must call this (the exchange is a DPP move);
// `in` says whether the lane's group lies inside the padded row (ld / 4 is a multiple of 8: both lanes of a pair agree).
__device__ __forceinline__ void fz_store(float* base, int o, int j, int ld, bool split, bool in, const float4 w) {
    if (!split) {
        if (in) reinterpret_cast<float4*>(base + (size_t)o * ld)[j] = w;
        return;
    }
    const bool odd = threadIdx.x & 1;
    uint2 hi, lo;
    fz_split4(w, hi, lo);
    const uint32_t r0 = fz_xor1(odd ? hi.x : lo.x), r1 = fz_xor1(odd ? hi.y : lo.y);
    const uint4 unit = make_uint4(odd ? r0 : hi.x, odd ? r1 : hi.y, odd ? lo.x : r0, odd ? lo.y : r1);
    const size_t at = split_hi_index((size_t)o, 4 * (j & ~1), ld) + (odd ? kSplitLoOffset : 0);
    if (in) *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(base) + at) = unit;
}

// the layer of this workgroup from the prefix ends of the layers' workgroup ranges
template <typename B>
__device__ __forceinline__ int fz_layer_of(const LBBNN_CONST_AS B* bt, int& wg0) {
    int li = 0;
#pragma unroll
    for (int t = 0; t < LBBNN_MAX_LAYERS - 1; ++t) if (t + 1 < bt->n && (int)blockIdx.x >= bt->wg_end[t]) li = t + 1;
    wg0 = li ? bt->wg_end[li - 1] : 0;
    return li;
}

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

struct FzElem { float e0, v; int kept; };
// mode 0: a = alpha (K1's operands: e_w = mu * alpha, var_w = sigma^2 * alpha^2, LBBNN-GP-MF-LRT.py:170-171);
// mode 1: a = [lambdal > cut] (outofsample(medimod=True)): e0 = mu or 0, V = sigma^2 or 0 (a^2 = a)
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

__global__ __launch_bounds__(kFzNT) void frozen_operands_kernel(const FrozenBatch bt_) {
    const LBBNN_CONST_AS FrozenBatch* bt = kernarg_as<FrozenBatch>();
    int wg0;
    const int li = fz_layer_of(bt, wg0);
    const LBBNN_CONST_AS FrozenLayer& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kFzRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;                                                 // (whole waves leave: no barrier below)
    const int I = a.I, P = a.ld, nq = P >> 2;
    const int iq = (I + 3) >> 2;                                          // groups holding at least one weight
    const int G = (nq + 63) >> 6;
    const bool vec = a.vec != 0, split = a.split != 0;
    const int mode = a.mode;
    const float cut = a.cut;
    const size_t rowoff = (size_t)o * I;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int kept = 0;
    for (int g0 = 0; g0 < G; g0 += kFzB) {
        float4 mu[kFzB], rho[kFzB], lam[kFzB];
#pragma unroll
        for (int g = 0; g < kFzB; ++g) {
            const int j = lane + 64 * (g0 + g);
            mu[g] = zero4; rho[g] = zero4; lam[g] = zero4;
            if (j < iq) {
                if (vec) { mu[g] = fz_ld4(a.mu + rowoff, j); rho[g] = fz_ld4(a.rho + rowoff, j); lam[g] = fz_ld4(a.lambdal + rowoff, j); }
                else {
                    mu[g] = fz_ld4_scalar(a.mu + rowoff, j, I); rho[g] = fz_ld4_scalar(a.rho + rowoff, j, I);
                    lam[g] = fz_ld4_scalar(a.lambdal + rowoff, j, I);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < kFzB; ++g) {
            if (g0 + g >= G) break;                                       // wave-uniform
            const int j = lane + 64 * (g0 + g);
            float4 e0 = zero4, vw = zero4;
            if (j < iq) {
                const FzElem x = fz_elem(mu[g].x, rho[g].x, lam[g].x, mode, cut), y = fz_elem(mu[g].y, rho[g].y, lam[g].y, mode, cut);
                const FzElem z = fz_elem(mu[g].z, rho[g].z, lam[g].z, mode, cut), w = fz_elem(mu[g].w, rho[g].w, lam[g].w, mode, cut);
                const int k = 4 * j;                                      // the zero tail of a partial group (I % 4 != 0)
                const bool ky = k + 1 < I, kz = k + 2 < I, kw = k + 3 < I;
                e0 = make_float4(x.e0, ky ? y.e0 : 0.f, kz ? z.e0 : 0.f, kw ? w.e0 : 0.f);
                vw = make_float4(x.v, ky ? y.v : 0.f, kz ? z.v : 0.f, kw ? w.v : 0.f);
                kept += x.kept + (ky ? y.kept : 0) + (kz ? z.kept : 0) + (kw ? w.kept : 0);
            }
            const bool in = j < nq;
            if (in) reinterpret_cast<float4*>(a.e0 + (size_t)o * P)[j] = e0;
            fz_store(a.e_w, o, j, P, split, in, e0);
            fz_store(a.var_w, o, j, P, split, in, vw);
        }
    }
    // per-lane counts are < 2^24: their float sum is exact
    const int total = (int)wave_sum((float)kept);
    if (lane == 0) {
        a.kept_rows[o] = total;
        const float sb = softplus_ref(a.bias_rho[o]);
        a.bias_var[o] = sb * sb;                      // bias.sigma**2, LBBNN-GP-MF-LRT.py:173 (never gated)
    }
}

__global__ __launch_bounds__(kFzNT) void frozen_scale_kernel(const ScaleBatch bt_) {
    const LBBNN_CONST_AS ScaleBatch* bt = kernarg_as<ScaleBatch>();
    int wg0;
    const int li = fz_layer_of(bt, wg0);
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
    for (int g0 = 0; g0 < G; g0 += kFzB) {
        float4 e[kFzB], zz[kFzB];
#pragma unroll
        for (int g = 0; g < kFzB; ++g) {
            const int j = lane + 64 * (g0 + g);
            e[g] = zero4; zz[g] = zero4;
            if (j < iq) { e[g] = fz_ld4(a.e0 + (size_t)o * P, j); zz[g] = fz_ld4(z, j); }
        }
#pragma unroll
        for (int g = 0; g < kFzB; ++g) {
            if (g0 + g >= G) break;
            const int j = lane + 64 * (g0 + g);
            // (mu * a) * z_k: the mean operand of an MNF layer (LBBNN-GP-MF-MNF.py:195,197), K1's order of products
            const float4 w = make_float4(e[g].x * zz[g].x, e[g].y * zz[g].y, e[g].z * zz[g].z, e[g].w * zz[g].w);
            fz_store(out, o, j, P, split, j < nq, w);
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int lbbnn_frozen_operands(const lbbnn_frozen_desc_t* L, int n, void* stream) {
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
        if ((reinterpret_cast<uintptr_t>(d.weight_mu) | reinterpret_cast<uintptr_t>(d.weight_rho) |
             reinterpret_cast<uintptr_t>(d.lambdal) | reinterpret_cast<uintptr_t>(d.bias_rho) |
             reinterpret_cast<uintptr_t>(d.bias_var) | reinterpret_cast<uintptr_t>(d.kept_rows)) & 3u) return LBBNN_E_ALIGN;
        if (d.flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
        if (d.mode != LBBNN_FROZEN_ALPHA && d.mode != LBBNN_FROZEN_MPM) return LBBNN_E_FLAGS;
        FrozenLayer& a = bt.l[i];
        a.mu = d.weight_mu; a.rho = d.weight_rho; a.lambdal = d.lambdal; a.bias_rho = d.bias_rho;
        a.e0 = d.e0; a.e_w = static_cast<float*>(d.e_w); a.var_w = static_cast<float*>(d.var_w);
        a.bias_var = d.bias_var; a.kept_rows = d.kept_rows;
        a.O = d.O; a.I = d.I; a.ld = d.ld; a.mode = d.mode; a.cut = d.cut;
        a.split = (d.flags & LBBNN_F_SPLIT16) ? 1 : 0;
        a.vec = (d.I % 4 == 0 && aligned16(d.weight_mu) && aligned16(d.weight_rho) && aligned16(d.lambdal)) ? 1 : 0;
        if (a.split && !a.vec) return LBBNN_E_ALIGN;        // split operands need whole aligned float4 rows, as K1
        wgs += (d.O + kFzRows - 1) / kFzRows;
        bt.wg_end[i] = wgs;
    }
    bt.n = n;
    hipLaunchKernelGGL(frozen_operands_kernel, dim3(wgs), dim3(kFzNT), 0, static_cast<hipStream_t>(stream), bt);
    return (int)hipGetLastError();
}

// the per-member part of a frozen model: the z flows of the MNF layers (planar: d.z_flow; dense: F, lbbnn_flow_dense_members),
// then frozen_scale_kernel
static int frozen_members_impl(const lbbnn_frozen_desc_t* L, const lbbnn_dense_members_t* F, bool dense, int n, int members,
                               const uint64_t* rng, uint64_t member_advance, void* stream) {
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
        if (!d.q0_log_var || !d.z_fwd || !d.e0 || !d.e_w_members) return LBBNN_E_NULL;
        if (!dense) {
            if (d.z_flow.T < 0 || d.z_flow.T > LBBNN_MAX_FLOW_T) return LBBNN_E_SHAPE;
            for (int t = 0; t < d.z_flow.T; ++t)
                if (!d.z_flow.u[t] || !d.z_flow.w[t] || !d.z_flow.b[t]) return LBBNN_E_NULL;
        }
        if (!rng) return LBBNN_E_NOISE;
        if (d.O <= 0 || d.I <= 0 || d.ld < d.I || d.I > LBBNN_MAX_FLOW_DIM) return LBBNN_E_SHAPE;
        if (d.z_mstride < d.I) return LBBNN_E_SHAPE;
        if ((d.ld & 31) || (d.I & 3) || (d.z_mstride & 3)) return LBBNN_E_ALIGN;
        if (!aligned16(d.e0) || !aligned16(d.e_w_members) || !aligned16(d.z_fwd)) return LBBNN_E_ALIGN;
        if (d.flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
        if (dense) {
            fd[nf] = F[i];
            fd[nf].z_fwd = d.z_fwd; fd[nf].z_mstride = d.z_mstride;
        } else {
            FlowArgs& f = fa[nf];
            f = FlowArgs{};
            f.q0_mean = d.q0_mean; f.q0_log_var = d.q0_log_var; f.rng = rng; f.z_fwd = d.z_fwd; f.zf = d.z_flow; f.rf.T = 0;
            f.I = d.I; f.want_kl = 0; f.layer = d.layer_id & 63u;
        }
        ScaleLayer& a = bt.l[nf];
        a.e0 = d.e0; a.z = d.z_fwd; a.e_w_members = static_cast<float*>(d.e_w_members); a.z_ms = (long long)d.z_mstride;
        a.O = d.O; a.I = d.I; a.ld = d.ld; a.split = (d.flags & LBBNN_F_SPLIT16) ? 1 : 0;
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
    hipLaunchKernelGGL(frozen_scale_kernel, dim3(wgs, members), dim3(kFzNT), 0, s, bt);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_frozen_members(const lbbnn_frozen_desc_t* L, int n, int members, const uint64_t* rng,
                                    uint64_t member_advance, void* stream) {
    return frozen_members_impl(L, nullptr, false, n, members, rng, member_advance, stream);
}

extern "C" int lbbnn_frozen_members_dense(const lbbnn_frozen_desc_t* L, const lbbnn_dense_members_t* F, int n, int members,
                                          const uint64_t* rng, uint64_t member_advance, void* stream) {
    return frozen_members_impl(L, F, true, n, members, rng, member_advance, stream);
}
