// Compact median-probability model (gfx950): the frozen operands of the units some output depends on, see include/lbbnn.h.
// A compact layer is the full layer's rows `rows` and columns `cols` (sorted index lists built on the host side from the kept
// masks); everything downstream runs the existing GEMMs at the smaller shape.
//
//   compact_operands_kernel -- lbbnn_frozen_operands_compact: frozen_operands_kernel (frozen.hip) with gathered loads.  ONE
//     WAVE PER COMPACT ROW, a lane owns the float4 column groups lane, lane + 64, ... of the COMPACT row: four column indices,
//     then four scalar loads of each of mu / rho / lambdal at (rows[o'], cols[j']); the stores are the 16-B vectors of
//     frozen.hip (fp32, or the bf16 hi | lo units).  Median-probability gates only: a = [lambdal > cut].  The kept count is
//     reduced with DPP moves and stored by lane 0: no atomics, no LDS.  It runs once per freeze.
//   compact_scale_kernel -- lbbnn_frozen_members_compact: e_w_members[m] = operand(E0'[o'][j'] * z_m[cols[j']]), the gather
//     of the full-width z fused into frozen_scale_kernel: no compact z is ever stored.
//   gather_columns_kernel -- lbbnn_gather_columns: out[b][j] = x[b][idx[j]], one thread per float4 of the output.
// The device helpers of frozen.hip (which stays as it is) are restated here, as frozen.hip restates K1's.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"

namespace {

using namespace lbbnn;

constexpr int kFcRows = 4;                 // rows (= waves) per workgroup
constexpr int kFcNT = 64 * kFcRows;
constexpr int kFcB = 2;                    // float4 groups per lane in flight together (12 gathered loads each)

struct CompactLayer {
    const float* mu; const float* rho; const float* lambdal; const float* bias_rho;
    const int32_t* rows; const int32_t* cols;
    float* e0; float* e_w; float* var_w; float* bias_var; int32_t* kept_rows;
    int O, I, ld, O_full, I_full, split;
    float cut;
};
struct CompactBatch { CompactLayer l[LBBNN_MAX_LAYERS]; int wg_end[LBBNN_MAX_LAYERS]; int n; };

struct CScaleLayer {
    const float* e0; const float* z; const int32_t* cols; float* e_w_members;
    long long z_ms;
    int O, I, ld, I_full, split;
};
struct CScaleBatch { CScaleLayer l[LBBNN_MAX_LAYERS]; int wg_end[LBBNN_MAX_LAYERS]; int n; };

// w = hi + lo (both bf16, RNE), four elements as two uint2 -- the split of frozen.hip / K1
typedef __bf16 fc_bf16x2 __attribute__((ext_vector_type(2)));
typedef float fc_floatx2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t fc_cvt_pk(float a, float b) {
    const fc_floatx2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, fc_bf16x2));
}
__device__ __forceinline__ void fc_split4(const float4 w, uint2& hi, uint2& lo) {
    const uint32_t h0 = fc_cvt_pk(w.x, w.y), h1 = fc_cvt_pk(w.z, w.w);
    hi = make_uint2(h0, h1);
    lo = make_uint2(fc_cvt_pk(w.x - __uint_as_float(h0 << 16), w.y - __uint_as_float(h0 & 0xFFFF0000u)),
                    fc_cvt_pk(w.z - __uint_as_float(h1 << 16), w.w - __uint_as_float(h1 & 0xFFFF0000u)));
}
__device__ __forceinline__ uint32_t fc_xor1(uint32_t v) { return (uint32_t)dpp_mov<0xB1>((int)v); }   // lane ^ 1

// One operand group (columns 4j .. 4j+3 of row o) to memory, as fz_store of frozen.hip: EVERY lane of the wave must call
// this (the exchange is a DPP move); `in` says whether the lane's group lies inside the padded row.
__device__ __forceinline__ void fc_store(float* base, int o, int j, int ld, bool split, bool in, const float4 w) {
    if (!split) {
        if (in) reinterpret_cast<float4*>(base + (size_t)o * ld)[j] = w;
        return;
    }
    const bool odd = threadIdx.x & 1;
    uint2 hi, lo;
    fc_split4(w, hi, lo);
    const uint32_t r0 = fc_xor1(odd ? hi.x : lo.x), r1 = fc_xor1(odd ? hi.y : lo.y);
    const uint4 unit = make_uint4(odd ? r0 : hi.x, odd ? r1 : hi.y, odd ? lo.x : r0, odd ? lo.y : r1);
    const size_t at = split_hi_index((size_t)o, 4 * (j & ~1), ld) + (odd ? kSplitLoOffset : 0);
    if (in) *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(base) + at) = unit;
}

template <typename B>
__device__ __forceinline__ int fc_layer_of(const LBBNN_CONST_AS B* bt, int& wg0) {
    int li = 0;
#pragma unroll
    for (int t = 0; t < LBBNN_MAX_LAYERS - 1; ++t) if (t + 1 < bt->n && (int)blockIdx.x >= bt->wg_end[t]) li = t + 1;
    wg0 = li ? bt->wg_end[li - 1] : 0;
    return li;
}

// an index of a map as the kernels use it: inside [0, n) whatever the array holds (the host side builds them in range)
__device__ __forceinline__ int fc_index(const int32_t* idx, int k, int n) {
    const int v = idx[k];
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}

__global__ __launch_bounds__(kFcNT) void compact_operands_kernel(const CompactBatch bt_) {
    const LBBNN_CONST_AS CompactBatch* bt = kernarg_as<CompactBatch>();
    int wg0;
    const int li = fc_layer_of(bt, wg0);
    const LBBNN_CONST_AS CompactLayer& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kFcRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;                                                 // (whole waves leave: no barrier below)
    const int I = a.I, P = a.ld, nq = P >> 2, If = a.I_full;
    const int G = (nq + 63) >> 6;
    const bool split = a.split != 0;
    const float cut = a.cut;
    const int r = fc_index(a.rows, o, a.O_full);
    const size_t rowoff = (size_t)r * If;
    const float* mu_r = a.mu + rowoff; const float* rho_r = a.rho + rowoff; const float* lam_r = a.lambdal + rowoff;
    int kept = 0;
    for (int g0 = 0; g0 < G; g0 += kFcB) {
        float mu[kFcB][4], rho[kFcB][4], lam[kFcB][4];
#pragma unroll
        for (int g = 0; g < kFcB; ++g) {
            const int k = 4 * (lane + 64 * (g0 + g));
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                mu[g][t] = 0.f; rho[g][t] = 0.f; lam[g][t] = 0.f;
                if (k + t < I) {
                    const int c = fc_index(a.cols, k + t, If);
                    mu[g][t] = mu_r[c]; rho[g][t] = rho_r[c]; lam[g][t] = lam_r[c];
                }
            }
        }
#pragma unroll
        for (int g = 0; g < kFcB; ++g) {
            if (g0 + g >= G) break;                                       // wave-uniform
            const int j = lane + 64 * (g0 + g), k = 4 * j;
            float e[4], v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                // a = [lambdal > cut], compared in fp32 (NaN is never kept): e0 = mu or +0.0, V = sigma^2 or 0, as fz_elem
                const bool keep = (k + t < I) && (lam[g][t] > cut);
                const float sigma = k1_sigma(rho[g][t]);
                e[t] = keep ? mu[g][t] : 0.f;
                v[t] = keep ? sigma * sigma : 0.f;
                kept += keep ? 1 : 0;
            }
            const float4 e0 = make_float4(e[0], e[1], e[2], e[3]), vw = make_float4(v[0], v[1], v[2], v[3]);
            const bool in = j < nq;
            if (in) reinterpret_cast<float4*>(a.e0 + (size_t)o * P)[j] = e0;
            fc_store(a.e_w, o, j, P, split, in, e0);
            fc_store(a.var_w, o, j, P, split, in, vw);
        }
    }
    // per-lane counts are < 2^24: their float sum is exact
    const int total = (int)wave_sum((float)kept);
    if (lane == 0) {
        a.kept_rows[o] = total;
        const float sb = softplus_ref(a.bias_rho[r]);
        a.bias_var[o] = sb * sb;                      // bias.sigma**2 of the full row (never gated)
    }
}

__global__ __launch_bounds__(kFcNT) void compact_scale_kernel(const CScaleBatch bt_) {
    const LBBNN_CONST_AS CScaleBatch* bt = kernarg_as<CScaleBatch>();
    int wg0;
    const int li = fc_layer_of(bt, wg0);
    const LBBNN_CONST_AS CScaleLayer& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kFcRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;
    const int mem = blockIdx.y;
    const int P = a.ld, nq = P >> 2, iq = a.I >> 2, If = a.I_full;        // I % 4 == 0 (checked on the host)
    const int G = (nq + 63) >> 6;
    const bool split = a.split != 0;
    const float* z = a.z + (size_t)mem * a.z_ms;
    float* out = a.e_w_members + (size_t)mem * a.O * P;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g0 = 0; g0 < G; g0 += kFcB) {
        float4 e[kFcB], zz[kFcB];
#pragma unroll
        for (int g = 0; g < kFcB; ++g) {
            const int j = lane + 64 * (g0 + g);
            e[g] = zero4; zz[g] = zero4;
            if (j < iq) {
                e[g] = reinterpret_cast<const float4*>(a.e0 + (size_t)o * P)[j];
                zz[g] = make_float4(z[fc_index(a.cols, 4 * j, If)], z[fc_index(a.cols, 4 * j + 1, If)],
                                    z[fc_index(a.cols, 4 * j + 2, If)], z[fc_index(a.cols, 4 * j + 3, If)]);
            }
        }
#pragma unroll
        for (int g = 0; g < kFcB; ++g) {
            if (g0 + g >= G) break;
            const int j = lane + 64 * (g0 + g);
            // (mu * a) * z_k: the mean operand of an MNF layer, the product frozen_scale_kernel forms
            const float4 w = make_float4(e[g].x * zz[g].x, e[g].y * zz[g].y, e[g].z * zz[g].z, e[g].w * zz[g].w);
            fc_store(out, o, j, P, split, j < nq, w);
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
    for (int t = 0; t < 4; ++t) v[t] = (k + t < n_idx) ? row[fc_index(idx, k + t, ldx)] : 0.f;   // zero tail [n_idx, ldo)
    reinterpret_cast<float4*>(out + (size_t)b * ldo)[k >> 2] = make_float4(v[0], v[1], v[2], v[3]);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the checks both compact entry points make of a layer's map
inline int check_map(const lbbnn_compact_map_t& m, int O, int I) {
    if (!m.rows || !m.cols) return LBBNN_E_NULL;
    if (m.O_full <= 0 || m.I_full <= 0 || O > m.O_full || I > m.I_full) return LBBNN_E_SHAPE;
    if (!aligned4(m.rows) || !aligned4(m.cols)) return LBBNN_E_ALIGN;
    return 0;
}

}  // namespace

extern "C" int lbbnn_frozen_operands_compact(const lbbnn_frozen_desc_t* L, const lbbnn_compact_map_t* M, int n, void* stream) {
    if (!L || !M) return LBBNN_E_NULL;
    if (n <= 0 || n > LBBNN_MAX_LAYERS) return LBBNN_E_SHAPE;
    CompactBatch bt = {};
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
        if (d.mode != LBBNN_FROZEN_MPM) return LBBNN_E_FLAGS;  // alpha gates are never exactly zero: nothing to drop
        const int rc = check_map(M[i], d.O, d.I);
        if (rc) return rc;
        if ((d.flags & LBBNN_F_SPLIT16) && (d.I & 7)) return LBBNN_E_ALIGN;   // the bf16 hi | lo kernels' rule (I % 8)
        CompactLayer& a = bt.l[i];
        a.mu = d.weight_mu; a.rho = d.weight_rho; a.lambdal = d.lambdal; a.bias_rho = d.bias_rho;
        a.rows = M[i].rows; a.cols = M[i].cols;
        a.e0 = d.e0; a.e_w = static_cast<float*>(d.e_w); a.var_w = static_cast<float*>(d.var_w);
        a.bias_var = d.bias_var; a.kept_rows = d.kept_rows;
        a.O = d.O; a.I = d.I; a.ld = d.ld; a.O_full = M[i].O_full; a.I_full = M[i].I_full; a.cut = d.cut;
        a.split = (d.flags & LBBNN_F_SPLIT16) ? 1 : 0;
        wgs += (d.O + kFcRows - 1) / kFcRows;
        bt.wg_end[i] = wgs;
    }
    bt.n = n;
    hipLaunchKernelGGL(compact_operands_kernel, dim3(wgs), dim3(kFcNT), 0, static_cast<hipStream_t>(stream), bt);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_frozen_members_compact(const lbbnn_frozen_desc_t* L, const lbbnn_compact_map_t* M, int n, int members,
                                            const uint64_t* rng, uint64_t member_advance, void* stream) {
    if (!L || !M) return LBBNN_E_NULL;
    if (n <= 0 || n > LBBNN_MAX_LAYERS || members < 1 || members > 65535) return LBBNN_E_SHAPE;
    FlowArgs fa[LBBNN_MAX_LAYERS];
    CScaleBatch bt = {};
    int nf = 0, wgs = 0;
    bool one_stride = true;
    for (int i = 0; i < n; ++i) {
        const lbbnn_frozen_desc_t& d = L[i];
        if (!d.q0_mean) continue;                           // an LRT layer: its e_w is shared by every member
        if (!d.q0_log_var || !d.z_fwd || !d.e0 || !d.e_w_members) return LBBNN_E_NULL;
        if (d.z_flow.T < 0 || d.z_flow.T > LBBNN_MAX_FLOW_T) return LBBNN_E_SHAPE;
        for (int t = 0; t < d.z_flow.T; ++t)
            if (!d.z_flow.u[t] || !d.z_flow.w[t] || !d.z_flow.b[t]) return LBBNN_E_NULL;
        if (!rng) return LBBNN_E_NOISE;
        if (d.O <= 0 || d.I <= 0 || d.ld < d.I) return LBBNN_E_SHAPE;
        const int rc = check_map(M[i], d.O, d.I);
        if (rc) return rc;
        const int If = M[i].I_full;                         // the flow runs, and z lies, at the FULL width
        if (If > LBBNN_MAX_FLOW_DIM || d.z_mstride < If) return LBBNN_E_SHAPE;
        if ((d.ld & 31) || (d.I & 3) || (If & 3) || (d.z_mstride & 3)) return LBBNN_E_ALIGN;
        if (!aligned16(d.e0) || !aligned16(d.e_w_members) || !aligned16(d.z_fwd)) return LBBNN_E_ALIGN;
        if (d.flags & ~LBBNN_F_SPLIT16) return LBBNN_E_FLAGS;
        if ((d.flags & LBBNN_F_SPLIT16) && (d.I & 7)) return LBBNN_E_ALIGN;
        FlowArgs& f = fa[nf];
        f = FlowArgs{};
        f.q0_mean = d.q0_mean; f.q0_log_var = d.q0_log_var; f.rng = rng; f.z_fwd = d.z_fwd; f.zf = d.z_flow; f.rf.T = 0;
        f.I = If; f.want_kl = 0; f.layer = d.layer_id & 63u;
        CScaleLayer& a = bt.l[nf];
        a.e0 = d.e0; a.z = d.z_fwd; a.cols = M[i].cols; a.e_w_members = static_cast<float*>(d.e_w_members);
        a.z_ms = (long long)d.z_mstride;
        a.O = d.O; a.I = d.I; a.ld = d.ld; a.I_full = If; a.split = (d.flags & LBBNN_F_SPLIT16) ? 1 : 0;
        wgs += (d.O + kFcRows - 1) / kFcRows;
        bt.wg_end[nf] = wgs;
        ++nf;
    }
    if (!nf) return 0;
    for (int k = 1; k < nf; ++k) one_stride = one_stride && bt.l[k].z_ms == bt.l[0].z_ms;
    bt.n = nf;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the flow launch of lbbnn_frozen_members, at the full width: member m's z is the full model's, bit for bit
    if (one_stride) {
        const int rc = launch_flow_planar(fa, nf, s, members, member_advance, bt.l[0].z_ms);
        if (rc) return rc;
    } else {
        for (int k = 0; k < nf; ++k) {
            const int rc = launch_flow_planar(&fa[k], 1, s, members, member_advance, bt.l[k].z_ms);
            if (rc) return rc;
        }
    }
    hipLaunchKernelGGL(compact_scale_kernel, dim3(wgs, members), dim3(kFcNT), 0, s, bt);
    return (int)hipGetLastError();
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
