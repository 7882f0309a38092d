// K2'' -- the two activation-moment GEMMs of the local-reparameterisation layer on the FP16 matrix cores of gfx950
// (v_mfma_f32_16x16x32_f16, fp32 accumulate) with ROW-SCALED hi + lo operands: the LBBNN_F_F16S format of include/lbbnn.h.
//
//   mean[b,o] = sum_k x[b,k]   * e_w[o,k]   + bias_mean[o]                   (torch.mm, LBBNN-GP-MF-LRT.py:172; ...MNF.py:197)
//   var [b,o] = sum_k x[b,k]^2 * var_w[o,k] (*var_scale[o]) + bias_var[o]    (...LRT.py:173; ...MNF.py:198)
//   out [b,o] = mean + sqrt(var) * eps[b,o]  (+ReLU)                         (...LRT.py:174-175; ...MNF.py:199-200)
//
// Why this format (round 3).  The bf16x3 kernel (lrt_gemm.hip) is co-limited by the matrix pipe and by the
// VALU port: ~112 conversion instructions per wave and K step (x and x^2 split into bf16 hi / lo in registers) beside 60
// MFMAs that hold the same issue port for 8 of their 16 cycles.  Here
//   * x arrives ALREADY split -- fp16 hi | lo units in the same 128-B line layout as the weights (LBBNN_F_XPLANES), written
//     by the previous layer's epilogue or by lbbnn_format_x: no split in the consumer at all; x^2 is formed from the planes by
//     four packed-fp16 instructions per 2 k (a = xh 2^-4, b = xl 2^-3, s = fma(a, a, a b));
//   * the variance GEMM takes ONE product (LBBNN_F_VAR1: sh.vh; 4 MFMAs per tile step instead of 6, 15 fragment reads instead
//     of 20) or the full three (sh.vh + sh.vl + sl.vh);
//   * fp16 carries 11 significand bits per part against bf16's 8: hi + lo represent an fp32 value to 2^-22, the 3-product
//     mean to ~3e-8 of max|out| (bf16x3: 2.7e-6), so the 3 + 3 form is tighter than an fp32-accumulate torch.mm and the 3 + 1
//     form sits at 1.4-1.8e-5 (tools/format_error.py; contract 1e-4).
// fp16's 5 exponent bits are handled by exact power-of-two scales: one per weight row and operand (mean_scale / wvar_scale,
// taken out again in the epilogue) and the fixed 2^-8 on x^2.  |x| >= 4096 makes x^2 2^-8 overflow to +inf: the output of
// such a row is non-finite, never silently saturated (tests/test_f16_gemm.py::test_range_overflow_is_loud).
//
// Tile, LDS image, LDS-DMA pieces, swizzle, XCD tile ownership, schedule: those of lrt_gemm_bf16x3_body (lrt_gemm.hip) --
// 80(o) x 128(b) per 4-wave workgroup, two workgroups per CU, K step 32, one 128-B line per row and step in every region,
// 1-KiB pieces of 8 rows, slot s of row r stored at s ^ G(r & 15).
#include <cstdlib>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "kl_piggy.h"
#include "gemm_common.h"
#include "../../include/lbbnn.h"

namespace {

using namespace lbbnn;
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int BKS = 32;
constexpr float kS2 = 0.00390625f;          // 2^-8: the fixed scale of the x^2 planes
constexpr float kS2inv = 256.f;

__device__ __forceinline__ int swzx(int r) { return (((r >> 1) & 3) << 1) | ((r >> 3) & 1); }
// 64-B rows (the hi-only var_w region of the 3 + 1 form): slot s of row r is stored at s ^ F[(r >> 2) & 3], F = {0, 2, 3, 1} --
// the conflict-free map of the fp32 LDS-DMA kernel (lrt_gemm.hip), whose image has the same shape (16 rows x 64 B per piece)
__device__ __forceinline__ int swz4(int rowgrp) { return (0x78 >> (2 * (rowgrp & 3))) & 3; }

struct G16Args {
    const char* x; const char* e_w; const char* var_w;
    const float* mean_scale; const float* wvar_scale;
    const float* bias_mean; const float* bias_var; const float* var_scale;
    const float* eps; const uint64_t* rng;
    float* out; char* out_planes; float* std_out;
    long long row_offset;
    int ldx, ld, ldo, ldp, B, I, O;
    uint32_t rng_stream;
    int relu;
    // head fold (lbbnn_gemm_desc_t::head_*): h_slab != NULL => the epilogue also contracts this tile's 80 output features
    // with the <= 16 rows of the NEXT layer's fp32 operands and writes partial moments to h_slab[o tile][b][2][16]
    const float* h_e; const float* h_v; float* h_slab;
    int h_ld, h_C;
    // the tile grid (launch16): grid.x x grid.y without the finalize row, so that a workgroup finds its tile -- and whether
    // it is the finalize row, which exists only behind the tiles -- from this one fetch, not from the dispatch packet
    int gx, gy;
    FinalizePiggy fin;
};

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
constexpr float kHeadES = 256.f, kHeadVS = 16384.f;       // fixed power-of-two scales of the head's e_w / var_w fp16 parts

__device__ __forceinline__ uint32_t cvt_pk_h(float a, float b) {
    const floatx2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}
__device__ __forceinline__ float h_lo(uint32_t p) { return (float)__builtin_bit_cast(f16x2, p)[0]; }
__device__ __forceinline__ float h_hi(uint32_t p) { return (float)__builtin_bit_cast(f16x2, p)[1]; }

// The epilogue's operands, staged ONCE per workgroup in the K-step buffer that is idle during the last step (it was consumed
// in step nsteps - 2; with one step the second buffer is never used at all) -- every wave used to fetch all of them itself,
// 16 lanes per address: 25 (35 with the head fold) 1-KiB wave loads at the head of a VALU-bound epilogue, and their values
// held 80 (120) registers through it.  Image, BN = 16 TO features:
//   float bm[BN] | bv[BN] | vs[BN] | ms[BN]      per-feature constants, vs = (wvar_scale 2^8) var_scale; fills 0, 0, 1, 1
//   uint4 he[TO][64]                             head fold: (ehd | eld) of lane (class lr, quad q) of tile row i at [i][16 q + lr]
//   uint4 hv[TO][64]                             (vhd | vld), vld = 0 with one variance product
// The loop's closing s_waitcnt + barrier publishes the image; the epilogue reads one float4 per array and tile row.
template <int TO>
struct EpiImage {
    static constexpr int BN = TO * 16;
    static constexpr int kConst = 0, kHeadE = 4 * BN * 4, kHeadV = kHeadE + TO * 64 * 16, kBytes = kHeadV + TO * 64 * 16;
};

// The epilogue and its staging read their arguments from the kernarg segment where they use them (scalar loads): fetched with
// the by-value struct at kernel entry, the twenty epilogue-only fields stay in SGPRs through the K loop, and the spills that
// follow take the kernel's scratch allocation with them.
typedef const LBBNN_CONST_AS G16Args KArgs;

// Values a thread carries from stage_load to stage_store: the image is written behind the last step's MFMAs, loads first.
template <int NQ>
struct EpiStage { float c[5]; float4 he[NQ], hv[NQ]; };

// One float per thread and array: any alignment, any O tail, a null pointer -> the fill value.
__device__ __forceinline__ float ld1f(const float* p, int o, bool in, float fill) { return (p && in) ? p[o] : fill; }

template <int TO, int WB>
__device__ __forceinline__ void stage_load(const KArgs& a, int o0, int tid, EpiStage<(TO + WB - 1) / WB>& st) {
    constexpr int BN = TO * 16, NQ = (TO + WB - 1) / WB;
    static_assert(WB * 64 >= BN, "one thread per feature");
    if (tid < BN) {
        const int o = o0 + tid;
        const bool in = o < a.O;
        st.c[0] = ld1f(a.bias_mean, o, in, 0.f);
        st.c[1] = ld1f(a.bias_var, o, in, 0.f);
        st.c[2] = ld1f(a.var_scale, o, in, 1.f);
        st.c[3] = ld1f(a.mean_scale, o, in, 1.f);
        st.c[4] = ld1f(a.wvar_scale, o, in, 1.f);
    }
    if (a.h_slab) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int s = tid + u * WB * 64;                      // slot [i][16 q + lr]
            const int o = o0 + (s >> 6) * 16 + 4 * ((s >> 4) & 3), cls = s & 15;
            st.he[u] = make_float4(0.f, 0.f, 0.f, 0.f); st.hv[u] = st.he[u];
            if (s < TO * 64 && cls < a.h_C && o < a.O) {
                st.he[u] = *reinterpret_cast<const float4*>(a.h_e + (size_t)cls * a.h_ld + o);
                st.hv[u] = *reinterpret_cast<const float4*>(a.h_v + (size_t)cls * a.h_ld + o);
            }
        }
    }
}

template <int TO, int WB, int NPV>
__device__ __forceinline__ void stage_store(const KArgs& a, int tid, const EpiStage<(TO + WB - 1) / WB>& st, char* img) {
    constexpr int BN = TO * 16, NQ = (TO + WB - 1) / WB;
    typedef EpiImage<TO> IM;
    if (tid < BN) {
        float* c = reinterpret_cast<float*>(img + IM::kConst);
        c[tid] = st.c[0];
        c[BN + tid] = st.c[1];
        c[2 * BN + tid] = (st.c[4] * kS2inv) * st.c[2];           // exact powers of two first
        c[3 * BN + tid] = st.c[3];
    }
    if (a.h_slab) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int s = tid + u * WB * 64;
            if (s >= TO * 64) continue;
            const float4 e4 = st.he[u], v4 = st.hv[u];
            const uint32_t eh0 = cvt_pk_h(e4.x * kHeadES, e4.y * kHeadES), eh1 = cvt_pk_h(e4.z * kHeadES, e4.w * kHeadES);
            const uint32_t el0 = cvt_pk_h(e4.x * kHeadES - h_lo(eh0), e4.y * kHeadES - h_hi(eh0));
            const uint32_t el1 = cvt_pk_h(e4.z * kHeadES - h_lo(eh1), e4.w * kHeadES - h_hi(eh1));
            const uint32_t vh0 = cvt_pk_h(v4.x * kHeadVS, v4.y * kHeadVS), vh1 = cvt_pk_h(v4.z * kHeadVS, v4.w * kHeadVS);
            uint32_t vl0 = 0, vl1 = 0;
            if (NPV == 3) {
                vl0 = cvt_pk_h(v4.x * kHeadVS - h_lo(vh0), v4.y * kHeadVS - h_hi(vh0));
                vl1 = cvt_pk_h(v4.z * kHeadVS - h_lo(vh1), v4.w * kHeadVS - h_hi(vh1));
            }
            reinterpret_cast<uint4*>(img + IM::kHeadE)[s] = make_uint4(eh0, eh1, el0, el1);
            reinterpret_cast<uint4*>(img + IM::kHeadV)[s] = make_uint4(vh0, vh1, vl0, vl1);
        }
    }
}

// Epilogue of a wave's TO x TB accumulator tiles (lane: out[b][o .. o+3] of tile (i, j), o = o0 + 16 i + 4 q, b = brow0 + 16 j).
// Phase 1: the explicit eps loads back to back.  Phase 2 per tile row: the row's constants (and head fragments) from the
//   staged image `img` (EpiImage), then per tile: noise, arithmetic, stores --
//   fp32 `out` (float4 per lane), sqrt(var) for the backward pass, and the fp16 hi | lo PLANES of the next layer's x: the
//   lane pair (q, q ^ 1) holds the 8 consecutive k of one 16-B unit pair, v_permlane16_swap_b32 moves the halves so that
//   the even lane stores the hi unit and the odd lane the lo unit (16 B each, 64 B contiguous per row and tile).
//   Noise: tile t = i TB + j < NPRE was drawn by the caller ahead of the K loop (`pre`, zeros where the tile is not live);
//   the others are drawn here -- counter-based Philox gives the same bits wherever it runs.
//   Head fold (a.h_slab): the NEXT layer is a <= 16-class head (LBBNN-GP-MF-MNF.py:256: l3 on relu(l2)).  Its two moment
//   products over THIS workgroup's 80 features are formed here, on the matrix cores: the accumulator layout of a 16 x 16
//   tile (lane (b, q): features 4q..4q+3 of row b) IS the B-operand layout of v_mfma_f32_16x16x16_f16 (k = 4q + r), the A
//   operand is the head's weight tile (lane (class, q)), both as fp16 hi + lo with 3 + 1 (3) products like the main loop.
//   Each wave owns its 32 rows, so nothing is reduced across waves: per o tile a slab row of 2 x 16 floats per batch row;
//   head_finalize_kernel adds the slabs in o-tile order.  Saves the h2 store + re-read and the head's own launch.
template <int TO, int TB, int NPV, int NPRE>
__device__ __forceinline__ void epilogue16(const KArgs& a, int o0, int q, int lr, int brow0, const char* img,
                                           uint64_t seed, uint64_t offs, const float (&pre)[NPRE > 0 ? NPRE : 1][4],
                                           const floatx4 (&accm)[TO][TB], const floatx4 (&accv)[TO][TB]) {
    typedef EpiImage<TO> IM;
    constexpr int BN = TO * 16;
    const bool ovec = ((a.O & 3) == 0) && (!a.out || (((a.ldo & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.out) & 15u) == 0))) &&
                      (!a.eps || (reinterpret_cast<uintptr_t>(a.eps) & 15u) == 0) &&
                      (!a.std_out || (reinterpret_cast<uintptr_t>(a.std_out) & 15u) == 0);
    float pe[TO][TB][4];
    if (a.eps) {
#pragma unroll
        for (int i = 0; i < TO; ++i) {
            const int o = o0 + i * 16 + 4 * q;
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                const int b = brow0 + j * 16;
                if (o >= a.O || b >= a.B) continue;
                const float* p = a.eps + (size_t)b * a.O + o;
                if (ovec) { const float4 t = *reinterpret_cast<const float4*>(p); pe[i][j][0] = t.x; pe[i][j][1] = t.y; pe[i][j][2] = t.z; pe[i][j][3] = t.w; }
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pe[i][j][r] = (o + r < a.O) ? p[r] : 0.f;
                }
            }
        }
    }
    const bool head = a.h_slab != nullptr;
    const float* cst = reinterpret_cast<const float*>(img + IM::kConst);
    __builtin_amdgcn_sched_barrier(0);
    const bool odd = q & 1;
    floatx4 hm[TB], hv[TB];
#pragma unroll
    for (int j = 0; j < TB; ++j) { hm[j] = floatx4{0.f, 0.f, 0.f, 0.f}; hv[j] = floatx4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int i = 0; i < TO; ++i) {
        const int o = o0 + i * 16 + 4 * q;
        const bool oin = o < a.O;
        const int fo = i * 16 + 4 * q;
        const float4 bm = *reinterpret_cast<const float4*>(cst + fo), bv = *reinterpret_cast<const float4*>(cst + BN + fo);
        const float4 vs = *reinterpret_cast<const float4*>(cst + 2 * BN + fo), ms = *reinterpret_cast<const float4*>(cst + 3 * BN + fo);
        const float c_bm[4] = {bm.x, bm.y, bm.z, bm.w}, c_bv[4] = {bv.x, bv.y, bv.z, bv.w};
        const float c_vs[4] = {vs.x, vs.y, vs.z, vs.w}, c_ms[4] = {ms.x, ms.y, ms.z, ms.w};
        f16x4 ehd = {0, 0, 0, 0}, eld = {0, 0, 0, 0}, vhd = {0, 0, 0, 0}, vld = {0, 0, 0, 0};
        if (head) {
            const uint4 ea = reinterpret_cast<const uint4*>(img + IM::kHeadE)[i * 64 + 16 * q + lr];
            const uint4 va = reinterpret_cast<const uint4*>(img + IM::kHeadV)[i * 64 + 16 * q + lr];
            ehd = __builtin_bit_cast(f16x4, make_uint2(ea.x, ea.y)); eld = __builtin_bit_cast(f16x4, make_uint2(ea.z, ea.w));
            vhd = __builtin_bit_cast(f16x4, make_uint2(va.x, va.y));
            if (NPV == 3) vld = __builtin_bit_cast(f16x4, make_uint2(va.z, va.w));
        }
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const int b = brow0 + j * 16;
            const bool live = oin && b < a.B;
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.eps) {
#pragma unroll
                for (int r = 0; r < 4; ++r) e[r] = pe[i][j][r];
            } else if (i * TB + j < NPRE) {
#pragma unroll
                for (int r = 0; r < 4; ++r) e[r] = pre[i * TB + j < NPRE ? i * TB + j : 0][r];
            } else if (live) {
                philox_normal4(seed, offs, a.rng_stream, (uint64_t)(a.row_offset + b), (uint32_t)(o >> 2), e);
            }
            float res[4], sd[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sd[r] = sqrt_hw(accv[i][j][r] * c_vs[r] + c_bv[r]);
                const float m = accm[i][j][r] * c_ms[r] + c_bm[r] + sd[r] * e[r];
                res[r] = a.relu ? fmaxf(m, 0.f) : m;
            }
            if (a.out && live) {
                float* p = a.out + (size_t)b * a.ldo + o;
                if (ovec) *reinterpret_cast<float4*>(p) = make_float4(res[0], res[1], res[2], res[3]);
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (o + r < a.O) p[r] = res[r];
                }
            }
            if (a.std_out && live) {
                float* p = a.std_out + (size_t)b * a.O + o;
                if (ovec) *reinterpret_cast<float4*>(p) = make_float4(sd[0], sd[1], sd[2], sd[3]);
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (o + r < a.O) p[r] = sd[r];
                }
            }
            if (head) {                                           // wave-uniform; dead lanes contribute zeros
                float hx[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) hx[r] = (live && o + r < a.O) ? res[r] : 0.f;
                const uint32_t h01 = cvt_pk_h(hx[0], hx[1]), h23 = cvt_pk_h(hx[2], hx[3]);
                const uint32_t l01 = cvt_pk_h(hx[0] - h_lo(h01), hx[1] - h_hi(h01)), l23 = cvt_pk_h(hx[2] - h_lo(h23), hx[3] - h_hi(h23));
                const f16x4 xh = __builtin_bit_cast(f16x4, make_uint2(h01, h23)), xl = __builtin_bit_cast(f16x4, make_uint2(l01, l23));
                const float s0 = hx[0] * hx[0] * kS2, s1 = hx[1] * hx[1] * kS2, s2 = hx[2] * hx[2] * kS2, s3 = hx[3] * hx[3] * kS2;
                const uint32_t q01 = cvt_pk_h(s0, s1), q23 = cvt_pk_h(s2, s3);
                const f16x4 sh = __builtin_bit_cast(f16x4, make_uint2(q01, q23));
                hm[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(ehd, xh, hm[j], 0, 0, 0);
                hm[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(eld, xh, hm[j], 0, 0, 0);
                hm[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(ehd, xl, hm[j], 0, 0, 0);
                hv[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(vhd, sh, hv[j], 0, 0, 0);
                if (NPV == 3) {
                    const uint32_t r01 = cvt_pk_h(s0 - h_lo(q01), s1 - h_hi(q01)), r23 = cvt_pk_h(s2 - h_lo(q23), s3 - h_hi(q23));
                    const f16x4 sl = __builtin_bit_cast(f16x4, make_uint2(r01, r23));
                    hv[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(vld, sh, hv[j], 0, 0, 0);
                    hv[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(vhd, sl, hv[j], 0, 0, 0);
                }
            }
            if (a.out_planes) {                                   // wave-uniform; every lane takes part in the swaps
                const uint32_t h01 = cvt_pk_h(res[0], res[1]), h23 = cvt_pk_h(res[2], res[3]);
                const uint32_t l01 = cvt_pk_h(res[0] - h_lo(h01), res[1] - h_hi(h01));
                const uint32_t l23 = cvt_pk_h(res[2] - h_lo(h23), res[3] - h_hi(h23));
                // permlane16_swap(A, B): odd rows (of 16 lanes) of A <-> even rows of B.  With A = hi, B = lo the even lane
                // ends with (own hi, partner's hi) and the odd lane with (partner's lo, own lo): the unit it stores, in k order
                const auto s0 = __builtin_amdgcn_permlane16_swap(h01, l01, false, false);
                const auto s1 = __builtin_amdgcn_permlane16_swap(h23, l23, false, false);
                if (live) {
                    const int kk = o & ~7;
                    char* p = a.out_planes + (size_t)b * a.ldp * 4 + (size_t)(kk >> 5) * 128 + ((kk >> 3) & 3) * 32 + (odd ? 16 : 0);
                    *reinterpret_cast<uint4*>(p) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
                }
            }
        }
    }
    if (head) {
        // lane (b = lr, q): classes 4q .. 4q+3 of row brow0 + 16 j; slab row = [mean 16 | var 16] floats of one batch row
        const int ot = o0 / (TO * 16);
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const int b = brow0 + j * 16;
            if (b < a.B) {
                float* p = a.h_slab + ((size_t)ot * a.B + b) * 32 + 4 * q;
                *reinterpret_cast<float4*>(p) = make_float4(hm[j][0], hm[j][1], hm[j][2], hm[j][3]);
                *reinterpret_cast<float4*>(p + 16) = make_float4(hv[j][0], hv[j][1], hv[j][2], hv[j][3]);
            }
        }
    }
}

// Accumulator tiles whose noise is drawn in the launch ramp, between the issue of the first step's LDS-DMA and the first
// barrier (0 .. TO TB; the rest is drawn in the epilogue): 4, by measurement (gemm_f16s_body keeps the numbers).
// -DLBBNN_G16_NPRE=n overrides it for A/B builds.
#ifndef LBBNN_G16_NPRE
#define LBBNN_G16_NPRE 4
#endif
constexpr int npre_of(int TO, int TB, int NPV) {               // three variance products leave no registers for it
    return NPV == 3 ? 0 : (LBBNN_G16_NPRE < TO * TB ? LBBNN_G16_NPRE : TO * TB);
}

// NPV: products of the variance GEMM (1 or 3).  XPL: x given as fp16 hi | lo planes (else fp32 rows, split in registers).
template <int TO, int TB, int WB, int NPV, bool XPL>
__device__ __forceinline__ void gemm_f16s_body(const G16Args& a) {
    static_assert(NPV == 1 || NPV == 3, "one or three variance products");
    constexpr int BN = TO * 16, BM = TB * WB * 16, NPRE = npre_of(TO, TB, NPV);
    // LDS image of one K step: X BM rows x 128 B | E BN rows x 128 B (hi | lo units) | V: BN rows x 128 B (NPV == 3), or
    // BN rows x 64 B = the hi parts alone, a plain fp16 matrix in memory (NPV == 1: a quarter fewer weight bytes per step)
    constexpr int VROW = NPV == 1 ? 64 : 128;
    constexpr int XB = BM * 128, WRB = BN * 128, VRB = BN * VROW, BUFB = XB + WRB + VRB;
    constexpr int NGX = BM / 8, NGW = BN / 8, NGV = VRB / 1024, NG = NGX + NGW + NGV, NPW = (NG + WB - 1) / WB;
    static_assert(VRB % 1024 == 0, "whole 1-KiB pieces");
    static_assert(EpiImage<TO>::kBytes <= BUFB, "the epilogue's operand image fits one K-step buffer");
    extern __shared__ __attribute__((aligned(16))) char smc[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, q = lane >> 4;
    if ((int)blockIdx.y >= a.gy) {                                             // the finalize row (uniform per workgroup)
        if (blockIdx.x == 0) kl_finalize_piggy<WB>(kernarg_as<G16Args>()->fin, reinterpret_cast<float*>(smc));
        return;
    }
    int tox, tby;
    tile_of_block(tox, tby, a.gx, a.gy);
    const int o0 = tox * BN, b0 = tby * BM;
    uint64_t seed = 0, offs = 0;
    if (!a.eps) { seed = a.rng[0]; offs = a.rng[1]; }

    // LDS-DMA through buffer descriptors (see lrt_gemm_bf16x3_body): per-lane byte offsets computed once, the K step
    // advances a scalar offset of 128 B in every region.  fp32 x: lanes past I in the K tail are pointed out of range
    // (the bounds check returns zeros); planes carry their own zero tail.
    const size_t xsz = XPL ? (size_t)a.B * a.ldx * 4 : ((size_t)(a.B - 1) * a.ldx + a.I) * 4;
    const unsigned xbytes = (unsigned)min((size_t)0x7FFFFFF0u, xsz);
    const unsigned wbytes = (unsigned)min((size_t)0x7FFFFFF0u, (size_t)a.O * a.ld * 4);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc((void*)a.e_w, 0, (int)wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)a.var_w, 0, (int)(NPV == 1 ? wbytes / 2 : wbytes), 0x00020000);
    int gv[NPW], kx[NPW];
#pragma unroll
    for (int u = 0; u < NPW; ++u) {
        const int g = wv + WB * u;
        if (g < NGX) {
            const int row = 8 * g + (lane >> 3);
            const int slot = (lane & 7) ^ swzx(row & 15);
            gv[u] = (int)((size_t)min(b0 + row, a.B - 1) * a.ldx * 4) + 16 * slot;
            kx[u] = XPL ? -1 : 4 * slot;
        } else if (g < NGX + NGW || NPV == 3) {
            const int gw = g - NGX, row = 8 * (gw % NGW) + (lane >> 3);
            const int slot = (lane & 7) ^ swzx(row & 15);
            gv[u] = (int)((size_t)min(o0 + row, a.O - 1) * a.ld * 4) + 16 * slot;
            kx[u] = -1;
        } else {
            const int gw = g - NGX - NGW, row = 16 * gw + (lane >> 2);                   // hi-only var_w: 16 rows x 64 B per piece
            const int slot = (lane & 3) ^ swz4(row >> 2);
            gv[u] = (int)((size_t)min(o0 + row, a.O - 1) * a.ld * 2) + 16 * slot;
            kx[u] = -1;
        }
    }
    const int nsteps = (a.I + BKS - 1) / BKS;
    const bool has_tail = !XPL && (a.I % BKS) != 0;
    int gvt[NPW];                                         // the K-tail step's offsets in registers of their own (lrt_gemm.hip)
#pragma unroll
    for (int u = 0; u < NPW; ++u)
        gvt[u] = (kx[u] >= 0 && (nsteps - 1) * BKS + kx[u] >= a.I) ? 0x7FFFFFF0 : gv[u];
    auto dma_pieces = [&](int c, char* buf, const int (&va)[NPW]) {
#pragma unroll
        for (int u = 0; u < NPW; ++u) {
            const int g = wv + WB * u;                   // wave-uniform
            if (g < NG) {
                const int loff = g < NGX ? g * 1024 : XB + (g - NGX) * 1024;
                auto* dst = (__attribute__((address_space(3))) void*)(buf + loff);
                if (g < NGX)                 __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, dst, 16, va[u], c * 128, 0, 0);
                else if (g - NGX < NGW)      __builtin_amdgcn_raw_ptr_buffer_load_lds(re, dst, 16, va[u], c * 128, 0, 0);
                else                         __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, dst, 16, va[u], c * VROW, 0, 0);
            }
        }
    };
    auto dma_step = [&](int c, char* buf) {
        if (has_tail && c == nsteps - 1) dma_pieces(c, buf, gvt);
        else dma_pieces(c, buf, gv);
    };

    floatx4 accm[TO][TB], accv[TO][TB];
#pragma unroll
    for (int i = 0; i < TO; ++i)
#pragma unroll
        for (int j = 0; j < TB; ++j) { accm[i][j] = floatx4{0.f, 0.f, 0.f, 0.f}; accv[i][j] = floatx4{0.f, 0.f, 0.f, 0.f}; }

    const int gx = swzx(lr);
    const int xo0 = (wv * TB * 16 + lr) * 128 + 16 * ((2 * q) ^ gx);
    const int xo1 = (wv * TB * 16 + lr) * 128 + 16 * ((2 * q + 1) ^ gx);
    const int woh = XB + lr * 128 + 16 * ((2 * q) ^ gx);
    const int wol = XB + lr * 128 + 16 * ((2 * q + 1) ^ gx);
    const int vo1 = XB + WRB + lr * 64 + 16 * (q ^ swz4(lr >> 2));        // NPV == 1: row lr of the 64-B-row V region, unit q

    uint4 xu[TB][2];
    uint4 eh[TO], el[TO], vh[TO], vl[TO];
    auto read_frags = [&](const char* cur) {
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            xu[j][0] = *reinterpret_cast<const uint4*>(cur + xo0 + j * 16 * 128);
            xu[j][1] = *reinterpret_cast<const uint4*>(cur + xo1 + j * 16 * 128);
        }
#pragma unroll
        for (int i = 0; i < TO; ++i) {
            eh[i] = *reinterpret_cast<const uint4*>(cur + woh + i * 16 * 128);
            el[i] = *reinterpret_cast<const uint4*>(cur + wol + i * 16 * 128);
            if (NPV == 3) {
                vh[i] = *reinterpret_cast<const uint4*>(cur + WRB + woh + i * 16 * 128);
                vl[i] = *reinterpret_cast<const uint4*>(cur + WRB + wol + i * 16 * 128);
            } else {
                vh[i] = *reinterpret_cast<const uint4*>(cur + vo1 + i * 16 * 64);
            }
        }
    };
    auto mfmas = [&]() {
        f16x8 xh[TB], xl[TB], sh[TB], sl[TB];
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            if (XPL) {
                xh[j] = __builtin_bit_cast(f16x8, xu[j][0]);
                xl[j] = __builtin_bit_cast(f16x8, xu[j][1]);
                if (NPV == 1) {
                    // s = (x 2^-4)^2 from the planes: a = xh 2^-4, b = xl 2^-3, s = a a + a b   (x^2 = xh^2 + 2 xh xl + O(2^-24))
                    const f16x8 pa = xh[j] * (_Float16)0.0625f, pb = xl[j] * (_Float16)0.125f;
                    const f16x8 t = pa * pb;
                    sh[j] = pa * pa + t;
                } else {
                    uint32_t ph[4], pl[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float h0 = (float)xh[j][2 * t], h1 = (float)xh[j][2 * t + 1];
                        const float l0 = (float)xl[j][2 * t], l1 = (float)xl[j][2 * t + 1];
                        const float s0 = (h0 * h0 + 2.f * h0 * l0) * kS2, s1 = (h1 * h1 + 2.f * h1 * l1) * kS2;
                        ph[t] = cvt_pk_h(s0, s1);
                        pl[t] = cvt_pk_h(s0 - h_lo(ph[t]), s1 - h_hi(ph[t]));
                    }
                    sh[j] = __builtin_bit_cast(f16x8, make_uint4(ph[0], ph[1], ph[2], ph[3]));
                    sl[j] = __builtin_bit_cast(f16x8, make_uint4(pl[0], pl[1], pl[2], pl[3]));
                }
            } else {
                const float4 f0 = __builtin_bit_cast(float4, xu[j][0]), f1 = __builtin_bit_cast(float4, xu[j][1]);
                const float v[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                uint32_t ph[4], pl[4], qh[4] = {0, 0, 0, 0}, ql[4] = {0, 0, 0, 0};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float v0 = v[2 * t], v1 = v[2 * t + 1];
                    ph[t] = cvt_pk_h(v0, v1);
                    pl[t] = cvt_pk_h(v0 - h_lo(ph[t]), v1 - h_hi(ph[t]));
                    if (NPV == 3) {
                        const float s0 = (v0 * v0) * kS2, s1 = (v1 * v1) * kS2;
                        qh[t] = cvt_pk_h(s0, s1);
                        ql[t] = cvt_pk_h(s0 - h_lo(qh[t]), s1 - h_hi(qh[t]));
                    }
                }
                xh[j] = __builtin_bit_cast(f16x8, make_uint4(ph[0], ph[1], ph[2], ph[3]));
                xl[j] = __builtin_bit_cast(f16x8, make_uint4(pl[0], pl[1], pl[2], pl[3]));
                if (NPV == 1) {
                    // the one variance product takes s from the halves just made, as the plane form does (a a + a b: four packed
                    // fp16 instructions per 8 k instead of two packed fp32 multiplies and a conversion per 2 k) -- and a layer fed
                    // fp32 rows now computes bit for bit what the same layer computes from lbbnn_format_x's planes
                    const f16x8 pa = xh[j] * (_Float16)0.0625f, pb = xl[j] * (_Float16)0.125f;
                    const f16x8 t2 = pa * pb;
                    sh[j] = pa * pa + t2;
                } else {
                    sh[j] = __builtin_bit_cast(f16x8, make_uint4(qh[0], qh[1], qh[2], qh[3]));
                }
                sl[j] = __builtin_bit_cast(f16x8, make_uint4(ql[0], ql[1], ql[2], ql[3]));
            }
        }
#pragma unroll
        for (int j = 0; j < TB; ++j) {
#pragma unroll
            for (int i = 0; i < TO; ++i) {
                const f16x8 ah = __builtin_bit_cast(f16x8, eh[i]), al = __builtin_bit_cast(f16x8, el[i]);
                accm[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xh[j], accm[i][j], 0, 0, 0);
                accm[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, xh[j], accm[i][j], 0, 0, 0);
                accm[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xl[j], accm[i][j], 0, 0, 0);
                const f16x8 bh = __builtin_bit_cast(f16x8, vh[i]);
                accv[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, sh[j], accv[i][j], 0, 0, 0);
                if (NPV == 3) {
                    accv[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vl[i]), sh[j], accv[i][j], 0, 0, 0);
                    accv[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, sl[j], accv[i][j], 0, 0, 0);
                }
            }
        }
    };

    // (Measured and dropped, round 3 -- VERDICT r02 item 3: x taken OUT of the LDS-DMA path.  A wave's 32 x rows are read by no other
    // wave, so each lane fetched its 32 B per row and step straight into registers (two buffer_load_dwordx4, one K step ahead, a
    // second register set, loop unrolled by two; LDS held the weight regions alone: 15 pieces per step instead of 31).
    // Bit-identical outputs; 0.1514 ms per forward against 0.1382 in the same process (commit "Experiment: x global->VGPR").
    // A fragment-shaped load touches 16 cache lines for 1 KiB where an LDS-DMA piece touches 8 whole lines: the address path,
    // not the byte rate, is what the x operand loads -- the cdna guide's GEMM table reports the same (+18...45 %).)
    // (Measured and dropped, round 3: drawing the noise of accumulator tile c INSIDE K step c < 8 -- Philox in the shadow of the
    // step's MFMAs, the VALU port being idle four cycles out of five in this loop -- bit-identical outputs, no spills at 8
    // tiles, and 0.1499 ms per forward against 0.1473: a wave issues in order, so the 140 instructions lengthen ITS chain of
    // the step by what the epilogue saves, and the chain of a wave, not the occupancy of a pipe, is what a step costs.)
    // (Measured and dropped, round 3, after the VALU trims (forward 0.1255 ms); all bit-identical.
    // (a) ROLLING FRAGMENT PREFETCH -- the weight fragments of tile row i re-loaded for step c + 1 right after step c's MFMAs
    //     of row i (same registers, order given by sched_group_barrier; 15 of the 19 ds_reads under the wave's own MFMAs), the
    //     LDS-DMA two steps ahead: 0.1303 ms -- the piece issue then sits between the barrier and the first MFMA instead of
    //     under the ds_read latency; with the issue after the MFMA groups: 0.1318 against 0.1271.
    // (b) STRAIGHT-LINE PIECE ISSUE -- per-piece descriptors / LDS offsets / strides in scalar registers set up once, 8 x
    //     (s_mov m0, s_add, buffer_load lds) per step instead of ~20 scalar branches: 0.1276 ms.
    // (a) + (b) with the pieces issued two at a time BETWEEN the MFMA groups: 0.1559 ms -- a wave issues in order, and a
    //     buffer_load ... lds that waits for a slot in the vector-memory queue holds back the MFMAs behind it.
    // (c) 64 x 80 per wave, two waves per workgroup, one wave per SIMD with 160 accumulator AGPRs (`<5, 4, 2>`: every weight
    //     fragment read by two waves instead of four): 0.1699 ms against 0.1271 -- nothing hides a lone wave's waits.
    // (d) x global -> VGPR from FRAGMENT-ORDERED planes (timing only: every load instruction 1 KiB contiguous, the penalty of
    //     the row-major form above gone), LDS holding the weights alone: 0.1288 against 0.1289; the same with THREE weight
    //     buffers and the LDS-DMA two steps ahead (vmcnt-counted barrier): 0.1282 against 0.1279.  Neither the LDS (x no longer
    //     in it) nor the latency of a piece (a whole extra step of slack) is what a step waits for.
    // What is left: the CU's ONE vector-memory path takes ~20 cycles per KiB whatever the destination (62 KiB per CU-step =
    // 1240 cycles), a wave stands still while its pieces / loads queue for it (~100 cycles each with eight waves queueing), and
    // the 2 x 640 MFMA cycles of a SIMD's two waves fit into what remains of the 2592-cycle step only where the other wave is
    // not queueing too.  The piece issue is cheapest where it is, under the ds_read latency.)
    // (VERDICT r02 item 6's premise tested, round 3: the second workgroup of every CU (linear id >= 256) delayed by d at its
    // start, so that one workgroup's VALU-bound epilogue falls beside the other's LDS-bound loop: forward 0.1255 ms at
    // d = 0, 0.1271 / 0.1279 / 0.1304 / 0.1322 at d = 0.85 / 1.7 / 3.4 / 5.1 us -- two thirds of every microsecond of skew
    // come back as time.  A workgroup looping alone does not use what its neighbour leaves free, so an uneven K split
    // between them would buy less than its combine costs: not built.)
    // (The first layer's in-register split of fp32 x on v_fma_mixlo/mixhi_f16 (f16(x - float(h)) in one instruction per
    // element, inline asm: 3 VALU per pair instead of the compiler's 5, bit-identical): forward 0.1240 / 0.1238 / 0.1237 ms
    // against 0.1240 / 0.1237 / 0.1237 -- the 16 instructions per wave-step are not on the chain either; dropped.)
    // (The launch's K-independent part: epilogue operands staged once per workgroup (EpiImage) and NPRE tiles' noise drawn in
    // the ramp.  All bit-identical; forward ms, builds in alternating processes, one line per box (profiles/f16_epilogue_ab.txt):
    //   parent 0.1290 | image loaded AHEAD of the last step's MFMAs and written after them 0.1336 -- the wave issues in order and
    //     21 more live registers cross the MFMAs: slower than fetching per wave; dropped | loads and writes behind the MFMAs,
    //     NPRE = 6: 0.1216
    //   parent 0.1245 | behind the MFMAs, NPRE = 0 / 4 / 6 / 8: 0.1198 / 0.1172 / 0.1189 / 0.1199 (8 spills 3 VGPRs with fp32 x)
    //   parent 0.1214 | NPRE = 0 / 4: 0.1169 / 0.1166 | the staging as ONE function with every load unconditional (clamped
    //     index, fill selected afterwards: one round trip instead of three): 0.1192; dropped, the form below is the measured one.
    // The first step's round trip hides about four tiles' Philox; what is drawn beyond that delays the first MFMA by as much as
    // the epilogue gains.  Three variance products leave no registers for it (NPRE = 6: 47-52 VGPRs spilled): NPRE = 0 there.)
    const int brow0 = b0 + wv * TB * 16 + lr;
    float pre[NPRE > 0 ? NPRE : 1][4];
    dma_step(0, smc);
    if (NPRE > 0) {
        // the first pieces are on their round trip and the VALU has nothing else to do: the Philox rounds of the first NPRE
        // tiles sit ahead of the first barrier (same counters, stream and guards as the epilogue's own draws)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NPRE; ++t) {
            const int o = o0 + (t / TB) * 16 + 4 * q, b = brow0 + (t % TB) * 16;
            pre[t][0] = pre[t][1] = pre[t][2] = pre[t][3] = 0.f;
            if (!a.eps && o < a.O && b < a.B)
                philox_normal4(seed, offs, a.rng_stream, (uint64_t)(a.row_offset + b), (uint32_t)(o >> 2), pre[t]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    // The last step issues no LDS-DMA; the buffer it would have filled is idle (consumed in step nsteps - 2, and with one
    // step never used): the epilogue's operand image goes there, loads and ds_writes behind the step's MFMAs, published by
    // the step's own closing s_waitcnt + barrier.  The steps before it run the stream they always ran.
    char* const img = smc + (nsteps & 1) * BUFB;
    EpiStage<(TO + WB - 1) / WB> st;
    for (int c = 0; c < nsteps; ++c) {
        read_frags(smc + (c & 1) * BUFB);
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < nsteps) dma_step(c + 1, smc + ((c & 1) ^ 1) * BUFB);
        __builtin_amdgcn_sched_barrier(0);
        mfmas();
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 == nsteps) {
            stage_load<TO, WB>(*kernarg_as<G16Args>(), o0, tid, st);
            stage_store<TO, WB, NPV>(*kernarg_as<G16Args>(), tid, st, img);
        }
        __syncthreads();
    }
    epilogue16<TO, TB, NPV, NPRE>(*kernarg_as<G16Args>(), o0, q, lr, brow0, img, seed, offs, pre, accm, accv);
}

template <int TO, int TB, int WB, int NPV, bool XPL>
__global__ __launch_bounds__(WB * 64, 2) void lrt_gemm_f16s_kernel(const G16Args a) {
    gemm_f16s_body<TO, TB, WB, NPV, XPL>(a);
}

template <int TO, int TB, int WB>
int launch16(G16Args& a, int npv, bool xpl, hipStream_t s, bool* hosted) {
    constexpr int BN = TO * 16, BM = TB * WB * 16;
    dim3 grid((a.O + BN - 1) / BN, (a.B + BM - 1) / BM, 1), block(WB * 64);
    const long nblocks = (long)grid.x * grid.y;
    const size_t lds = lds_request(2u * (BM * 128 + BN * 128 + BN * (npv == 1 ? 64 : 128)), nblocks);
    const int fin_n = a.fin.n;
    a.gx = (int)grid.x; a.gy = (int)grid.y;
    a.fin.n = 0;
    if (fin_n > 0 && hosted) {
        a.fin.n = fin_n;
        if (piggy_lds_bytes(a.fin) <= lds) { grid.y += 1; *hosted = true; }
        else a.fin.n = 0;
    }
    if (npv == 1) {
        if (xpl) return launch_one(lrt_gemm_f16s_kernel<TO, TB, WB, 1, true>, grid, block, lds, s, a);
        return launch_one(lrt_gemm_f16s_kernel<TO, TB, WB, 1, false>, grid, block, lds, s, a);
    }
    if (xpl) return launch_one(lrt_gemm_f16s_kernel<TO, TB, WB, 3, true>, grid, block, lds, s, a);
    return launch_one(lrt_gemm_f16s_kernel<TO, TB, WB, 3, false>, grid, block, lds, s, a);
}

// fp32 rows -> planes as a launch of its own (lbbnn_device.h: format_x_items; a fused forward lets the same job ride in the
// weight-pass launch instead: lbbnn_layers_operands_x)
__global__ __launch_bounds__(256) void format_x_kernel(const FormatJob j) {
    format_x_items(j, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}

// Second half of the head fold: out[b][c] = log_softmax_c( sum_ot mean[ot][b][c] / 2^8 + bias_mean[c]
//                                                        + sqrt(sum_ot var[ot][b][c] 2^8 / 2^14 + bias_var[c]) eps[b][c] )
// (LBBNN-GP-MF-MNF.py:197-200 for the last layer, :256 log_softmax); deterministic: every sum has a fixed order.
struct HeadFinArgs {
    const float* slab; const float* bias_mean; const float* bias_var; const float* eps; const uint64_t* rng;
    float* out; long long row_offset;
    int n_ot, B, C, ldo, log_softmax; uint32_t rng_stream;
};

// Sixteen lanes (one DPP row) per batch row: lane = 4 q + g owns classes 4q .. 4q+3 and the o tiles g, g + 4, g + 8, ... --
// at most four pairs of 16-B loads per lane, all in flight together (a thread per (row, q) that walked all 15 tiles made
// the launch latency-bound on 64 workgroups: 7.1 us for 7.9 MB); the partial sums are combined in a fixed order by DPP.
__global__ __launch_bounds__(256) void head_finalize_kernel(const HeadFinArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = t >> 4, q = (t >> 2) & 3, g = t & 3;
    const bool rowok = b < a.B;
    float m[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    if (rowok) {
        float4 pm[4], pv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ot = g + 4 * k;
            pm[k] = make_float4(0.f, 0.f, 0.f, 0.f); pv[k] = pm[k];
            if (ot < a.n_ot) {
                const float* p = a.slab + ((size_t)ot * a.B + b) * 32 + 4 * q;
                pm[k] = *reinterpret_cast<const float4*>(p); pv[k] = *reinterpret_cast<const float4*>(p + 16);
            }
        }
        for (int ot = g + 16; ot < a.n_ot; ot += 4) {              // more than 16 o tiles (O > 1280): the rest, sequentially
            const float* p = a.slab + ((size_t)ot * a.B + b) * 32 + 4 * q;
            const float4 xm = *reinterpret_cast<const float4*>(p), xv = *reinterpret_cast<const float4*>(p + 16);
            pm[0].x += xm.x; pm[0].y += xm.y; pm[0].z += xm.z; pm[0].w += xm.w;
            pv[0].x += xv.x; pv[0].y += xv.y; pv[0].z += xv.z; pv[0].w += xv.w;
        }
        m[0] = (pm[0].x + pm[1].x) + (pm[2].x + pm[3].x); m[1] = (pm[0].y + pm[1].y) + (pm[2].y + pm[3].y);
        m[2] = (pm[0].z + pm[1].z) + (pm[2].z + pm[3].z); m[3] = (pm[0].w + pm[1].w) + (pm[2].w + pm[3].w);
        v[0] = (pv[0].x + pv[1].x) + (pv[2].x + pv[3].x); v[1] = (pv[0].y + pv[1].y) + (pv[2].y + pv[3].y);
        v[2] = (pv[0].z + pv[1].z) + (pv[2].z + pv[3].z); v[3] = (pv[0].w + pv[1].w) + (pv[2].w + pv[3].w);
    }
    // the four o-tile groups of a (row, q) sit in one quad: lane ^ 1, lane ^ 2 -- every lane of the quad ends with the sum
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        m[r] += dpp_get<0xB1>(m[r]); m[r] += dpp_get<0x4E>(m[r]);
        v[r] += dpp_get<0xB1>(v[r]); v[r] += dpp_get<0x4E>(v[r]);
    }
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    const int c0 = 4 * q;
    if (rowok && c0 < a.C) {
        if (a.eps) {
#pragma unroll
            for (int r = 0; r < 4; ++r) if (c0 + r < a.C) e[r] = a.eps[(size_t)b * a.C + c0 + r];
        } else {
            philox_normal4(a.rng[0], a.rng[1], a.rng_stream, (uint64_t)(a.row_offset + b), (uint32_t)q, e);
        }
    }
    float res[4];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + r;
        const bool in = rowok && c < a.C;
        const float bm = (in && a.bias_mean) ? a.bias_mean[c] : 0.f, bv = (in && a.bias_var) ? a.bias_var[c] : 0.f;
        const float sd = sqrt_hw(v[r] * (kS2inv / kHeadVS) + bv);
        res[r] = m[r] * (1.f / kHeadES) + bm + sd * e[r];
        if (in) mx = fmaxf(mx, res[r]);
    }
    if (a.log_softmax) {
        // over the row's four q groups: quads of one 16-lane DPP row (all four lanes of a quad hold the same values)
        mx = fmaxf(mx, dpp_get<0x141>(mx));
        mx = fmaxf(mx, dpp_get<0x140>(mx));
        float se = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) if (rowok && c0 + r < a.C) se += expf(res[r] - mx);
        se += dpp_get<0x141>(se);
        se += dpp_get<0x140>(se);
        const float lse = mx + logf(se);
#pragma unroll
        for (int r = 0; r < 4; ++r) res[r] -= lse;
    }
    if (rowok && g == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r) if (c0 + r < a.C) a.out[(size_t)b * a.ldo + c0 + r] = res[r];
}

}  // namespace

extern "C" int64_t lbbnn_head_slab_floats(int B, int O) {
    if (B <= 0 || O <= 0) return 0;
    return (int64_t)((O + 79) / 80) * B * 32;
}

extern "C" int lbbnn_format_x(const float* x, int ldx, void* planes, int ldp, int B, int I, void* stream) {
    if (B == 0) return 0;
    if (!x || !planes) return LBBNN_E_NULL;
    if (B < 0 || I <= 0 || ldx < I || ldp < I) return LBBNN_E_SHAPE;
    if ((I & 7) || (ldx & 3) || (ldp & 31) || (reinterpret_cast<uintptr_t>(x) & 15u) || (reinterpret_cast<uintptr_t>(planes) & 15u))
        return LBBNN_E_ALIGN;
    const size_t n = (size_t)B * (ldp >> 3);
    const int blocks = (int)min((size_t)2048, (n + 255) / 256);
    const FormatJob j{x, static_cast<char*>(planes), ldx, ldp, B, I};
    hipLaunchKernelGGL(format_x_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), j);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_lrt_gemm_ex(const lbbnn_gemm_desc_t* d, void* stream) {
    if (!d) return LBBNN_E_NULL;
    const int B = d->B, I = d->I, O = d->O, flags = d->flags;
    if (!(flags & LBBNN_F_F16S)) return gemm_desc_f32(*d, stream);       // fp32 / bf16 operands: lrt_gemm.hip
    if (flags & ~(LBBNN_F_RELU | LBBNN_F_F16S | LBBNN_F_VAR1 | LBBNN_F_XPLANES)) return LBBNN_E_FLAGS;
    if (B == 0 && I > 0 && O > 0 && d->n_layers == 0 && !d->advance) return 0;
    if (!d->x || !d->e_w || !d->var_w || !d->mean_scale || !d->wvar_scale) return LBBNN_E_NULL;
    if (!d->eps && !d->rng) return LBBNN_E_NOISE;
    if (B <= 0 || I <= 0 || O <= 16 || d->ldx < I || (d->out && d->ldo < O)) return LBBNN_E_SHAPE;
    const bool xpl = (flags & LBBNN_F_XPLANES) != 0;
    if (d->ld < I || (d->ld & 31) || (I & 7)) return LBBNN_E_ALIGN;
    if ((I % BKS) != 0 && (d->ld - I) < 8) return LBBNN_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(d->e_w) | reinterpret_cast<uintptr_t>(d->var_w) | reinterpret_cast<uintptr_t>(d->x)) & 15u) return LBBNN_E_ALIGN;
    if (xpl ? (d->ldx & 31) != 0 : (d->ldx & 3) != 0) return LBBNN_E_ALIGN;
    if (d->out_planes && ((O & 7) || (d->ldp & 31) || d->ldp < O || (reinterpret_cast<uintptr_t>(d->out_planes) & 15u))) return LBBNN_E_ALIGN;
    if ((size_t)B * d->ldx * 4 >= 0x7FFFFFF0u || (size_t)O * d->ld * 4 >= 0x7FFFFFF0u) return LBBNN_E_SHAPE;   // 32-bit buffer offsets
    if (d->n_layers < 0 || (d->n_layers > 0 && !d->layers) || (d->advance && !d->rng_live)) return LBBNN_E_NULL;
    const bool head = d->head_out != nullptr;
    if (head) {
        if (!d->head_e || !d->head_v || !d->head_slab) return LBBNN_E_NULL;
        if (d->head_classes <= 0 || d->head_classes > 16 || d->head_ld < O || (d->head_ld & 3) || d->head_ldo < d->head_classes) return LBBNN_E_SHAPE;
        if ((O & 3) || ((reinterpret_cast<uintptr_t>(d->head_e) | reinterpret_cast<uintptr_t>(d->head_v) | reinterpret_cast<uintptr_t>(d->head_slab)) & 15u)) return LBBNN_E_ALIGN;
        if (!d->head_eps && !d->rng) return LBBNN_E_NOISE;
        if (!(flags & LBBNN_F_RELU)) return LBBNN_E_FLAGS;        // the head reads relu(this layer) (LBBNN-GP-MF-MNF.py:255-256)
    } else if (!d->out && !d->out_planes) return LBBNN_E_NULL;

    G16Args a;
    a.x = static_cast<const char*>(d->x); a.e_w = static_cast<const char*>(d->e_w); a.var_w = static_cast<const char*>(d->var_w);
    a.mean_scale = d->mean_scale; a.wvar_scale = d->wvar_scale;
    a.bias_mean = d->bias_mean; a.bias_var = d->bias_var; a.var_scale = d->var_scale;
    a.eps = d->eps; a.rng = d->rng; a.out = d->out; a.out_planes = static_cast<char*>(d->out_planes); a.std_out = d->std_out;
    a.row_offset = d->row_offset; a.ldx = d->ldx; a.ld = d->ld; a.ldo = d->ldo; a.ldp = d->ldp; a.B = B; a.I = I; a.O = O;
    a.rng_stream = d->rng_stream; a.relu = (flags & LBBNN_F_RELU) ? 1 : 0;
    a.h_e = head ? d->head_e : nullptr; a.h_v = head ? d->head_v : nullptr; a.h_slab = head ? d->head_slab : nullptr;
    a.h_ld = d->head_ld; a.h_C = d->head_classes;
    a.fin = FinalizePiggy{};
    const bool want_fin = d->n_layers > 0 || d->advance;
    if (d->n_layers > 0) {
        if (const int rc = fill_finalize_args(d->layers, d->n_layers, d->fin_rng, a.fin.l, a.fin.active)) return rc;
        if (d->kl_total) for (int i = 0; i < d->n_layers; ++i) if (!a.fin.active[i]) return LBBNN_E_NULL;
        a.fin.n = d->n_layers; a.fin.total = d->kl_total;
        a.fin.rng_adv = d->advance ? d->rng_live : nullptr; a.fin.adv = d->advance;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int npv = (flags & LBBNN_F_VAR1) ? 1 : 3;
    bool hosted = false;
    const long blocks_big = (long)((O + 79) / 80) * ((B + 127) / 128);
    int rc;
    // Tile configurations measured and dropped in round 3 (3 + 1 form, headline net, tools/precision_time.py): 256 x 80 with
    // eight waves and one workgroup per CU (<5,2,8>: a third fewer LDS-DMA pieces per product) 0.1513 ms per forward against
    // 0.1442 -- one barrier-locked workgroup loses the overlap two independent ones give each other; 128 x 80 with eight waves
    // of 16 rows at four waves per SIMD (<5,1,8>) does not fit 128 VGPRs (61-96 spilled).
    if (blocks_big >= 256 && B >= 96) rc = launch16<5, 2, 4>(a, npv, xpl, s, &hosted);
    else rc = launch16<5, 1, 2>(a, npv, xpl, s, &hosted);
    if (rc) return rc;
    if (head) {
        HeadFinArgs h;
        h.slab = d->head_slab; h.bias_mean = d->head_bias_mean; h.bias_var = d->head_bias_var; h.eps = d->head_eps; h.rng = d->rng;
        h.out = d->head_out; h.row_offset = d->row_offset; h.n_ot = (O + 79) / 80; h.B = B; h.C = d->head_classes; h.ldo = d->head_ldo;
        h.log_softmax = (d->head_flags & LBBNN_F_LOG_SOFTMAX) ? 1 : 0; h.rng_stream = d->head_rng_stream;
        hipLaunchKernelGGL(head_finalize_kernel, dim3((16 * (size_t)B + 255) / 256), dim3(256), 0, s, h);
        rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    if (!want_fin || hosted) return rc;
    if (d->n_layers > 0)
        return launch_kl_finalize_all(a.fin.l, a.fin.active, d->n_layers, d->advance ? d->rng_live : nullptr, d->advance,
                                      d->kl_total, s);
    return lbbnn_rng_advance(d->rng_live, d->advance, stream);
}
