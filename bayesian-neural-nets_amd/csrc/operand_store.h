// What writes a GEMM operand, once: the bf16 hi | lo split, the stores of both operand formats (fp32 rows, or the 16-B
// hi | lo units of lbbnn_device.h), the gate draw whose product is stored, and the two index rules of the batched row
// kernels (which layer a workgroup belongs to, which full index a compact index maps to).  The split layout is the contract
// between these writers and the GEMM's reader (gemm_common.h).  The frozen models (frozen.hip, base_frozen.hip) store through
// here; K1's row kernel (weight_pass.hip) and gate_members_kernel (gate_vd.hip) take the split and the exchange from here and
// spell out their address and store, because their instruction streams are pinned.
#pragma once
#include "lbbnn_device.h"

namespace lbbnn {

// ------------------------------------------------------------------------------------------------ the split, four at a time
// w = hi + lo (both bf16): hi = rne(w), lo = rne(w - hi); packs 4 elements into two uint2.  The roundings are the hardware's
// v_cvt_pk_bf16_f32 (RNE, two values per instruction): ~12 VALU per float4 instead of ~50 for the integer form below,
// bit-identical for finite inputs.
typedef __bf16 os_bf16x2 __attribute__((ext_vector_type(2)));
typedef float os_floatx2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t cvt_pk(float a, float b) {
    const os_floatx2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, os_bf16x2));
}
__device__ __forceinline__ void split4(const float4 w, uint2& hi, uint2& lo) {
    const uint32_t h0 = cvt_pk(w.x, w.y), h1 = cvt_pk(w.z, w.w);
    hi = make_uint2(h0, h1);
    lo = make_uint2(cvt_pk(w.x - __uint_as_float(h0 << 16), w.y - __uint_as_float(h0 & 0xFFFF0000u)),
                    cvt_pk(w.z - __uint_as_float(h1 << 16), w.w - __uint_as_float(h1 & 0xFFFF0000u)));
}
__device__ __forceinline__ uint32_t dpp_xor1(uint32_t v) { return (uint32_t)dpp_mov<0xB1>((int)v); }   // lane ^ 1

// The hi | lo halves of one group (columns 4j .. 4j+3 of row o) to memory as whole 16-B units: the even lane of a pair holds
// k = 8m..8m+3, the odd lane k = 8m+4..8m+7; the even lane stores the hi unit (its hi half | the partner's), the odd lane the
// lo unit next to it -- a wave covers 1 KiB contiguous.  EVERY lane of the wave must call this (the exchange is a DPP move);
// `in` says whether the lane stores (its group lies inside the padded row; ld / 4 is a multiple of 8: both lanes of a pair
// agree).  hi / lo are bf16 pairs, or the fp16 pairs of K1's row-scaled format.
__device__ __forceinline__ uint4 pair_unit(bool odd, const uint2 hi, const uint2 lo) {
    const uint32_t r0 = dpp_xor1(odd ? hi.x : lo.x), r1 = dpp_xor1(odd ? hi.y : lo.y);
    return make_uint4(odd ? r0 : hi.x, odd ? r1 : hi.y, odd ? lo.x : r0, odd ? lo.y : r1);
}
__device__ __forceinline__ void store_pair_units(void* base, int o, int j, int ld, bool in, const uint2 hi, const uint2 lo) {
    const bool odd = threadIdx.x & 1;
    const size_t at = split_hi_index((size_t)o, 4 * (j & ~1), ld) + (odd ? kSplitLoOffset : 0);
    const uint4 unit = pair_unit(odd, hi, lo);
    if (in) *reinterpret_cast<uint4*>(static_cast<uint16_t*>(base) + at) = unit;
}
// One operand group to memory in either format.  fp32: the float4 itself.  Split: store_pair_units of its bf16 split, so
// EVERY lane of the wave must call this too.
__device__ __forceinline__ void store4_operand(float* base, int o, int j, int ld, bool split, bool in, const float4 w) {
    if (!split) {
        if (in) reinterpret_cast<float4*>(base + (size_t)o * ld)[j] = w;
        return;
    }
    uint2 hi, lo;
    split4(w, hi, lo);
    store_pair_units(base, o, j, ld, in, hi, lo);
}

// ------------------------------------------------------------------------------------------------ the split, one at a time
// round-to-nearest-even fp32 -> bf16 bits (finite inputs), the integer form
__device__ __forceinline__ uint32_t bf16_rne_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// the split bf16 pair of one operand value: hi | lo << 16 (hi = RNE(v), lo = RNE(v - hi))
__device__ __forceinline__ uint32_t bf16_hi_lo(float v) {
    const uint32_t h = bf16_rne_bits(v);
    return h | (bf16_rne_bits(v - __uint_as_float(h << 16)) << 16);
}
// eight values of columns [i0, i0 + 8) of row o of an fp32 plane / of a GEMM operand in either format: two float4, or one
// hi unit and one lo unit -- no exchange between lanes
__device__ __forceinline__ void store8(float* base, size_t o, int i0, int ld, const float w[8]) {
    float* const p = base + o * ld + i0;
    *reinterpret_cast<float4*>(p) = make_float4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(w[4], w[5], w[6], w[7]);
}
__device__ __forceinline__ void store8_operand(void* base, bool split, size_t row, int i0, int ld, const float w[8]) {
    if (!split) { store8(static_cast<float*>(base), row, i0, ld, w); return; }
    uint32_t hl[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) hl[k] = bf16_hi_lo(w[k]);
    uint16_t* const p = static_cast<uint16_t*>(base) + split_hi_index(row, i0, ld);
    *reinterpret_cast<uint4*>(p) = make_uint4((hl[0] & 0xFFFFu) | (hl[1] << 16), (hl[2] & 0xFFFFu) | (hl[3] << 16),
                                              (hl[4] & 0xFFFFu) | (hl[5] << 16), (hl[6] & 0xFFFFu) | (hl[7] << 16));
    *reinterpret_cast<uint4*>(p + kSplitLoOffset) =
        make_uint4((hl[0] >> 16) | (hl[1] & 0xFFFF0000u), (hl[2] >> 16) | (hl[3] & 0xFFFF0000u),
                   (hl[4] >> 16) | (hl[5] & 0xFFFF0000u), (hl[6] >> 16) | (hl[7] & 0xFFFF0000u));
}

// ------------------------------------------------------------------------------------------------ the gate of a drawn weight
constexpr float kProbEps = 1.1920928955078125e-7f;      // torch.finfo(float32).eps: clamp_probs
constexpr float kTiny = 1.17549435082228750797e-38f;    // torch.finfo(float32).tiny: _clipped_sigmoid, Gamma.rsample

// 24 random bits -> (k + 0.5) 2^-24: strictly inside (0, 1), exact in fp32
__device__ __forceinline__ float uniform24(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-8f; }

// RelaxedBernoulli(probs = al, temperature = T).rsample() given its uniform (torch: LogitRelaxedBernoulli.rsample + the
// clipped SigmoidTransform); hard: Bernoulli(al).sample() as u < al.  *dcda: dc/d al (0 where a clamp is active).
__device__ __forceinline__ float gate_draw(float al, float u, float T, bool hard, float* dcda) {
    if (hard) { *dcda = 0.f; return u < al ? 1.f : 0.f; }
    const float p = fminf(fmaxf(al, kProbEps), 1.f - kProbEps);
    const float uc = fminf(fmaxf(u, kProbEps), 1.f - kProbEps);
    const float z = (((logf(uc) - log1pf(-uc)) + logf(p)) - log1pf(-p)) / T;
    const float s = 1.f / (1.f + expf(-z));
    const float c = fminf(fmaxf(s, kTiny), 1.f - kProbEps);
    const bool in = (al >= kProbEps && al <= 1.f - kProbEps) && (s >= kTiny && s <= 1.f - kProbEps);
    *dcda = in ? (c * (1.f - c)) / (T * (p * (1.f - p))) : 0.f;
    return c;
}

// ------------------------------------------------------------------------------------------------ index rules
// the layer of this workgroup from the prefix ends (Batch::wg_end, Batch::n) of the layers' workgroup ranges on gridDim.x
template <typename Batch>
__device__ __forceinline__ int layer_of(const LBBNN_CONST_AS Batch* bt, int& wg0) {
    int li = 0;
#pragma unroll
    for (int t = 0; t < LBBNN_MAX_LAYERS - 1; ++t) if (t + 1 < bt->n && (int)blockIdx.x >= bt->wg_end[t]) li = t + 1;
    wg0 = li ? bt->wg_end[li - 1] : 0;
    return li;
}
// an index of a compact map as the kernels use it: inside [0, n) whatever the array holds (the host side builds them in
// range).  map_index: no map (NULL) is the identity; a kernel that only exists with a map calls clamped_index.
__device__ __forceinline__ int clamped_index(const int32_t* idx, int k, int n) {
    const int v = idx[k];
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}
__device__ __forceinline__ int map_index(const int32_t* idx, int k, int n) { return idx ? clamped_index(idx, k, n) : k; }

}  // namespace lbbnn
