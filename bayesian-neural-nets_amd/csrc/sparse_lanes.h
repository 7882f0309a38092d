// What the sparse model's lane-per-batch-row kernels share (sparse_members.hip, sparse_explain.hip): the rows of a lane as one
// value, and the wave-uniform index helpers.
#pragma once
#include "lbbnn_device.h"

namespace lbbnn {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// kR batch rows of a lane as one value: the two-row form loads them as one 8-B word and does its FMAs as packed fp32
// (v_pk_fma_f32: IEEE per component, so a row's bits are those of the one-row form)
typedef float sp_f2 __attribute__((ext_vector_type(2)));
template <int kR> struct SpRows;
template <> struct SpRows<1> {
    typedef float T;
    static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
    }
    static __device__ __forceinline__ T splat(float v) { return v; }
    static __device__ __forceinline__ T fma(float w, T x, T acc) { return __builtin_fmaf(w, x, acc); }
    static __device__ __forceinline__ float get(T v, int) { return v; }
};
template <> struct SpRows<2> {
    typedef sp_f2 T;
    static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
        return __builtin_bit_cast(sp_f2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
    }
    static __device__ __forceinline__ T splat(float v) { return sp_f2{v, v}; }
    static __device__ __forceinline__ T fma(float w, T x, T acc) { return __builtin_elementwise_fma(sp_f2{w, w}, x, acc); }
    static __device__ __forceinline__ float get(T v, int i) { return i ? v.y : v.x; }
};

}  // namespace lbbnn
