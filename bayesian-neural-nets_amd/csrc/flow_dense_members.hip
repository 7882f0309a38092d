// K4m  lbbnn_flow_dense_members -- the z of every MEMBER of an evaluation ensemble and every MNF layer through a dense
// coupling flow (RNVP / MNF type, flows2.py:188-241) in ONE launch: what `members` consecutive single forwards compute in
// 1 + T launches each (flow_dense.hip), with every coupling matrix read once per 16 members instead of once per member.
//
// Structure of K4r (flow_dense_rows.hip), the members taking the place of its rows: one 512-thread workgroup carries up to
// 16 members of one layer through the whole chain, the members being the 16 columns of v_mfma_f32_16x16x4_f32 (exact
// fp32); z lives in LDS for all T transforms in K4r's swizzled chunk-major image.  Grid = (ceil(members / 16), layers).
// Per transform, as K4r:
//   A  hidden pre-activation  P (H x 16) = W_in (H x I) . (m (.) z)^T        K = I split over the 8 waves, summed in LDS
//   B  RNVP only: three H x H layers, n-blocks over the waves
//   C  heads S_a, S_b (I x 16) = W_a / W_b (I x H) . y, n-blocks over the waves; gate and update in the epilogue, z
//      updated in place in LDS.  No log-determinant: evaluation draws no KL.
// What differs from K4r: nothing is read for z0 or the masks.  Member m draws from {seed, offset} = {rng[0], rng[1] +
// m * member_advance} exactly what the single forward at that offset draws (dense_init_kernel, flow_dense.hip):
//   eps_i  = philox_normal4(stream EPS_Z * 64 + layer, counter (i / 4, 0))[i % 4],  z0_i = q0_mean_i + exp(q0_log_var_i)^.5 eps_i
//   mask of transform t at i = bit t of word x of philox_bits4(stream MASK * 64 + layer, counter (i, 0))
// Wave w, lane (member lr, quarter q) owns elements 16c + 4q .. + 3 of member lr for the chunks c = w, w + 8, ... in EVERY
// stage, so it draws them itself: z0 into the z image, and the T mask bits of its four elements as the four bytes of one
// LDS word (MW[c][lane]: lane-contiguous, conflict-free) -- one Philox call per element for the whole chain.
// Deterministic: every sum has a fixed order; no atomics.  The result of a member does not depend on the member count or
// on which group of 16 it falls in (columns of an MFMA are independent), so chunked ensembles give the same bits.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"

namespace lbbnn {
namespace {

typedef float mf4 __attribute__((ext_vector_type(4)));

struct MemTransform {                      // lbbnn_dense_transform_t without the mask vectors (kernarg space: 4 layers x 8)
    int kind, hidden;
    const float *w_in, *b_in, *w_mid[3], *b_mid[3], *w_a, *b_a, *w_b, *b_b;
};
struct MemLayer {
    MemTransform tr[LBBNN_MAX_DENSE_T];
    const float *q0_mean, *q0_log_var;
    float* z_fwd;
    float* mask_out;                       // NULL, or [members][T][I]
    long long z_ms;
    int T, I;
    uint32_t layer;
    int pad_;
};
struct MemBatch {
    MemLayer l[LBBNN_MAX_LAYERS];
    const uint64_t* rng;
    uint64_t adv;
    int members;
};
static_assert(sizeof(MemBatch) <= 4096, "kernel arguments");

constexpr int kCols = 16;                              // members per workgroup
constexpr int kWaves = 8;                              // waves per workgroup (one workgroup per CU: LDS)
constexpr int kThreads = 64 * kWaves;
constexpr int kNB = LBBNN_MAX_HIDDEN / 16;             // hidden n-blocks (H <= 128)
constexpr int kHS = LBBNN_MAX_HIDDEN + 8;              // row stride of the hidden matrices in LDS

__device__ __forceinline__ int m_swz(int col) { return (0x78 >> (2 * ((col >> 2) & 3))) & 3; }   // F = {0,2,3,1}, as K4r

// 4 consecutive elements W[row][k..k+3] of a row-major (nrows x K) matrix; zero outside
__device__ __forceinline__ mf4 m_load_w4(const float* __restrict__ W, int row, int nrows, int k, int K) {
    mf4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= nrows) return v;
    const float* p = W + (size_t)row * K + k;
    if (k + 3 < K && ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) return *reinterpret_cast<const mf4*>(p);
    if (k < K) v.x = p[0];
    if (k + 1 < K) v.y = p[1];
    if (k + 2 < K) v.z = p[2];
    if (k + 3 < K) v.w = p[3];
    return v;
}
__device__ __forceinline__ mf4 m_load_vec4(const float* __restrict__ v, int k, int K) { return m_load_w4(v, 0, 1, k, K); }

__device__ __forceinline__ mf4 m_mfma4(mf4 a, mf4 b, mf4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// the masks of transform t for the four elements whose bits are the bytes of `mw`
__device__ __forceinline__ mf4 m_mask4(uint32_t mw, int t) {
    const uint32_t b = mw >> t;
    return mf4{(float)(b & 1u), (float)((b >> 8) & 1u), (float)((b >> 16) & 1u), (float)((b >> 24) & 1u)};
}

__device__ __forceinline__ mf4 m_leaky(mf4 s) {                       // LeakyReLU(0.1)  (flows2.py:176-185)
    s.x = s.x > 0.f ? s.x : 0.1f * s.x; s.y = s.y > 0.f ? s.y : 0.1f * s.y;
    s.z = s.z > 0.f ? s.z : 0.1f * s.z; s.w = s.w > 0.f ? s.w : 0.1f * s.w;
    return s;
}

__global__ __launch_bounds__(kThreads) void flow_dense_members_kernel(MemBatch bt_) {
    const LBBNN_CONST_AS MemBatch* bt = kernarg_as<MemBatch>();
    const LBBNN_CONST_AS MemLayer& a = bt->l[blockIdx.y];
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, q = lane >> 4;                 // member of the group / k quarter (operands), feature quad (results)
    const int I = a.I, T = a.T;
    const int C = (I + 15) >> 4;                             // 16-float chunks of a z vector
    const int mem = blockIdx.x * kCols + lr;
    const bool live = mem < bt->members;
    // LDS carve-up
    float* Z = lds;                                          // [C][16 members][16]  (swizzled slots)
    uint32_t* MW = reinterpret_cast<uint32_t*>(Z + (size_t)C * 256);   // [C][64 lanes]: mask bits, byte j = element j of the quad
    float* H0 = reinterpret_cast<float*>(MW + (size_t)C * 64);         // [16][kHS]
    float* H1 = H0 + kCols * kHS;
    float* part = H1 + kCols * kHS;                          // [4][kNB][64][4]: waves w and w + 4 share slot w
    const int zslot = lr * 16 + ((q ^ m_swz(lr)) << 2);      // this lane's quad inside a chunk of the z image

    // ---- the draws: z0 and the mask bits of this lane's own elements (columns past the last member: zeros)
    {
        const uint64_t seed = bt->rng[0], off = bt->rng[1] + (uint64_t)mem * bt->adv;
        const uint32_t s_eps = LBBNN_STREAM_EPS_Z * 64u + a.layer, s_mask = LBBNN_STREAM_MASK * 64u + a.layer;
        float* mout = a.mask_out;
        for (int c = w; c < C; c += kWaves) {
            const int i = 16 * c + 4 * q;                    // I % 4 == 0: a quad is wholly inside or outside the vector
            mf4 z = {0.f, 0.f, 0.f, 0.f};
            uint32_t mw = 0;
            if (live && i < I) {
                float e[4];
                philox_normal4(seed, off, s_eps, (uint64_t)(i >> 2), 0u, e);
                const mf4 qm = m_load_vec4(a.q0_mean, i, I), lv = m_load_vec4(a.q0_log_var, i, I);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float ev = expf(lv[j]);
                    z[j] = qm[j] + sqrtf(ev) * e[j];         // the expression of dense_init_kernel (LBBNN-GP-MF-MNF.py:183-185)
                    const Philox4 b = philox_bits4(seed, off, s_mask, (uint64_t)(i + j), 0u);
                    mw |= (b.x & 0xFFu) << (8 * j);          // bit t = transform t (T <= 8), the forward-draw word
                }
                if (mout != nullptr) {
                    for (int t = 0; t < T; ++t) {
                        const mf4 m = m_mask4(mw, t);
                        float* mp = mout + ((size_t)mem * T + t) * I + i;
                        mp[0] = m.x; mp[1] = m.y; mp[2] = m.z; mp[3] = m.w;
                    }
                }
            }
            *reinterpret_cast<mf4*>(Z + c * 256 + zslot) = z;
            MW[c * 64 + lane] = mw;
        }
    }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const int kind = a.tr[t].kind, H = a.tr[t].hidden;
        const int NB = (H + 15) >> 4;                         // hidden n-blocks
        // ------------------------------------------------------------------ A: input layer, K = I split over the waves
        {
            const float* W = a.tr[t].w_in;
            mf4 acc[kNB];
#pragma unroll
            for (int nb = 0; nb < kNB; ++nb) acc[nb] = mf4{0.f, 0.f, 0.f, 0.f};
            // every weight quad of a chunk is loaded before its first MFMA: the matrices stream through ONE CU per layer when
            // members <= 16, and the loads in flight are what bounds that stream
            for (int c = w; c < C; c += kWaves) {
                mf4 wv[kNB];
#pragma unroll
                for (int nb = 0; nb < kNB; ++nb)
                    if (nb < NB) wv[nb] = m_load_w4(W, 16 * nb + lr, H, 16 * c + 4 * q, I);
                const mf4 mz = m_mask4(MW[c * 64 + lane], t) * *reinterpret_cast<const mf4*>(Z + c * 256 + zslot);
#pragma unroll
                for (int nb = 0; nb < kNB; ++nb)
                    if (nb < NB) acc[nb] = m_mfma4(wv[nb], mz, acc[nb]);
            }
            // waves 4..7 hand their partials to waves 0..3 (fixed order), which add their own: four slots, as K4r
            if (w >= 4) {
#pragma unroll
                for (int nb = 0; nb < kNB; ++nb)
                    if (nb < NB) *reinterpret_cast<mf4*>(part + (((w - 4) * kNB + nb) * 64 + lane) * 4) = acc[nb];
            }
            __syncthreads();
            if (w < 4) {
#pragma unroll
                for (int nb = 0; nb < kNB; ++nb) {
                    if (nb < NB) {
                        mf4* pp = reinterpret_cast<mf4*>(part + ((w * kNB + nb) * 64 + lane) * 4);
                        *pp = acc[nb] + *pp;
                    }
                }
            }
            __syncthreads();
            const float* bias = a.tr[t].b_in;
            for (int u = tid; u < NB * 64; u += kThreads) {
                const int nb = u >> 6, ln = u & 63;
                mf4 s = *reinterpret_cast<const mf4*>(part + ((0 * kNB + nb) * 64 + ln) * 4);
                s += *reinterpret_cast<const mf4*>(part + ((1 * kNB + nb) * 64 + ln) * 4);
                s += *reinterpret_cast<const mf4*>(part + ((2 * kNB + nb) * 64 + ln) * 4);
                s += *reinterpret_cast<const mf4*>(part + ((3 * kNB + nb) * 64 + ln) * 4);
                const int n = 16 * nb + 4 * (ln >> 4);
                s += m_load_vec4(bias, n, H);
                if (kind == 0) s = m_leaky(s);                // RNVP
                else { s.x = tanhf(s.x); s.y = tanhf(s.y); s.z = tanhf(s.z); s.w = tanhf(s.w); }   // MNF type (flows2.py:235)
                *reinterpret_cast<mf4*>(H0 + (ln & 15) * kHS + n) = s;
            }
            __syncthreads();
        }
        float* Hin = H0;
        float* Hout = H1;
        // ------------------------------------------------------------------ B: RNVP middle layers (H x H)
        if (kind == 0) {
            for (int l = 0; l < 3; ++l) {
                const float* W = a.tr[t].w_mid[l];
                const float* bias = a.tr[t].b_mid[l];
                for (int nb = w; nb < NB; nb += kWaves) {
                    mf4 acc = {0.f, 0.f, 0.f, 0.f};
                    mf4 wv[kNB];                              // the whole weight row block in flight before the first MFMA
#pragma unroll
                    for (int c = 0; c < kNB; ++c)
                        if (c < NB) wv[c] = m_load_w4(W, 16 * nb + lr, H, 16 * c + 4 * q, H);
#pragma unroll
                    for (int c = 0; c < kNB; ++c) {
                        if (c < NB) {
                            const mf4 hv = *reinterpret_cast<const mf4*>(Hin + lr * kHS + 16 * c + 4 * q);
                            acc = m_mfma4(wv[c], hv, acc);
                        }
                    }
                    const int n = 16 * nb + 4 * q;
                    acc += m_load_vec4(bias, n, H);
                    if (l < 2) acc = m_leaky(acc);            // the last activation of the MLP is dropped (flows2.py:184)
                    // features >= H stay exactly zero (zero weight rows, zero bias): they are the K padding of the next layer
                    *reinterpret_cast<mf4*>(Hout + lr * kHS + n) = acc;
                }
                __syncthreads();
                float* tmp = Hin; Hin = Hout; Hout = tmp;
            }
        }
        // ------------------------------------------------------------------ C: heads + gate + update, n-blocks of I over the waves
        {
            const float* Wa = a.tr[t].w_a;
            const float* Wb = a.tr[t].w_b;
            const float* ba = a.tr[t].b_a;
            const float* bb = a.tr[t].b_b;
            for (int nb = w; nb < C; nb += kWaves) {
                mf4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
                for (int c0 = 0; c0 < NB; c0 += 4) {          // four k-blocks of both heads in flight before their MFMAs
                    mf4 wa[4], wb[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        wa[c] = m_load_w4(Wa, 16 * nb + lr, I, 16 * (c0 + c) + 4 * q, H);    // (zero past H)
                        wb[c] = m_load_w4(Wb, 16 * nb + lr, I, 16 * (c0 + c) + 4 * q, H);
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (c0 + c < NB) {
                            const mf4 hv = *reinterpret_cast<const mf4*>(Hin + lr * kHS + 16 * (c0 + c) + 4 * q);
                            sa = m_mfma4(wa[c], hv, sa);
                            sb = m_mfma4(wb[c], hv, sb);
                        }
                    }
                }
                const int i = 16 * nb + 4 * q;               // this lane: features i..i+3 of member lr
                sa += m_load_vec4(ba, i, I);
                sb += m_load_vec4(bb, i, I);
                float* zp = Z + nb * 256 + zslot;
                const mf4 z = *reinterpret_cast<const mf4*>(zp);
                const mf4 m = m_mask4(MW[nb * 64 + lane], t);
                mf4 x;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gate = 1.0f / (1.0f + expf(-sb[j]));          // sigmoid(scale) / sigmoid(k(h))
                    const float keep = m[j] * z[j], move = (1.f - m[j]) * z[j];
                    // RNVP  (flows2.py:211-215): x = z1*gate + (1-gate)*shift + z2,  z1 = (1-m) z, z2 = m z
                    // MNF   (flows2.py:238):     x = m z + (1-m) (z sigma + (1-sigma) mu)
                    x[j] = (kind == 0) ? (move * gate + (1.f - gate) * sa[j]) + keep
                                       : keep + (1.f - m[j]) * (z[j] * gate + (1.f - gate) * sa[j]);
                }
                if (!live || i >= I) x = mf4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<mf4*>(zp) = x;
            }
            __syncthreads();
        }
    }
    // ---- member m's z to z_fwd + m * z_mstride (16-B stores: z_fwd aligned, z_mstride % 4 == 0, I % 4 == 0)
    if (live) {
        float* zo = a.z_fwd + (size_t)mem * (size_t)a.z_ms;
        for (int c = w; c < C; c += kWaves) {
            const int i = 16 * c + 4 * q;
            if (i < I) *reinterpret_cast<mf4*>(zo + i) = *reinterpret_cast<const mf4*>(Z + c * 256 + zslot);
        }
    }
}

size_t members_lds_bytes(int I) {
    const size_t C = (size_t)(I + 15) / 16;
    return 4 * (C * 256 + C * 64 + 2 * kCols * kHS + 4 * kNB * 256);
}
constexpr size_t kMembersLdsMax = 160 * 1024;

}  // namespace
}  // namespace lbbnn

extern "C" int lbbnn_flow_dense_members_max_dim(void) {
    int I = 16;
    while (lbbnn::members_lds_bytes(I + 16) <= lbbnn::kMembersLdsMax) I += 16;
    return I;
}

extern "C" int lbbnn_flow_dense_members(const lbbnn_dense_members_t* L, int n, int members, const uint64_t* rng,
                                        uint64_t member_advance, void* stream) {
    using namespace lbbnn;
    if (L == nullptr) return LBBNN_E_NULL;
    if (n <= 0 || n > LBBNN_MAX_LAYERS || members < 1 || members > 65535) return LBBNN_E_SHAPE;
    const int max_dim = lbbnn_flow_dense_members_max_dim();
    MemBatch bt = {};
    int max_I = 0;
    for (int i = 0; i < n; ++i) {
        const lbbnn_dense_members_t& d = L[i];
        if (!d.q0_mean || !d.q0_log_var || !d.z_fwd) return LBBNN_E_NULL;
        if (d.T < 0 || d.T > LBBNN_MAX_DENSE_T) return LBBNN_E_SHAPE;
        if (d.T > 0 && !d.zt) return LBBNN_E_NULL;
        MemLayer& a = bt.l[i];
        for (int t = 0; t < d.T; ++t) {
            const lbbnn_dense_transform_t& s = d.zt[t];
            if (!s.w_in || !s.b_in || !s.w_a || !s.b_a || !s.w_b || !s.b_b) return LBBNN_E_NULL;
            if (s.kind == LBBNN_FLOW_RNVP)
                for (int l = 0; l < 3; ++l) if (!s.w_mid[l] || !s.b_mid[l]) return LBBNN_E_NULL;
            MemTransform& m = a.tr[t];
            m.kind = s.kind; m.hidden = s.hidden; m.w_in = s.w_in; m.b_in = s.b_in;
            for (int l = 0; l < 3; ++l) { m.w_mid[l] = s.w_mid[l]; m.b_mid[l] = s.b_mid[l]; }
            m.w_a = s.w_a; m.b_a = s.b_a; m.w_b = s.w_b; m.b_b = s.b_b;
        }
        if (!rng) return LBBNN_E_NOISE;
        if (d.I < 1 || d.I > max_dim || d.z_mstride < d.I) return LBBNN_E_SHAPE;
        for (int t = 0; t < d.T; ++t) {
            const lbbnn_dense_transform_t& s = d.zt[t];
            if (s.hidden < 1 || s.hidden > LBBNN_MAX_HIDDEN) return LBBNN_E_SHAPE;
            if ((s.kind != LBBNN_FLOW_RNVP && s.kind != LBBNN_FLOW_MNF) || s.kind != d.zt[0].kind) return LBBNN_E_SHAPE;
        }
        if ((d.I & 3) || (d.z_mstride & 3) || (reinterpret_cast<uintptr_t>(d.z_fwd) & 15u)) return LBBNN_E_ALIGN;
        a.q0_mean = d.q0_mean; a.q0_log_var = d.q0_log_var; a.z_fwd = d.z_fwd; a.mask_out = d.mask_out;
        a.z_ms = (long long)d.z_mstride; a.T = d.T; a.I = d.I; a.layer = d.layer_id & 63u;
        max_I = d.I > max_I ? d.I : max_I;
    }
    bt.rng = rng; bt.adv = member_advance; bt.members = members;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(flow_dense_members_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMembersLdsMax);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    hipLaunchKernelGGL(flow_dense_members_kernel, dim3((members + kCols - 1) / kCols, n), dim3(kThreads), members_lds_bytes(max_I),
                       (hipStream_t)stream, bt);
    return (int)hipGetLastError();
}
