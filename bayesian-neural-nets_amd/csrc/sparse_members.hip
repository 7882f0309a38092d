// Sparse median-probability model (gfx950): the kept weights of a frozen LRT / MNF network in CSR, and the member layers
// evaluated on the vector ALU from that format alone, see include/lbbnn.h.
//
//   csr_rows_kernel<LrtRule> (csr_pack.h) -- lbbnn_sparse_count / _pack and lbbnn_sparse_count_levels / _pack_levels: one wave per
//     weight row, the ballot of `lambdal > cut` and the count of the kept lanes below give each kept weight its slot.
//   sparse_layer_kernel -- lbbnn_sparse_layer_members: ONE LANE PER BATCH ROW, WEIGHTS WAVE-UNIFORM.  A wave owns 64 rows of
//     one member (blockIdx.y: the row tile, blockIdx.z: the member, so z_m[col] is uniform) and four consecutive output
//     units, one philox_normal4 call per lane as in the dense epilogue.  It walks the CSR row of each unit once: col / mean /
//     var (and z[col]) are the same for all lanes -- scalar loads, eight nonzeros a batch -- and a lane does two FMAs per
//     nonzero on its own row's activation, which it loads from the transposed buffer a[col][b]: one contiguous 256-B line
//     per wave and nonzero.  The four waves of a workgroup take the same row tile and neighbouring unit groups, so they
//     read the same activation lines.  No cross-lane step: the sums are sequential in CSR order by construction.  The only
//     LDS is the <= 16-unit head's: its four waves exchange the tile's logits for the log_softmax.  Two batch rows per lane
//     (tiles of 128 rows, 8-B loads, packed fp32 FMAs) halve the scalar work per row, which is what bounds the loop.
#include <cstdlib>
#include "csr_pack.h"

namespace {

using namespace lbbnn;

constexpr int kSpChunk = 8;                // nonzeros whose activation loads are in flight together

// lbbnn_sparse_count / _pack (K = 1, the single-level kernel) and the threshold sweep's lbbnn_sparse_count_levels / _pack_levels:
// csr_pack.h's kernel under LrtRule.  K = 0 tells csr_rows that the levels or the cuts are out of range.
template <int kMaxLevels, typename Desc>
void sparse_copy(const Desc& d, CsrLayer<kMaxLevels>& a, int K) {
    a.mu = d.weight_mu; a.rho = d.weight_rho; a.lambdal = d.lambdal; a.bias_rho = d.bias_rho;
    a.row_ptr = d.row_ptr; a.col = d.col; a.mean = d.mean; a.val = d.var; a.row0 = d.bias_var; a.kept_rows = d.kept_rows;
    a.O = d.O; a.I = d.I; a.nnz = d.nnz; a.K = K;
}

int sparse_rows(const lbbnn_sparse_desc_t* L, int n, bool pack, void* stream) {
    return csr_rows<LrtRule, 1>(L, n, pack, 0, stream, [](const lbbnn_sparse_desc_t& d, CsrLayer<1>& a) {
        sparse_copy(d, a, 1);
        a.cut[0] = d.cut;
    });
}

int sparse_levels(const lbbnn_sparse_levels_desc_t* L, int n, bool pack, void* stream) {
    return csr_rows<LrtRule, LBBNN_MAX_LEVELS>(L, n, pack, 0, stream, [](const lbbnn_sparse_levels_desc_t& d, CsrLayer<LBBNN_MAX_LEVELS>& a) {
        bool ok = d.levels >= 1 && d.levels <= LBBNN_MAX_LEVELS;
        for (int j = 0; ok && j < d.levels; ++j) {    // finite and strictly ascending (a NaN fails `< INFINITY`)
            ok = fabsf(d.cut[j]) < INFINITY && (!j || d.cut[j - 1] < d.cut[j]);
            a.cut[j] = d.cut[j];
        }
        sparse_copy(d, a, ok ? d.levels : 0);
    });
}

struct SpArgs {
    const int32_t* row_ptr; const int32_t* col; const float* mean; const float* var;
    const float* bias_mu; const float* bias_var;
    const float* a; long long a_ms; int lda; int a_bytes;     // a_bytes: what a member's block of `a` spans
    const float* z; long long z_ms;
    const uint64_t* rng; uint32_t rng_stream; long long row_offset; unsigned long long m_adv;
    float* out; long long o_ms; int ldo;
    int B, I, O, nnz, relu, lsm, out_rows;
    int S;                                                    // kLv: members (draws) per level
};

// One nonzero of a unit's CSR row for the lane's rows: the column index is taken inside [0, I) whatever the array holds
// (one unsigned minimum), the weights are wave-uniform, the activation line is a buffer load at a scalar offset
#define LBBNN_SP_LOAD(t, k)                                                         \
    do {                                                                            \
        const unsigned c = min((unsigned)a.col[k], imax);                           \
        w[t] = a.mean[k];                                                           \
        v[t] = kMeanOnly ? 0.f : a.var[k];                                          \
        if (kZ) w[t] *= z[c];               /* (mu * a) * z_k, K1's order of products */ \
        x[t] = R::load(act, boff, c * lda4);                                        \
    } while (0)
#define LBBNN_SP_FMA(t)                                                             \
    do {                                                                            \
        am[r] = R::fma(w[t], x[t], am[r]);                                          \
        if (!kMeanOnly) av[r] = R::fma(v[t], x[t] * x[t], av[r]);                   \
    } while (0)

// kR: batch rows per lane (1: tiles of 64 rows; 2: tiles of 128, lane l owns rows 2l and 2l + 1 of the tile).  The four waves
// of a workgroup take the same row tile and four neighbouring unit groups; a <= 16-unit head with log_softmax is one
// workgroup per tile, and its waves hand each other the tile's logits through LDS.
// kLv: a threshold sweep's launch (lbbnn_sparse_layer_levels) -- member blockIdx.z is level lv = z / S under draw dr = z % S:
// the level picks the row pointers (row_ptr + lv * O), the draw picks z and the Philox offset; both come from blockIdx.z and a
// kernel argument alone, so they live in scalar registers and everything indexed by them stays a scalar load.  !kLv: lv = 0,
// dr = the member -- the plain kernel, instruction for instruction.
template <bool kMeanOnly, bool kZ, int kR, bool kLv>
__global__ __launch_bounds__(256) void sparse_layer_kernel(const SpArgs a) {
#pragma clang fp contract(off)
    typedef SpRows<kR> R;
    typedef typename R::T rows_t;
    __shared__ float logits[16][64 * kR];
    const int lane = threadIdx.x & 63, wv = uniform(threadIdx.x >> 6);
    const int mem = blockIdx.z;
    const int lv = kLv ? mem / a.S : 0, dr = kLv ? mem - lv * a.S : mem;
    const int32_t* row_ptr = a.row_ptr + (size_t)lv * a.O;
    const int b = ((int)blockIdx.y * 64 + lane) * kR;                     // the lane's first row
    const bool live = b < a.B;
    // a lane past the batch computes rows 0 .. kR - 1 again (in bounds, never stored): no lane-dependent branch in the loop.
    // A load is a buffer load of the member's block: the lane's byte offset in a register that never changes, the line
    // (col * lda * 4) as the scalar offset -- no vector instruction for an address, and a range check in hardware
    const __amdgpu_buffer_rsrc_t act = __builtin_amdgcn_make_buffer_rsrc((void*)(a.a + (size_t)mem * a.a_ms), 0, a.a_bytes, 0x00020000);
    const unsigned lda4 = 4u * (unsigned)a.lda, imax = (unsigned)a.I - 1u;
    const unsigned boff = live ? 4u * (unsigned)b : 0u;
    const float* z = kZ ? a.z + (size_t)dr * a.z_ms : nullptr;
    uint64_t seed = 0, offs = 0;
    if (!kMeanOnly) { seed = a.rng[0]; offs = a.rng[1] + (uint64_t)dr * a.m_adv; }
    const int o0 = 4 * ((int)blockIdx.x * 4 + wv);
    const bool any = o0 < a.O;                                            // wave-uniform
    float res[kR][4];
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) res[i][r] = 0.f;
    if (any) {
        rows_t am[4], av[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            am[r] = R::splat(0.f); av[r] = R::splat(0.f);
            const int o = o0 + r;
            if (o >= a.O) continue;                                       // wave-uniform
            const int k0 = uniform(clampi(row_ptr[o], 0, a.nnz));
            const int k1 = uniform(clampi(row_ptr[o + 1], k0, a.nnz));
            int k = k0;
            rows_t x[kSpChunk];
            float w[kSpChunk], v[kSpChunk];
            for (; k + kSpChunk <= k1; k += kSpChunk) {
#pragma unroll
                for (int t = 0; t < kSpChunk; ++t) LBBNN_SP_LOAD(t, k + t);
#pragma unroll
                for (int t = 0; t < kSpChunk; ++t) LBBNN_SP_FMA(t);
            }
            const int rem = k1 - k;                                       // the last, partial batch: its loads in flight together too
            if (rem > 0) {
#pragma unroll
                for (int t = 0; t < kSpChunk - 1; ++t) if (t < rem) LBBNN_SP_LOAD(t, k + t);
#pragma unroll
                for (int t = 0; t < kSpChunk - 1; ++t) if (t < rem) LBBNN_SP_FMA(t);
            }
        }
        // the local-reparameterisation epilogue of the dense GEMMs (LBBNN-GP-MF-LRT.py:172-175) at the same counters
#pragma unroll
        for (int i = 0; i < kR; ++i) {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if (!kMeanOnly) philox_normal4(seed, offs, a.rng_stream, (uint64_t)(a.row_offset + b + i), (uint32_t)(o0 >> 2), e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = o0 + r;
                if (o >= a.O) continue;
                float mean = R::get(am[r], i) + a.bias_mu[o];
                if (!kMeanOnly) mean = __builtin_fmaf(sqrt_hw(R::get(av[r], i) + a.bias_var[o]), e[r], mean);
                res[i][r] = a.relu ? fmaxf(mean, 0.f) : mean;
            }
        }
    }
    if (a.lsm) {                                                          // (every wave of the one workgroup of the tile gets here)
        // log_softmax over the row (LBBNN-GP-MF-LRT.py:210): the tile's logits through LDS, every lane sums its rows in unit order
#pragma unroll
        for (int i = 0; i < kR; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) logits[4 * wv + r][kR * lane + i] = res[i][r];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kR; ++i) {
            float mx = -INFINITY;
            for (int j = 0; j < a.O; ++j) mx = fmaxf(mx, logits[j][kR * lane + i]);
            float se = 0.f;
            for (int j = 0; j < a.O; ++j) se += expf(logits[j][kR * lane + i] - mx);
            const float lse = mx + logf(se);
#pragma unroll
            for (int r = 0; r < 4; ++r) res[i][r] -= lse;
        }
    }
    if (!live || !any) return;
    float* out = a.out + (size_t)mem * a.o_ms;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + r;
        if (o >= a.O) continue;
        if (kR == 2 && !a.out_rows && b + 1 < a.B) {                      // both rows of the lane: one 8-B store
            *reinterpret_cast<sp_f2*>(out + (size_t)o * a.ldo + b) = sp_f2{res[0][r], res[kR - 1][r]};
            continue;
        }
#pragma unroll
        for (int i = 0; i < kR; ++i) {
            if (b + i >= a.B) continue;
            if (a.out_rows) out[(size_t)(b + i) * a.ldo + o] = res[i][r];
            else out[(size_t)o * a.ldo + b + i] = res[i][r];
        }
    }
}
#undef LBBNN_SP_LOAD
#undef LBBNN_SP_FMA

// rows per lane: LBBNN_SPARSE_ROWS = 1 | 2 overrides the choice (a knob for A/B timing; both forms give the same bits)
int sparse_rows_per_lane(const SpArgs& a) {
    static const char* env = getenv("LBBNN_SPARSE_ROWS");
    // the two-row form reads and writes 8-B words: even strides on 8-B boundaries, and a row B (odd B) that exists
    const bool can2 = !off(a.a, 8) && !(a.lda & 1) && !(a.a_ms & 1) && a.lda >= a.B + (a.B & 1) &&
                      (a.out_rows || (!off(a.out, 8) && !(a.ldo & 1) && !(a.o_ms & 1)));
    if (!can2) return 1;
    if (env && env[0] == '1') return 1;
    if (env && env[0] == '2') return 2;
    return a.B > 64 ? 2 : 1;
}

template <bool kMeanOnly, bool kZ, bool kLv>
void launch_sparse_layer(const SpArgs& a, int members, hipStream_t s) {
    const dim3 block(256);
    const unsigned groups = (unsigned)((a.O + 15) / 16);                  // (1 with log_softmax: O <= 16)
    if (sparse_rows_per_lane(a) == 2)
        hipLaunchKernelGGL((sparse_layer_kernel<kMeanOnly, kZ, 2, kLv>), dim3(groups, (unsigned)((a.B + 127) / 128), members), block, 0, s, a);
    else
        hipLaunchKernelGGL((sparse_layer_kernel<kMeanOnly, kZ, 1, kLv>), dim3(groups, (unsigned)((a.B + 63) / 64), members), block, 0, s, a);
}

// Both layer entry points.  !lv: lbbnn_sparse_layer_members, `per_level` members of the one model (levels = 1); lv:
// lbbnn_sparse_layer_levels, levels * per_level members of which `per_level` differ in their draws.
int sparse_layer_impl(const int32_t* row_ptr, const int32_t* col, const float* mean, const float* var, int nnz,
                      const float* bias_mu, const float* bias_var, const float* a, int lda, int64_t a_mstride, const float* z,
                      int64_t z_mstride, const uint64_t* rng, uint32_t rng_stream, int64_t row_offset, uint64_t member_advance,
                      float* out, int ldo, int64_t o_mstride, int out_rows, int B, int I, int O, int flags, bool lv,
                      int levels, int per_level, void* stream) {
    if (B == 0) return 0;
    if (!row_ptr || !bias_mu || !bias_var || !a || !out) return LBBNN_E_NULL;
    if (nnz > 0 && (!col || !mean || !var)) return LBBNN_E_NULL;
    if (levels < 1 || levels > LBBNN_MAX_LEVELS) return LBBNN_E_SHAPE;
    if (per_level < 1 || per_level > 65535) return LBBNN_E_SHAPE;
    const int members = levels * per_level;                    // (at most 16 * 65535: no overflow)
    if (B < 0 || (long long)B > 65535LL * 64 || I <= 0 || O <= 0 || nnz < 0 || members > 65535) return LBBNN_E_SHAPE;
    if (lda < B || ldo < (out_rows ? O : B) || a_mstride < 0 || z_mstride < 0 || o_mstride < 0) return LBBNN_E_SHAPE;
    // the kernel addresses a member's input as a buffer: I lines of B rows -- of B + 1 where lda has room for the pair of an
    // odd last row (the two-row form reads it and drops it)
    const long long a_bytes = 4 * ((long long)(I - 1) * lda + B + ((B & 1) && lda > B ? 1 : 0));
    if (a_bytes > 0x7FFFFFF0LL) return LBBNN_E_SHAPE;
    if (members > 1) {
        // members may share an input (a_mstride == 0: the first layer's x^T), never an output
        const long long need = out_rows ? (long long)(B - 1) * ldo + O : (long long)(O - 1) * ldo + B;
        if (o_mstride < need || (a_mstride && a_mstride < (long long)(I - 1) * lda + B)) return LBBNN_E_SHAPE;
    }
    if (per_level > 1 && z && z_mstride < I) return LBBNN_E_SHAPE;         // (the levels of one draw share its z)
    const bool mean_only = (flags & LBBNN_F_MEAN_ONLY) != 0, lsm = (flags & LBBNN_F_LOG_SOFTMAX) != 0;
    if (flags & ~(LBBNN_F_RELU | LBBNN_F_MEAN_ONLY | LBBNN_F_LOG_SOFTMAX)) return LBBNN_E_FLAGS;
    if (lsm && (O > 16 || (flags & LBBNN_F_RELU) || !out_rows)) return LBBNN_E_FLAGS;
    if (!mean_only && !rng) return LBBNN_E_NOISE;
    if (!aligned4(row_ptr) || !aligned4(col) || !aligned4(mean) || !aligned4(var) || !aligned4(bias_mu) || !aligned4(bias_var) ||
        !aligned4(a) || !aligned4(z) || !aligned4(out) || off(rng, 8)) return LBBNN_E_ALIGN;
    SpArgs k = {};
    k.row_ptr = row_ptr; k.col = col; k.mean = mean; k.var = var; k.bias_mu = bias_mu; k.bias_var = bias_var;
    k.a = a; k.a_ms = a_mstride; k.lda = lda; k.a_bytes = (int)a_bytes; k.z = z; k.z_ms = z_mstride;
    k.rng = rng; k.rng_stream = rng_stream; k.row_offset = row_offset; k.m_adv = member_advance;
    k.out = out; k.o_ms = o_mstride; k.ldo = ldo;
    k.B = B; k.I = I; k.O = O; k.nnz = nnz; k.relu = (flags & LBBNN_F_RELU) ? 1 : 0; k.lsm = lsm ? 1 : 0; k.out_rows = out_rows ? 1 : 0;
    k.S = per_level;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int form = (mean_only ? 4 : 0) | (z ? 2 : 0) | (lv ? 1 : 0);
    switch (form) {
        case 0: launch_sparse_layer<false, false, false>(k, members, s); break;
        case 1: launch_sparse_layer<false, false, true>(k, members, s); break;
        case 2: launch_sparse_layer<false, true, false>(k, members, s); break;
        case 3: launch_sparse_layer<false, true, true>(k, members, s); break;
        case 4: launch_sparse_layer<true, false, false>(k, members, s); break;
        case 5: launch_sparse_layer<true, false, true>(k, members, s); break;
        case 6: launch_sparse_layer<true, true, false>(k, members, s); break;
        default: launch_sparse_layer<true, true, true>(k, members, s); break;
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int lbbnn_sparse_count(const lbbnn_sparse_desc_t* L, int n, void* stream) {
    return sparse_rows(L, n, false, stream);
}

extern "C" int lbbnn_sparse_pack(const lbbnn_sparse_desc_t* L, int n, void* stream) {
    return sparse_rows(L, n, true, stream);
}

extern "C" int lbbnn_sparse_count_levels(const lbbnn_sparse_levels_desc_t* L, int n, void* stream) {
    return sparse_levels(L, n, false, stream);
}

extern "C" int lbbnn_sparse_pack_levels(const lbbnn_sparse_levels_desc_t* L, int n, void* stream) {
    return sparse_levels(L, n, true, stream);
}

extern "C" int lbbnn_sparse_layer_members(const int32_t* row_ptr, const int32_t* col, const float* mean, const float* var,
                                          int nnz, const float* bias_mu, const float* bias_var, const float* a, int lda,
                                          int64_t a_mstride, const float* z, int64_t z_mstride, const uint64_t* rng,
                                          uint32_t rng_stream, int64_t row_offset, uint64_t member_advance, float* out,
                                          int ldo, int64_t o_mstride, int out_rows, int B, int I, int O, int flags,
                                          int members, void* stream) {
    return sparse_layer_impl(row_ptr, col, mean, var, nnz, bias_mu, bias_var, a, lda, a_mstride, z, z_mstride, rng, rng_stream,
                             row_offset, member_advance, out, ldo, o_mstride, out_rows, B, I, O, flags, false, 1, members, stream);
}

extern "C" int lbbnn_sparse_layer_levels(const int32_t* row_ptr, const int32_t* col, const float* mean, const float* var,
                                         int nnz, const float* bias_mu, const float* bias_var, const float* a, int lda,
                                         int64_t a_mstride, const float* z, int64_t z_mstride, const uint64_t* rng,
                                         uint32_t rng_stream, int64_t row_offset, uint64_t member_advance, float* out,
                                         int ldo, int64_t o_mstride, int out_rows, int B, int I, int O, int flags, int levels,
                                         int members_per_level, void* stream) {
    return sparse_layer_impl(row_ptr, col, mean, var, nnz, bias_mu, bias_var, a, lda, a_mstride, z, z_mstride, rng, rng_stream,
                             row_offset, member_advance, out, ldo, o_mstride, out_rows, B, I, O, flags, true, levels,
                             members_per_level, stream);
}

