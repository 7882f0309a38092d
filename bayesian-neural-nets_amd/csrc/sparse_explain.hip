// Explanations of sampled-weight members of the sparse median-probability model (gfx950), see include/lbbnn.h.
//
//   sparse_draw_kernel -- lbbnn_sparse_draw_members: one launch over the CSR slots and the biases of up to LBBNN_MAX_LAYERS
//     layers (blockIdx.x: the layer's quads, blockIdx.y: the member).  ONE THREAD PER QUAD: one philox_normal4 call, four
//     weights (or four biases), one 16-B store.  The member's z[col] is a gather; everything else is contiguous.
//   sparse_gather_kernel -- lbbnn_sparse_gather_members: sparse_layer_kernel's loop on STORED values.  One lane per batch row
//     (two when B > 64), four units per wave, the pattern (ptr / idx / slot) and the member's values wave-uniform scalar
//     loads, the input line a buffer load at a scalar offset, sequential FMAs in pattern order from 0.  The forward runs it on
//     row_ptr / col, the backward sweep on the transposed pattern col_ptr / trow with the values read through tslot: the
//     sweep's product G_l = W_{l+1}^T G_{l+1} is a member layer whose "weights" are the same (nnz,) vector in another order.
//     Three post-ops: + bias and ReLU (forward), the mask h_l > 0 (sweep), * x^T (finish).
//     The draw also stores every member's values column by column (through the inverse of tslot), so the sweep reads them in
//     pattern order like the forward; the slot form stays for values kept in CSR order alone.
//   explain_seed_kernel -- lbbnn_explain_seed: the explained output per row ("pred": the largest member-mean logit), the one-hot
//     seed G_L, the intercept's first term b_L and the advance of the live Philox offset, one launch.
//     Extra workgroups of a sweep launch add <G_l, b_l>, the bias path of the layer whose G is the launch's input, to the
//     intercept (gather_bias_dot): no launch of its own.
//   member_stats_kernel -- lbbnn_explain_member_stats: a 64 x 64 (feature x row) tile of every member
//     goes through LDS (rows of 65 floats: both sides conflict-free), so the transposed contributions are read in whole lines
//     and the row-major statistics written in whole lines; fp64 sums in member order, the deviations from sums shifted by the
//     first member.
// No atomics; the only exchange between lanes is the fixed-order add of four waves' partial sums in the bias dot and the
// residual: the bits of a number depend on its member, row and unit alone.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "operand_store.h"
#include "sparse_lanes.h"

namespace {

using namespace lbbnn;

constexpr int kDrawNT = 256;               // quads per workgroup of the draw kernel
constexpr int kGaChunk = 8;                // nonzeros whose input-line loads are in flight together
constexpr int kDotNT = 64;                 // batch rows (= lanes) per workgroup of the bias-dot and residual kernels
constexpr int kDotW = 4;                   // waves of the bias-dot workgroup: the units in quarters
constexpr int kDotChunk = 32;              // line loads in flight together there
constexpr int kTile = 64;                  // the statistics' tile: 64 features x 64 rows, 16 elements per thread

struct DrawLayer {
    const int32_t* col; const float* mean; const float* var; const float* bias_mu; const float* bias_var;
    const float* z; long long z_ms;
    const int32_t* tpos; float* wt;        // nullable pair: the weights once more, slot k at place tpos[k] (column by column)
    float* w; long long w_ms; float* b; long long b_ms;
    int O, I, nnz, nq;                     // nq: quads of weights; the layer's quads after them are its biases'
    uint32_t layer;
};
struct DrawBatch { DrawLayer l[LBBNN_MAX_LAYERS]; int wg_end[LBBNN_MAX_LAYERS]; int n; int mean_only; const uint64_t* rng; };

__global__ __launch_bounds__(kDrawNT) void sparse_draw_kernel(const DrawBatch bt_) {
#pragma clang fp contract(off)
    const LBBNN_CONST_AS DrawBatch* bt = kernarg_as<DrawBatch>();
    int wg0;
    const int li = layer_of(bt, wg0);
    const LBBNN_CONST_AS DrawLayer& a = bt->l[li];
    const int m = blockIdx.y;
    const int q = ((int)blockIdx.x - wg0) * kDrawNT + (int)threadIdx.x;
    const int nq = a.nq, oq = (a.O + 3) >> 2;
    if (q >= nq + oq) return;
    const bool noise = !bt->mean_only;
    uint64_t seed = 0, offs = 0;
    if (noise) { seed = bt->rng[0]; offs = bt->rng[1] + (uint64_t)m; }
    float e[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (q < nq) {
        if (noise) philox_normal4(seed, offs, LBBNN_STREAM_EPS_W * 64u + a.layer, (uint64_t)q, 0u, e);
        const float* z = a.z ? a.z + (size_t)m * a.z_ms : nullptr;
        const unsigned imax = (unsigned)a.I - 1u;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = 4 * q + t;
            o[t] = 0.f;                                                   // (the tail of the last quad)
            if (k >= a.nnz) continue;
            float mz = a.mean[k];
            if (z) mz *= z[min((unsigned)a.col[k], imax)];                // the column inside [0, I) whatever the array holds
            o[t] = noise ? __builtin_fmaf(sqrt_hw(a.var[k]), e[t], mz) : mz;
        }
        *reinterpret_cast<float4*>(a.w + (size_t)m * a.w_ms + 4 * (size_t)q) = make_float4(o[0], o[1], o[2], o[3]);
        if (a.wt) {                                                       // the sweep's order: the place inside [0, nnz) whatever tpos holds
            float* wt = a.wt + (size_t)m * a.w_ms;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (4 * q + t < a.nnz) wt[min((unsigned)a.tpos[4 * q + t], (unsigned)a.nnz - 1u)] = o[t];
        }
    } else {
        const int p = q - nq;
        if (noise) philox_normal4(seed, offs, LBBNN_STREAM_EPS_B * 64u + a.layer, (uint64_t)p, 0u, e);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int u = 4 * p + t;
            o[t] = 0.f;
            if (u >= a.O) continue;
            o[t] = noise ? __builtin_fmaf(sqrt_hw(a.bias_var[u]), e[t], a.bias_mu[u]) : a.bias_mu[u];
        }
        *reinterpret_cast<float4*>(a.b + (size_t)m * a.b_ms + 4 * (size_t)p) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

struct GaArgs { lbbnn_sparse_gather_args_t g; int a_bytes; };            // a_bytes: what a block of `a` spans

// One entry of a unit's pattern row for the lane's rows: the input line is taken inside [0, K) and the value slot inside
// [0, nnz) whatever the arrays hold (one unsigned minimum each); the value is wave-uniform, the line a buffer load at a
// scalar offset
#define LBBNN_GA_LOAD(t, k)                                                         \
    do {                                                                            \
        const unsigned c = min((unsigned)a.idx[k], kmax);                           \
        w[t] = wm[kSlot ? min((unsigned)a.slot[k], smax) : (unsigned)(k)];          \
        x[t] = R::load(act, boff, c * lda4);                                        \
    } while (0)

// The bias path of the layer whose G is this launch's INPUT, done by kR extra workgroups per row tile ahead of the unit groups
// (blockIdx.x < kR): 64 batch rows, four waves.  Wave w walks the w-th quarter of the input lines (a stream of
// independent line loads, kDotChunk of them in flight, feeding ONE chain of FMAs in line order) and lane-for-lane the four
// partial sums are added in wave order through LDS -- an order fixed by K alone.  acc[(m * B + b) * per_member + c] += the sum.
// A launch of its own per layer was what the call's time at one row tile was made of.
__device__ __forceinline__ void gather_bias_dot(const lbbnn_sparse_gather_args_t& a, int blk, int mem, int b0) {
#pragma clang fp contract(off)
    __shared__ float part[kDotW][kDotNT];
    const int lane = threadIdx.x & (kDotNT - 1), wv = threadIdx.x / kDotNT;
    const int b = b0 + lane, bb = b < a.B ? b : 0;                        // (a lane past the batch sums row 0, never stored)
    const float* g = a.a + (size_t)blk * a.a_mstride + bb;
    const float* bias = a.dot_bias + (size_t)mem * a.dot_b_mstride;
    const int q = (a.K + kDotW - 1) / kDotW, u1 = min(a.K, (wv + 1) * q);
    float s = 0.f;
    int u = wv * q;
    for (; u + kDotChunk <= u1; u += kDotChunk) {
        float v[kDotChunk];
#pragma unroll
        for (int t = 0; t < kDotChunk; ++t) v[t] = g[(size_t)(u + t) * a.lda];
#pragma unroll
        for (int t = 0; t < kDotChunk; ++t) s = __builtin_fmaf(v[t], bias[u + t], s);
    }
    for (; u < u1; ++u) s = __builtin_fmaf(g[(size_t)u * a.lda], bias[u], s);
    part[wv][lane] = s;
    __syncthreads();
    if (wv || b >= a.B) return;
    s = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    float* dst = a.dot_acc + ((size_t)mem * a.B + b) * a.per_member + (blk - mem * a.per_member);
    *dst += s;
}

// kR: batch rows per lane, as in sparse_layer_kernel (1: tiles of 64 rows; 2: tiles of 128, lane l owns rows 2l and 2l + 1).
// kU: units per wave -- 4, or 1 where the batch is ONE row tile: a wave's units are walked one after the other, each a chain of
// dependent loads, so at one tile (where the grid is small and every launch is latency) four times the waves take a quarter
// of the time each; a unit's sum is the same chain either way
template <bool kSlot, int kR, int kU>
__global__ __launch_bounds__(256) void sparse_gather_kernel(const GaArgs ga) {
#pragma clang fp contract(off)
    typedef SpRows<kR> R;
    typedef typename R::T rows_t;
    const lbbnn_sparse_gather_args_t& a = ga.g;
    const int lane = threadIdx.x & 63, wv = uniform(threadIdx.x >> 6);
    const int blk = blockIdx.z;
    const int mem = blk / a.per_member;
    const int ablk = a.a_shared ? blk - mem * a.per_member : blk;
    // with dot_bias the first kR workgroups of a row tile are the bias path's (first: their one long chain of loads then runs
    // under the unit groups' work, not behind it)
    const int ndot = a.dot_bias ? kR : 0;
    if ((int)blockIdx.x < ndot) {                                         // (whole workgroups)
        gather_bias_dot(a, blk, mem, ((int)blockIdx.y * kR + (int)blockIdx.x) * 64);
        return;
    }
    const int b = ((int)blockIdx.y * 64 + lane) * kR;                     // the lane's first row
    const bool live = b < a.B;
    // a lane past the batch computes rows 0 .. kR - 1 again (in bounds, never stored): no lane-dependent branch in the loop
    const __amdgpu_buffer_rsrc_t act =
        __builtin_amdgcn_make_buffer_rsrc((void*)(a.a + (size_t)ablk * a.a_mstride), 0, ga.a_bytes, 0x00020000);
    const unsigned lda4 = 4u * (unsigned)a.lda, kmax = (unsigned)a.K - 1u, smax = (unsigned)max(a.nnz, 1) - 1u;
    const unsigned boff = live ? 4u * (unsigned)b : 0u;
    const float* wm = a.w + (size_t)mem * a.w_mstride;
    const int o0 = kU * (((int)blockIdx.x - ndot) * 4 + wv);
    if (o0 >= a.N) return;                                                // (whole waves leave: no barrier below)
    rows_t am[kU];
#pragma unroll
    for (int r = 0; r < kU; ++r) {
        am[r] = R::splat(0.f);
        const int o = o0 + r;
        if (o >= a.N) continue;                                           // wave-uniform
        const int k0 = uniform(clampi(a.ptr[o], 0, a.nnz));
        const int k1 = uniform(clampi(a.ptr[o + 1], k0, a.nnz));
        int k = k0;
        rows_t x[kGaChunk];
        float w[kGaChunk];
        for (; k + kGaChunk <= k1; k += kGaChunk) {
#pragma unroll
            for (int t = 0; t < kGaChunk; ++t) LBBNN_GA_LOAD(t, k + t);
#pragma unroll
            for (int t = 0; t < kGaChunk; ++t) am[r] = R::fma(w[t], x[t], am[r]);
        }
        const int rem = k1 - k;                                           // the last, partial batch: its loads in flight together too
        if (rem > 0) {
#pragma unroll
            for (int t = 0; t < kGaChunk - 1; ++t) if (t < rem) LBBNN_GA_LOAD(t, k + t);
#pragma unroll
            for (int t = 0; t < kGaChunk - 1; ++t) if (t < rem) am[r] = R::fma(w[t], x[t], am[r]);
        }
    }
    if (!live) return;
    float* out = a.out + (size_t)blk * a.o_mstride;
#pragma unroll
    for (int r = 0; r < kU; ++r) {
        const int o = o0 + r;
        if (o >= a.N) continue;
        float res[kR];
#pragma unroll
        for (int i = 0; i < kR; ++i) {
            const int hb = b + i < a.B ? b + i : b;                       // (the pair of an odd last row: computed, never stored)
            const float s = R::get(am[r], i);
            if (a.mode == LBBNN_GATHER_FORWARD) {
                const float v = s + a.bias[(size_t)mem * a.b_mstride + o];
                res[i] = a.relu ? fmaxf(v, 0.f) : v;
            } else if (a.mode == LBBNN_GATHER_SWEEP) {
                res[i] = a.h[(size_t)mem * a.h_mstride + (size_t)o * a.ldh + hb] > 0.f ? s : 0.f;
            } else {
                res[i] = s * a.h[(size_t)o * a.ldh + hb];
            }
        }
        if (kR == 2 && !a.out_rows && b + 1 < a.B) {                      // both rows of the lane: one 8-B store
            *reinterpret_cast<sp_f2*>(out + (size_t)o * a.ldo + b) = sp_f2{res[0], res[kR - 1]};
            continue;
        }
#pragma unroll
        for (int i = 0; i < kR; ++i) {
            if (b + i >= a.B) continue;
            if (a.out_rows) out[(size_t)(b + i) * a.ldo + o] = res[i];
            else out[(size_t)o * a.ldo + b + i] = res[i];
        }
    }
}
#undef LBBNN_GA_LOAD

struct SeedArgs {
    const float* logits; const long long* targets; long long* targets_out; const float* bias; long long b_ms;
    float* seed; float* intercept;
    unsigned long long* rng_live; unsigned long long advance;
    int S, B, C, Cp, ld, pred;
};

// One lane per line position b < ld: the explained output of row b (c', the given target, or with `pred` the first largest
// member-mean logit, summed in member order), the one-hot seed G_L[c'][c][b] (0 past the batch) and the intercept's first term
__global__ __launch_bounds__(kDotNT) void explain_seed_kernel(const SeedArgs a) {
#pragma clang fp contract(off)
    const int b = (int)blockIdx.x * kDotNT + (int)threadIdx.x;
    // the live Philox offset moves on here: every launch that drew from it is ahead of this one on the stream
    if (b == 0 && a.rng_live) a.rng_live[1] += a.advance;
    if (b >= a.ld) return;
    const bool row = b < a.B;
    int t = -1;
    if (row && a.pred) {
        float best = 0.f;
        for (int c = 0; c < a.C; ++c) {
            float s = 0.f;
            for (int m = 0; m < a.S; ++m) s += a.logits[((size_t)m * a.B + b) * a.C + c];
            s /= (float)a.S;
            if (c == 0 || s > best || (s != s && best == best)) { best = s; t = c; }   // (a NaN wins, as torch.argmax has it)
        }
        a.targets_out[b] = t;
    } else if (row && a.targets) {
        const long long v = a.targets[b];
        t = v < 0 ? 0 : (v >= a.C ? a.C - 1 : (int)v);
    }
    for (int cp = 0; cp < a.Cp; ++cp) {
        const int tt = (a.pred || a.targets) ? t : cp;
        for (int c = 0; c < a.C; ++c) a.seed[((size_t)cp * a.C + c) * a.ld + b] = (row && c == tt) ? 1.f : 0.f;
        if (row)
            for (int m = 0; m < a.S; ++m) a.intercept[((size_t)m * a.B + b) * a.Cp + cp] = a.bias[(size_t)m * a.b_ms + tt];
    }
}

// The tile of member m into LDS ([feature][row], rows of 65 floats), zeros outside (F, B)
__device__ __forceinline__ void stats_load_tile(const lbbnn_member_stats_args_t& a, int m, int c, int f0, int b0,
                                                float (*tile)[kTile + 1]) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const float* t = a.t + (size_t)(m * a.C + c) * a.t_mstride;
    const int b = b0 + tx;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int fl = ty * 16 + j, f = f0 + fl;
        tile[fl][tx] = (f < a.F && b < a.B) ? t[(size_t)f * a.ldt + b] : 0.f;
    }
}

// One pass over the members: the mean from the fp64 sum of the values in member order; the deviations from the fp64 sums of
// d = v - v_0 and d^2 (shifted by the first member's value, so the two sums are of the size of the spread and their difference
// does not cancel): sum_m (v - mean)^2 = sum d^2 - (sum d)^2 / S.  Members that agree give d = 0 and a deviation of exactly 0.
__device__ __forceinline__ void member_residual(const lbbnn_member_stats_args_t& a, int m, int c, int b0);

__global__ __launch_bounds__(256) void member_stats_kernel(const lbbnn_member_stats_args_t a) {
    __shared__ float tile[kTile][kTile + 1];
    const int nres = a.residual ? a.S : 0;
    if ((int)blockIdx.x < nres) {                                         // (whole workgroups, ahead of the feature tiles: one per member)
        member_residual(a, blockIdx.x, blockIdx.z, (int)blockIdx.y * kTile);
        return;
    }
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int f0 = ((int)blockIdx.x - nres) * kTile, b0 = (int)blockIdx.y * kTile, c = blockIdx.z;
    const int f = f0 + tx;                                                // the thread's feature; its rows: b0 + 16 ty + j
    double sum[16], ds[16], d2[16];
    float v0[16];
    unsigned cnt[16];                                                     // members > 0 | members < 0 << 16 (S <= 65535)
#pragma unroll
    for (int j = 0; j < 16; ++j) { sum[j] = ds[j] = d2[j] = 0.0; v0[j] = 0.f; cnt[j] = 0u; }
    for (int m = 0; m < a.S; ++m) {
        stats_load_tile(a, m, c, f0, b0, tile);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int b = b0 + ty * 16 + j;
            const float v = tile[tx][ty * 16 + j];
            if (m == 0) v0[j] = v;
            const double d = (double)v - (double)v0[j];
            sum[j] += (double)v; ds[j] += d; d2[j] += d * d;
            cnt[j] += (v > 0.f ? 1u : 0u) + (v < 0.f ? 0x10000u : 0u);
            if (a.members && f < a.F && b < a.B) a.members[(((size_t)m * a.B + b) * a.C + c) * a.F + f] = v;
        }
        __syncthreads();
    }
    if (f >= a.F) return;
    const double S = (double)a.S;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int b = b0 + ty * 16 + j;
        if (b >= a.B) continue;
        const size_t at = ((size_t)b * a.C + c) * a.F + f;
        const double ss = d2[j] - ds[j] * ds[j] / S;
        a.mean[at] = (float)(sum[j] / S);
        a.std[at] = a.S > 1 && ss > 0.0 ? (float)sqrt(ss / (S - 1.0)) : 0.f;
        a.prob_pos[at] = (float)((double)(cnt[j] & 0xFFFFu) / S);
        a.prob_neg[at] = (float)((double)(cnt[j] >> 16) / S);
    }
}

// The residual of member m at 64 rows, by the workgroups of the statistics launch ahead of the feature tiles: as the bias dot,
// kDotW waves take quarters of the features and the four fp64 partial sums are added in wave order
__device__ __forceinline__ void member_residual(const lbbnn_member_stats_args_t& a, int m, int c, int b0) {
    __shared__ double part[kDotW][kDotNT];
    const int lane = threadIdx.x & (kDotNT - 1), wv = threadIdx.x / kDotNT;
    const int b = b0 + lane, bb = b < a.B ? b : 0;
    const float* t = a.t + (size_t)(m * a.C + c) * a.t_mstride + bb;
    const int q = (a.F + kDotW - 1) / kDotW, i1 = min(a.F, (wv + 1) * q);
    double s = 0.0;
    int i = wv * q;
    for (; i + kDotChunk <= i1; i += kDotChunk) {                         // (the loads in flight together, the sum in index order)
        float v[kDotChunk];
#pragma unroll
        for (int k = 0; k < kDotChunk; ++k) v[k] = t[(size_t)(i + k) * a.ldt];
#pragma unroll
        for (int k = 0; k < kDotChunk; ++k) s += (double)v[k];
    }
    for (; i < i1; ++i) s += (double)t[(size_t)i * a.ldt];
    part[wv][lane] = s;
    __syncthreads();
    if (wv || b >= a.B) return;
    s = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    int col = c;
    if (a.targets) {
        const long long v = a.targets[b];
        col = v < 0 ? 0 : (v >= a.n_logits ? a.n_logits - 1 : (int)v);
    }
    const size_t row = (size_t)m * a.B + b;
    a.residual[row * a.C + c] = (float)((double)a.logits[row * a.ldl + col] - (s + (double)a.intercept[row * a.C + c]));
}

bool gather_two_rows(const lbbnn_sparse_gather_args_t& a) {
    // the two-row form reads and writes 8-B words: even strides on 8-B boundaries, and a row B (odd B) that exists
    const bool can2 = !off(a.a, 8) && !(a.lda & 1) && !(a.a_mstride & 1) && a.lda >= a.B + (a.B & 1) &&
                      (a.out_rows || (!off(a.out, 8) && !(a.ldo & 1) && !(a.o_mstride & 1)));
    return can2 && a.B > 64;
}

}  // namespace

extern "C" int lbbnn_sparse_draw_members(const lbbnn_sparse_draw_desc_t* L, int n, int members, const uint64_t* rng, int flags,
                                         void* stream) {
    if (!L) return LBBNN_E_NULL;
    if (n <= 0 || n > LBBNN_MAX_LAYERS || members < 1 || members > 65535) return LBBNN_E_SHAPE;
    if (flags & ~LBBNN_F_MEAN_ONLY) return LBBNN_E_FLAGS;
    const bool mean_only = (flags & LBBNN_F_MEAN_ONLY) != 0;
    if (!mean_only && !rng) return LBBNN_E_NOISE;
    if (off(rng, 8)) return LBBNN_E_ALIGN;
    DrawBatch bt = {};
    int wgs = 0;
    for (int i = 0; i < n; ++i) {
        const lbbnn_sparse_draw_desc_t& d = L[i];
        if (!d.bias_mu || !d.bias_var || !d.b) return LBBNN_E_NULL;
        if (d.nnz > 0 && (!d.col || !d.mean || !d.var || !d.w)) return LBBNN_E_NULL;
        if ((d.tpos != nullptr) != (d.wt != nullptr)) return LBBNN_E_NULL;
        if (d.O < 1 || d.I < 1 || d.nnz < 0) return LBBNN_E_SHAPE;
        const long long wq = ((long long)d.nnz + 3) / 4 * 4, bq = ((long long)d.O + 3) / 4 * 4;
        if (d.w_mstride < wq || d.b_mstride < bq || (d.z && d.z_mstride < d.I)) return LBBNN_E_SHAPE;
        if (!aligned4(d.col) || !aligned4(d.mean) || !aligned4(d.var) || !aligned4(d.bias_mu) || !aligned4(d.bias_var) ||
            !aligned4(d.z) || !aligned4(d.tpos) || !aligned4(d.wt) || off(d.w, 16) || off(d.b, 16) || (d.w_mstride & 3) || (d.b_mstride & 3)) return LBBNN_E_ALIGN;
        DrawLayer& a = bt.l[i];
        a.col = d.col; a.mean = d.mean; a.var = d.var; a.bias_mu = d.bias_mu; a.bias_var = d.bias_var;
        a.z = d.z; a.z_ms = d.z_mstride; a.tpos = d.tpos; a.wt = d.wt; a.w = d.w; a.w_ms = d.w_mstride; a.b = d.b; a.b_ms = d.b_mstride;
        a.O = d.O; a.I = d.I; a.nnz = d.nnz; a.nq = (int)(wq / 4); a.layer = d.layer_id;
        wgs += (int)((wq / 4 + bq / 4 + kDrawNT - 1) / kDrawNT);
        bt.wg_end[i] = wgs;
    }
    bt.n = n; bt.mean_only = mean_only ? 1 : 0; bt.rng = rng;
    hipLaunchKernelGGL(sparse_draw_kernel, dim3(wgs, members), dim3(kDrawNT), 0, static_cast<hipStream_t>(stream), bt);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_sparse_gather_members(const lbbnn_sparse_gather_args_t* args, void* stream) {
    if (!args) return LBBNN_E_NULL;
    const lbbnn_sparse_gather_args_t& a = *args;
    if (a.B == 0) return 0;
    if (a.mode != LBBNN_GATHER_FORWARD && a.mode != LBBNN_GATHER_SWEEP && a.mode != LBBNN_GATHER_FINISH) return LBBNN_E_FLAGS;
    const bool fwd = a.mode == LBBNN_GATHER_FORWARD;
    if (!a.ptr || !a.a || !a.out || (fwd ? !a.bias : !a.h)) return LBBNN_E_NULL;
    if (a.nnz > 0 && (!a.idx || !a.w)) return LBBNN_E_NULL;
    if ((a.dot_bias != nullptr) != (a.dot_acc != nullptr)) return LBBNN_E_NULL;
    if (a.dot_bias && (a.a_shared || a.dot_b_mstride < 0)) return LBBNN_E_FLAGS;
    if (a.B < 0 || (long long)a.B > 65535LL * 64 || a.K < 1 || a.N < 1 || a.nnz < 0 || a.blocks < 1 || a.blocks > 65535 ||
        a.per_member < 1 || a.blocks % a.per_member) return LBBNN_E_SHAPE;
    if (a.lda < a.B || (!fwd && a.ldh < a.B) || a.ldo < (a.out_rows ? a.N : a.B) || a.w_mstride < 0 || a.b_mstride < 0 ||
        a.a_mstride < 0 || a.h_mstride < 0 || a.o_mstride < 0) return LBBNN_E_SHAPE;
    const long long need = a.out_rows ? (long long)(a.B - 1) * a.ldo + a.N : (long long)(a.N - 1) * a.ldo + a.B;
    if (a.blocks > 1 && a.o_mstride < need) return LBBNN_E_SHAPE;
    // the kernel addresses a block's input as a buffer: K lines of B rows -- of B + 1 where lda has room for the pair of an
    // odd last row (the two-row form reads it and drops it)
    const long long a_bytes = 4 * ((long long)(a.K - 1) * a.lda + a.B + ((a.B & 1) && a.lda > a.B ? 1 : 0));
    if (a_bytes > 0x7FFFFFF0LL) return LBBNN_E_SHAPE;
    if (!aligned4(a.ptr) || !aligned4(a.idx) || !aligned4(a.slot) || !aligned4(a.w) || !aligned4(a.bias) || !aligned4(a.a) ||
        !aligned4(a.h) || !aligned4(a.out) || !aligned4(a.dot_bias) || !aligned4(a.dot_acc)) return LBBNN_E_ALIGN;
    GaArgs k = {a, (int)a_bytes};
    k.g.relu = a.relu ? 1 : 0; k.g.out_rows = a.out_rows ? 1 : 0; k.g.a_shared = a.a_shared ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(256);
    const bool two = gather_two_rows(a), slot = a.slot != nullptr;
    const unsigned tiles = (unsigned)(two ? (a.B + 127) / 128 : (a.B + 63) / 64);
    const bool one = tiles == 1;                                          // one unit per wave
    // (with dot_bias: one more workgroup per 64 rows of a tile, ahead of the unit groups)
    const dim3 grid((unsigned)((one ? (a.N + 3) / 4 : (a.N + 15) / 16) + (a.dot_bias ? (two ? 2 : 1) : 0)), tiles, (unsigned)a.blocks);
#define LBBNN_GA_LAUNCH(S_, R_, U_) hipLaunchKernelGGL((sparse_gather_kernel<S_, R_, U_>), grid, block, 0, s, k)
    if (two) {
        if (slot) { if (one) LBBNN_GA_LAUNCH(true, 2, 1); else LBBNN_GA_LAUNCH(true, 2, 4); }
        else { if (one) LBBNN_GA_LAUNCH(false, 2, 1); else LBBNN_GA_LAUNCH(false, 2, 4); }
    } else {
        if (slot) { if (one) LBBNN_GA_LAUNCH(true, 1, 1); else LBBNN_GA_LAUNCH(true, 1, 4); }
        else { if (one) LBBNN_GA_LAUNCH(false, 1, 1); else LBBNN_GA_LAUNCH(false, 1, 4); }
    }
#undef LBBNN_GA_LAUNCH
    return (int)hipGetLastError();
}

extern "C" int lbbnn_explain_seed(const float* logits, const int64_t* targets, int pred, int64_t* targets_out, const float* bias,
                                  int64_t b_mstride, float* seed, int ld, float* intercept, int S, int B, int C, int Cp,
                                  uint64_t* rng_live, uint64_t advance, void* stream) {
    if (B == 0) return 0;
    if (!bias || !seed || !intercept || (pred && (!logits || !targets_out))) return LBBNN_E_NULL;
    if (S < 1 || S > 65535 || B < 0 || C < 1 || Cp < 1 || ld < B || b_mstride < 0 || (S > 1 && b_mstride < C)) return LBBNN_E_SHAPE;
    if ((pred || targets) ? Cp != 1 : Cp != C) return LBBNN_E_SHAPE;
    if (pred && targets) return LBBNN_E_FLAGS;
    if (!aligned4(logits) || !aligned4(bias) || !aligned4(seed) || !aligned4(intercept) || off(targets, 8) || off(targets_out, 8) ||
        off(rng_live, 8)) return LBBNN_E_ALIGN;
    SeedArgs k = {logits, (const long long*)targets, (long long*)targets_out, bias, b_mstride, seed, intercept,
                  (unsigned long long*)rng_live, (unsigned long long)advance, S, B, C, Cp, ld, pred ? 1 : 0};
    hipLaunchKernelGGL(explain_seed_kernel, dim3((unsigned)((ld + kDotNT - 1) / kDotNT)), dim3(kDotNT), 0,
                       static_cast<hipStream_t>(stream), k);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_explain_member_stats(const lbbnn_member_stats_args_t* args, void* stream) {
    if (!args) return LBBNN_E_NULL;
    const lbbnn_member_stats_args_t& a = *args;
    if (a.B == 0) return 0;
    if (!a.t || !a.mean || !a.std || !a.prob_pos || !a.prob_neg) return LBBNN_E_NULL;
    if (a.residual && (!a.logits || !a.intercept)) return LBBNN_E_NULL;
    if (a.S < 1 || a.S > 65535 || a.C < 1 || (long long)a.S * a.C > 65535 || a.F < 1 || a.B < 0 || a.ldt < a.B ||
        a.t_mstride < (long long)(a.F - 1) * a.ldt + a.B || (long long)a.B > 65535LL * kTile) return LBBNN_E_SHAPE;
    if (a.residual && (a.n_logits < 1 || a.ldl < a.n_logits || (a.targets ? a.C != 1 : a.C > a.n_logits))) return LBBNN_E_SHAPE;
    if (!aligned4(a.t) || !aligned4(a.mean) || !aligned4(a.std) || !aligned4(a.prob_pos) || !aligned4(a.prob_neg) ||
        !aligned4(a.members) || !aligned4(a.logits) || !aligned4(a.intercept) || !aligned4(a.residual) || off(a.targets, 8))
        return LBBNN_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (with residual: S more workgroups per row tile and output, ahead of the feature tiles)
    hipLaunchKernelGGL(member_stats_kernel, dim3((unsigned)((a.F + kTile - 1) / kTile + (a.residual ? a.S : 0)),
                                                 (unsigned)((a.B + kTile - 1) / kTile), (unsigned)a.C), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}
