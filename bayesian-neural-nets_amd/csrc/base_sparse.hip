// Sparse median-probability model of a baseline LBBNN network (gfx950), see include/lbbnn.h: the kept weights of
// freeze_base(net, "mpm") in CSR, and every member's explicit weights drawn on that pattern alone.
//
//   csr_rows_kernel<BaseRule> (csr_pack.h) -- lbbnn_base_sparse_count / lbbnn_base_sparse_pack: the count / pack of the LRT / MNF
//     sparse model with the keep rule of base_frozen_operands_kernel, sigma itself as the third value, b_mu / b_sigma per row.
//   base_sparse_draw_kernel -- lbbnn_base_sparse_draw_members: ONE WAVE PER CSR ROW, the rows of all layers on gridDim.x, the
//     members on gridDim.y with a stride inside (base_frozen_members_kernel's split: pattern and planes are read once per
//     member stride).  A lane owns slot row_ptr[o] + 64 j + lane: the row o is the wave's, so the Philox counter of the weight is
//     the FULL network's (o, col / 4) without a row array, and the value is base_frozen_members_kernel's fused mu + sigma * eps.
//     One Philox evaluation per lane and member: at the densities this model is for, most quads hold one kept weight.
// No LDS, no atomics, plain vector stores; every index read from device memory is clamped before it is followed.
#include "csr_pack.h"

namespace {

using namespace lbbnn;

constexpr int kBsRows = 4;                 // weight rows (= waves) per workgroup of the draw kernel
constexpr int kBsNT = 64 * kBsRows;

// lbbnn_base_sparse_count / _pack: csr_pack.h's single-level kernel under BaseRule, the threshold as every layer's one cut
int base_sparse_rows(const lbbnn_base_sparse_desc_t* L, int n, float threshold, bool pack, void* stream) {
    const int args = threshold > 0.f && threshold < 1.f ? 0 : LBBNN_E_FLAGS;
    return csr_rows<BaseRule, 1>(L, n, pack, args, stream, [threshold](const lbbnn_base_sparse_desc_t& d, CsrLayer<1>& a) {
        a.mu = d.mu; a.rho = d.rho; a.lambdal = d.lambdal; a.bias_mu = d.bias_mu; a.bias_rho = d.bias_rho;
        a.row_ptr = d.row_ptr; a.col = d.col; a.mean = d.mean; a.val = d.sigma; a.row0 = d.b_mu; a.row1 = d.b_sigma;
        a.kept_rows = d.kept_rows;
        a.O = d.O; a.I = d.I; a.nnz = d.nnz; a.K = 1; a.cut[0] = threshold;
    });
}

struct BdLayer {
    const int32_t* row_ptr; const int32_t* col; const float* mean; const float* sigma; const float* b_mu; const float* b_sigma;
    const int32_t* tpos; float* wt;        // nullable pair: the weights once more, slot k at place tpos[k] (column by column)
    float* w; long long w_ms; float* b; long long b_ms;
    int O, I, nnz;
    uint32_t layer;
};
struct BdBatch {
    BdLayer l[LBBNN_MAX_LAYERS];
    int wg_end[LBBNN_MAX_LAYERS];
    int n, mean_only, members;
    unsigned long long adv;
    const uint64_t* rng;
};

// word `k` (0..3) of a register quad without indexing memory
__device__ __forceinline__ float word4(const float v[4], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3]; }

__global__ __launch_bounds__(kBsNT) void base_sparse_draw_kernel(const BdBatch bt_) {
    const LBBNN_CONST_AS BdBatch* bt = kernarg_as<BdBatch>();
    int wg0;
    const int li = layer_of(bt, wg0);
    const LBBNN_CONST_AS BdLayer& a = bt->l[li];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int o = kBsRows * ((int)blockIdx.x - wg0) + wv;
    if (o >= a.O) return;                                                 // (whole waves leave: no barrier below)
    const int members = bt->members, m0 = blockIdx.y, mstep = gridDim.y;
    const int nnz = a.nnz, O = a.O;
    const bool noise = !bt->mean_only;
    uint64_t seed = 0, off0 = 0;
    if (noise) { seed = bt->rng[0]; off0 = bt->rng[1]; }
    const uint64_t adv = bt->adv;
    const uint32_t s_w = LBBNN_STREAM_EPS_W * 64u + a.layer, s_b = LBBNN_STREAM_EPS_B * 64u + a.layer;
    const bool last = o == O - 1;

    // the member biases, at the row's counter: lane t draws those of members t, t + 64, ... (first member stride only); the
    // wave of the last row also writes the zero tail of every member's block
    if (m0 == 0) {
        const float bm = a.b_mu[o], sb = a.b_sigma[o];
        const int tail = ((O + 3) & ~3) - O;
        for (int m = lane; m < members; m += 64) {
            float v = bm;
            if (noise) {
                float n[4];
                philox_normal4(seed, off0 + (uint64_t)m * adv, s_b, (uint64_t)(o >> 2), 0u, n);
                v = __builtin_fmaf(sb, word4(n, o & 3), bm);              // b_mu + b_sigma * eps as base_frozen_members_kernel fuses it
            }
            float* const bp = a.b + (size_t)m * a.b_ms;
            bp[o] = v;
            if (last) for (int t = 0; t < tail; ++t) bp[O + t] = 0.f;
        }
    }

    // the row's slots, inside [0, nnz] whatever row_ptr holds
    const int k0 = uniform(clampi(a.row_ptr[o], 0, nnz));
    const int k1 = uniform(clampi(a.row_ptr[o + 1], k0, nnz));
    const unsigned imax = (unsigned)a.I - 1u;
    for (int kb = k0; kb < k1; kb += 64) {
        const int k = kb + lane;
        if (k >= k1) continue;                                            // (no wave operation below)
        const unsigned c = min((unsigned)a.col[k], imax);                 // the column inside [0, I) whatever the array holds
        const float mu = a.mean[k], sg = a.sigma[k];
        const unsigned tp = a.wt ? min((unsigned)a.tpos[k], (unsigned)nnz - 1u) : 0u;
        for (int m = m0; m < members; m += mstep) {
            float v = mu;
            if (noise) {
                float n[4];
                philox_normal4(seed, off0 + (uint64_t)m * adv, s_w, (uint64_t)o, (uint32_t)(c >> 2), n);
                v = __builtin_fmaf(sg, word4(n, (int)(c & 3u)), mu);      // mu + sigma * eps, fused as in the dense member kernel
            }
            a.w[(size_t)m * a.w_ms + k] = v;
            if (a.wt) a.wt[(size_t)m * a.w_ms + tp] = v;
        }
    }
    // the zero tail of the last quad of every member's block
    const int wtail = ((nnz + 3) & ~3) - nnz;
    if (last && lane < wtail) {
        for (int m = m0; m < members; m += mstep) {
            a.w[(size_t)m * a.w_ms + nnz + lane] = 0.f;
            if (a.wt) a.wt[(size_t)m * a.w_ms + nnz + lane] = 0.f;
        }
    }
}

}  // namespace

extern "C" int lbbnn_base_sparse_count(const lbbnn_base_sparse_desc_t* L, int n, float threshold, void* stream) {
    return base_sparse_rows(L, n, threshold, false, stream);
}

extern "C" int lbbnn_base_sparse_pack(const lbbnn_base_sparse_desc_t* L, int n, float threshold, void* stream) {
    return base_sparse_rows(L, n, threshold, true, stream);
}

extern "C" int lbbnn_base_sparse_draw_members(const lbbnn_base_sparse_draw_desc_t* L, int n, int members, const uint64_t* rng,
                                              uint64_t member_advance, int flags, void* stream) {
    if (!L) return LBBNN_E_NULL;
    if (n <= 0 || n > LBBNN_MAX_LAYERS || members < 1 || members > 65535) return LBBNN_E_SHAPE;
    if (flags & ~LBBNN_F_MEAN_ONLY) return LBBNN_E_FLAGS;
    const bool mean_only = (flags & LBBNN_F_MEAN_ONLY) != 0;
    if (!mean_only && !rng) return LBBNN_E_NOISE;
    if (off(rng, 8)) return LBBNN_E_ALIGN;
    BdBatch bt = {};
    int wgs = 0;
    for (int i = 0; i < n; ++i) {
        const lbbnn_base_sparse_draw_desc_t& d = L[i];
        if (!d.row_ptr || !d.b_mu || !d.b_sigma || !d.b) return LBBNN_E_NULL;
        if (d.nnz > 0 && (!d.col || !d.mean || !d.sigma || !d.w)) return LBBNN_E_NULL;
        if ((d.tpos != nullptr) != (d.wt != nullptr)) return LBBNN_E_NULL;
        if (d.O < 1 || d.I < 1 || d.nnz < 0) return LBBNN_E_SHAPE;
        const long long wq = ((long long)d.nnz + 3) / 4 * 4, bq = ((long long)d.O + 3) / 4 * 4;
        if (d.w_mstride < wq || d.b_mstride < bq) return LBBNN_E_SHAPE;
        if (!aligned4(d.row_ptr) || !aligned4(d.col) || !aligned4(d.mean) || !aligned4(d.sigma) || !aligned4(d.b_mu) ||
            !aligned4(d.b_sigma) || !aligned4(d.tpos) || off(d.wt, 16) || off(d.w, 16) || off(d.b, 16) || (d.w_mstride & 3) ||
            (d.b_mstride & 3)) return LBBNN_E_ALIGN;
        BdLayer& a = bt.l[i];
        a.row_ptr = d.row_ptr; a.col = d.col; a.mean = d.mean; a.sigma = d.sigma; a.b_mu = d.b_mu; a.b_sigma = d.b_sigma;
        a.tpos = d.tpos; a.wt = d.nnz > 0 ? d.wt : nullptr; a.w = d.w; a.w_ms = d.w_mstride; a.b = d.b; a.b_ms = d.b_mstride;
        a.O = d.O; a.I = d.I; a.nnz = d.nnz; a.layer = d.layer_id;
        wgs += (d.O + kBsRows - 1) / kBsRows;
        bt.wg_end[i] = wgs;
    }
    bt.n = n; bt.mean_only = mean_only ? 1 : 0; bt.members = members; bt.adv = member_advance; bt.rng = rng;
    // members on gridDim.y while the rows alone leave compute units idle (about 8 workgroups per unit), looped inside beyond that
    int my = (2048 + wgs - 1) / wgs;
    my = my < 1 ? 1 : (my > members ? members : my);
    hipLaunchKernelGGL(base_sparse_draw_kernel, dim3(wgs, my), dim3(kBsNT), 0, static_cast<hipStream_t>(stream), bt);
    return (int)hipGetLastError();
}
