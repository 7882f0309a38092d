// lbbnn_adam_step: multi-tensor Adam in one launch (see include/lbbnn.h).  HBM-bound elementwise: 16 B read + 12 B
// written per parameter.  Workgroup -> (tensor, 4096-element chunk) by a binary search over the per-tensor chunk
// prefix held in the kernel arguments (read through the kernarg pointer: scalar loads, no scratch copy).
// lbbnn_adam_step_groups: the same pass for the tensors of any number of parameter groups, hyper-parameters and step counters
// read from device tables; lbbnn_sgd_step_groups: torch.optim.SGD's update in the same form;
// lbbnn_grad_sumsq: the global gradient norm for clipping, fixed-order sums.  lbbnn_*_step_groups_guarded: the two list kernels
// instantiated with a device-side skip word.
#include <cmath>
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "reduce_partials.h"

namespace {

using namespace lbbnn;
constexpr int CHUNK = 4096;     // elements per workgroup: 256 threads x 4 float4

struct AdamKArgs {
    lbbnn_adam_list_t l;
    int first[LBBNN_ADAM_MAX_TENSORS + 1];     // first workgroup of tensor i; first[n] = grid size
    float lr, b1, b2, eps, wd;
    const float* step;
};

__global__ __launch_bounds__(256) void adam_kernel(const AdamKArgs ka) {
    const LBBNN_CONST_AS AdamKArgs& a = *kernarg_as<AdamKArgs>();
    const int blk = blockIdx.x;
    int lo = 0, hi = a.l.n;                                   // largest i with first[i] <= blk
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.first[mid] <= blk) lo = mid; else hi = mid; }
    const int ti = lo;
    float* __restrict__ p = a.l.p[ti];
    const float* __restrict__ g = a.l.g[ti];
    float* __restrict__ m = a.l.m[ti];
    float* __restrict__ v = a.l.v[ti];
    const int64_t n = a.l.numel[ti];
    const int64_t base = (int64_t)(blk - a.first[ti]) * CHUNK;
    const float t = a.step[0] + 1.f;
    const float bc1 = 1.f - powf(a.b1, t), bc2s = sqrtf(1.f - powf(a.b2, t));
    const float step_size = a.lr / bc1, b1 = a.b1, b2 = a.b2, eps = a.eps, wd = a.wd;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + (int64_t)(threadIdx.x + 256 * k) * 4;
        if (i >= n) break;
        float pp[4], gg[4], mm[4], vv[4];
        const int cnt = (int)((n - i) < 4 ? (n - i) : 4);
        if (vec && cnt == 4) {
            const float4 a0 = *reinterpret_cast<const float4*>(p + i), a1 = *reinterpret_cast<const float4*>(g + i);
            const float4 a2 = *reinterpret_cast<const float4*>(m + i), a3 = *reinterpret_cast<const float4*>(v + i);
            pp[0] = a0.x; pp[1] = a0.y; pp[2] = a0.z; pp[3] = a0.w;  gg[0] = a1.x; gg[1] = a1.y; gg[2] = a1.z; gg[3] = a1.w;
            mm[0] = a2.x; mm[1] = a2.y; mm[2] = a2.z; mm[3] = a2.w;  vv[0] = a3.x; vv[1] = a3.y; vv[2] = a3.z; vv[3] = a3.w;
        } else {
            for (int q = 0; q < 4; ++q) { const bool in = q < cnt; pp[q] = in ? p[i + q] : 0.f; gg[q] = in ? g[i + q] : 0.f; mm[q] = in ? m[i + q] : 0.f; vv[q] = in ? v[i + q] : 0.f; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float gq = gg[q] + wd * pp[q];
            mm[q] = b1 * mm[q] + (1.f - b1) * gq;
            vv[q] = b2 * vv[q] + (1.f - b2) * gq * gq;
            const float denom = sqrtf(vv[q]) / bc2s + eps;
            pp[q] = pp[q] - step_size * (mm[q] / denom);
        }
        if (vec && cnt == 4) {
            *reinterpret_cast<float4*>(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
            *reinterpret_cast<float4*>(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            *reinterpret_cast<float4*>(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
        } else {
            for (int q = 0; q < cnt; ++q) { p[i + q] = pp[q]; m[i + q] = mm[q]; v[i + q] = vv[q]; }
        }
    }
}

__global__ void adam_advance_kernel(float* step) { step[0] += 1.f; }

// ---- lbbnn_adam_step_groups / lbbnn_grad_sumsq: the list kernels with per-group hyper-parameters read from device memory ----
static_assert(CHUNK == LBBNN_ADAM_CHUNK, "include/lbbnn.h documents the chunk size");

// The counters advance in the launch that used them (both list kernels end in this).  Every wave reaches this barrier only after
// its last use of step[gi] (a value that was used has been returned by its load), thread 0 draws the workgroup's ticket after
// the barrier, and only the holder of the last ticket -- drawn after every other workgroup's barrier -- writes the counters: no
// workgroup can read an advanced one.  The next launch reads them across a kernel boundary.
constexpr uint32_t F_INACTIVE = LBBNN_ADAM_F_INACTIVE;      // "a group without parameters": the same bit in both tables' flags
static_assert(LBBNN_SGD_F_INACTIVE == F_INACTIVE, "advance_groups reads one bit for both tables");
// A guarded launch that skips (skip_step below: the same value in every workgroup) leaves the counters alone and counts the
// skipped step instead; the ticket goes back to zero either way.
template <bool GUARDED, class Hyper>
__device__ __forceinline__ void advance_groups(const Hyper* hyper, float* step, unsigned* ticket, int n_groups, bool skip,
                                               long long* skipped) {
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!last) return;
    if (GUARDED && skip) {
        if (threadIdx.x == 0 && skipped) *skipped += 1;
    } else {
        for (int gq = threadIdx.x; gq < n_groups; gq += 256)
            if (!(hyper[gq].flags & F_INACTIVE)) step[gq] += 1.f;
    }
    if (threadIdx.x == 0) atomicExch(ticket, 0u);
}
// The skip word of a guarded launch, read once at kernel entry.  *guard and *grad_scale are written by earlier launches of the
// stream (the loss, lbbnn_grad_sumsq) and by nothing in this one: every workgroup reads the same value whenever it runs.
__device__ __forceinline__ bool skip_step(const int* guard, const float* grad_scale) {
    return guard[0] != 0 || (grad_scale != nullptr && !isfinite(grad_scale[0]));
}
struct GroupsKArgs {
    lbbnn_adam_group_list_t l;
    int first[LBBNN_ADAM_GROUPS_MAX_TENSORS + 1];     // first workgroup of tensor i; first[n] = number of updating workgroups
    const lbbnn_adam_hyper_t* hyper;
    float* step;
    const float* grad_scale;
    unsigned* ticket;
    int n_groups, advance;
    const int* guard;                                         // the guarded instantiation only
    long long* skipped;
};
static_assert(sizeof(GroupsKArgs) <= 4096, "kernel-argument segment");

template <bool GUARDED>
__global__ __launch_bounds__(256) void adam_groups_kernel(const GroupsKArgs ka) {
    const LBBNN_CONST_AS GroupsKArgs& a = *kernarg_as<GroupsKArgs>();
    const int blk = blockIdx.x;
    const bool skip = GUARDED ? skip_step(a.guard, a.grad_scale) : false;
    if (!skip && blk < a.first[a.l.n]) {                      // (an advance-only launch has one workgroup and no tensor)
        int lo = 0, hi = a.l.n;                               // largest i with first[i] <= blk
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.first[mid] <= blk) lo = mid; else hi = mid; }
        const int ti = lo;
        float* __restrict__ p = a.l.p[ti];
        const float* __restrict__ g = a.l.g[ti];
        float* __restrict__ m = a.l.m[ti];
        float* __restrict__ v = a.l.v[ti];
        const float* __restrict__ mk = a.l.mask[ti];
        const int64_t n = a.l.numel[ti];
        const int64_t base = (int64_t)(blk - a.first[ti]) * CHUNK;
        const int gi = a.l.group[ti];
        const lbbnn_adam_hyper_t h = a.hyper[gi];
        const float t = a.step[gi] + 1.f;
        const float bc1 = 1.f - powf(h.beta1, t), bc2s = sqrtf(1.f - powf(h.beta2, t));
        const bool decoupled = (h.flags & LBBNN_ADAM_F_DECOUPLED) != 0;
        const float step_size = h.lr / bc1, b1 = h.beta1, b2 = h.beta2, eps = h.eps, wd = decoupled ? 0.f : h.weight_decay;
        const float shrink = 1.f - h.lr * h.weight_decay;
        const bool scaled = a.grad_scale != nullptr;
        const float gscale = scaled ? a.grad_scale[0] : 1.f;
        const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                           reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(mk)) & 15u) == 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + (int64_t)(threadIdx.x + 256 * k) * 4;
            if (i >= n) break;
            float pp[4], gg[4], mm[4], vv[4];
            const int cnt = (int)((n - i) < 4 ? (n - i) : 4);
            if (vec && cnt == 4) {
                const float4 a0 = *reinterpret_cast<const float4*>(p + i), a1 = *reinterpret_cast<const float4*>(g + i);
                const float4 a2 = *reinterpret_cast<const float4*>(m + i), a3 = *reinterpret_cast<const float4*>(v + i);
                pp[0] = a0.x; pp[1] = a0.y; pp[2] = a0.z; pp[3] = a0.w;  gg[0] = a1.x; gg[1] = a1.y; gg[2] = a1.z; gg[3] = a1.w;
                mm[0] = a2.x; mm[1] = a2.y; mm[2] = a2.z; mm[3] = a2.w;  vv[0] = a3.x; vv[1] = a3.y; vv[2] = a3.z; vv[3] = a3.w;
                if (mk) { const float4 a4 = *reinterpret_cast<const float4*>(mk + i); gg[0] *= a4.x; gg[1] *= a4.y; gg[2] *= a4.z; gg[3] *= a4.w; }
            } else {
                for (int q = 0; q < 4; ++q) {
                    const bool in = q < cnt;
                    pp[q] = in ? p[i + q] : 0.f; gg[q] = in ? g[i + q] : 0.f; mm[q] = in ? m[i + q] : 0.f; vv[q] = in ? v[i + q] : 0.f;
                    if (mk && in) gg[q] *= mk[i + q];
                }
            }
            if (scaled) {
#pragma unroll
                for (int q = 0; q < 4; ++q) gg[q] *= gscale;
            }
            if (decoupled) {
#pragma unroll
                for (int q = 0; q < 4; ++q) pp[q] *= shrink;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {                     // adam_kernel's update, expression for expression
                const float gq = gg[q] + wd * pp[q];
                mm[q] = b1 * mm[q] + (1.f - b1) * gq;
                vv[q] = b2 * vv[q] + (1.f - b2) * gq * gq;
                const float denom = sqrtf(vv[q]) / bc2s + eps;
                pp[q] = pp[q] - step_size * (mm[q] / denom);
            }
            if (vec && cnt == 4) {
                *reinterpret_cast<float4*>(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
                *reinterpret_cast<float4*>(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
                *reinterpret_cast<float4*>(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
            } else {
                for (int q = 0; q < cnt; ++q) { p[i + q] = pp[q]; m[i + q] = mm[q]; v[i + q] = vv[q]; }
            }
        }
    }
    if (a.advance) advance_groups<GUARDED>(a.hyper, a.step, a.ticket, a.n_groups, skip, a.skipped);
}

// ---- lbbnn_sgd_step_groups: torch.optim.SGD's update over the same list, one row of lbbnn_sgd_hyper_t per group ----
struct SgdKArgs {
    lbbnn_adam_group_list_t l;                                // v is not read; m[i] == NULL: no momentum buffer
    int first[LBBNN_ADAM_GROUPS_MAX_TENSORS + 1];
    const lbbnn_sgd_hyper_t* hyper;
    float* step;
    const float* grad_scale;
    unsigned* ticket;
    int n_groups, advance;
    const int* guard;                                         // the guarded instantiation only
    long long* skipped;
};
static_assert(sizeof(SgdKArgs) <= 4096, "kernel-argument segment");

template <bool GUARDED>
__global__ __launch_bounds__(256) void sgd_groups_kernel(const SgdKArgs ka) {
    const LBBNN_CONST_AS SgdKArgs& a = *kernarg_as<SgdKArgs>();
    const int blk = blockIdx.x;
    const bool skip = GUARDED ? skip_step(a.guard, a.grad_scale) : false;
    if (!skip && blk < a.first[a.l.n]) {                      // (an advance-only launch has one workgroup and no tensor)
        int lo = 0, hi = a.l.n;                               // largest i with first[i] <= blk
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.first[mid] <= blk) lo = mid; else hi = mid; }
        const int ti = lo;
        float* __restrict__ p = a.l.p[ti];
        const float* __restrict__ g = a.l.g[ti];
        const float* __restrict__ mk = a.l.mask[ti];
        const int64_t n = a.l.numel[ti];
        const int64_t base = (int64_t)(blk - a.first[ti]) * CHUNK;
        const int gi = a.l.group[ti];
        const lbbnn_sgd_hyper_t h = a.hyper[gi];
        const bool first_step = a.step[gi] == 0.f;
        const float lr = h.lr, mom = h.momentum, keep = 1.f - h.dampening, wd = h.weight_decay;
        const bool decay = wd != 0.f, nesterov = (h.flags & LBBNN_SGD_F_NESTEROV) != 0;
        float* __restrict__ m = mom != 0.f ? a.l.m[ti] : nullptr;         // the buffer is neither read nor written without momentum
        const bool scaled = a.grad_scale != nullptr;
        const float gscale = scaled ? a.grad_scale[0] : 1.f;
        const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                           reinterpret_cast<uintptr_t>(mk)) & 15u) == 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + (int64_t)(threadIdx.x + 256 * k) * 4;
            if (i >= n) break;
            float pp[4], gg[4], mm[4] = {0.f, 0.f, 0.f, 0.f};
            const int cnt = (int)((n - i) < 4 ? (n - i) : 4);
            const bool load_m = m && !first_step;             // the first step overwrites the buffer: it may hold anything
            if (vec && cnt == 4) {
                const float4 a0 = *reinterpret_cast<const float4*>(p + i), a1 = *reinterpret_cast<const float4*>(g + i);
                pp[0] = a0.x; pp[1] = a0.y; pp[2] = a0.z; pp[3] = a0.w;  gg[0] = a1.x; gg[1] = a1.y; gg[2] = a1.z; gg[3] = a1.w;
                if (load_m) { const float4 a2 = *reinterpret_cast<const float4*>(m + i); mm[0] = a2.x; mm[1] = a2.y; mm[2] = a2.z; mm[3] = a2.w; }
                if (mk) { const float4 a4 = *reinterpret_cast<const float4*>(mk + i); gg[0] *= a4.x; gg[1] *= a4.y; gg[2] *= a4.z; gg[3] *= a4.w; }
            } else {
                for (int q = 0; q < 4; ++q) {
                    const bool in = q < cnt;
                    pp[q] = in ? p[i + q] : 0.f; gg[q] = in ? g[i + q] : 0.f;
                    if (load_m && in) mm[q] = m[i + q];
                    if (mk && in) gg[q] *= mk[i + q];
                }
            }
            if (scaled) {
#pragma unroll
                for (int q = 0; q < 4; ++q) gg[q] *= gscale;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {                     // torch.optim.SGD's _single_tensor_sgd, line for line
                float gq = gg[q];
                if (decay) gq = gq + wd * pp[q];
                if (m) {
                    mm[q] = first_step ? gq : mom * mm[q] + keep * gq;
                    gq = nesterov ? gq + mom * mm[q] : mm[q];
                }
                pp[q] = pp[q] - lr * gq;
            }
            if (vec && cnt == 4) {
                *reinterpret_cast<float4*>(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
                if (m) *reinterpret_cast<float4*>(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            } else {
                for (int q = 0; q < cnt; ++q) { p[i + q] = pp[q]; if (m) m[i + q] = mm[q]; }
            }
        }
    }
    if (a.advance) advance_groups<GUARDED>(a.hyper, a.step, a.ticket, a.n_groups, skip, a.skipped);
}

struct SumsqKArgs {
    lbbnn_adam_group_list_t l;
    int first[LBBNN_ADAM_GROUPS_MAX_TENSORS + 1];
    float* work;                                              // already offset to this list's first partial
    int pad;                                                  // zeros written after the last partial (to a multiple of 64 overall)
};
static_assert(sizeof(SumsqKArgs) <= 4096, "kernel-argument segment");

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const SumsqKArgs ka) {
    const LBBNN_CONST_AS SumsqKArgs& a = *kernarg_as<SumsqKArgs>();
    __shared__ float scratch[4];
    const int blk = blockIdx.x;
    int lo = 0, hi = a.l.n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.first[mid] <= blk) lo = mid; else hi = mid; }
    const float* __restrict__ g = a.l.g[lo];
    const float* __restrict__ mk = a.l.mask[lo];
    const int64_t n = a.l.numel[lo], base = (int64_t)(blk - a.first[lo]) * CHUNK;
    const bool vec = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(mk)) & 15u) == 0;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + (int64_t)(threadIdx.x + 256 * k) * 4;
        if (i >= n) break;
        float gg[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && i + 4 <= n) {
            const float4 a1 = *reinterpret_cast<const float4*>(g + i);
            gg[0] = a1.x; gg[1] = a1.y; gg[2] = a1.z; gg[3] = a1.w;
            if (mk) { const float4 a4 = *reinterpret_cast<const float4*>(mk + i); gg[0] *= a4.x; gg[1] *= a4.y; gg[2] *= a4.z; gg[3] *= a4.w; }
        } else {
            for (int q = 0; q < 4 && i + q < n; ++q) gg[q] = mk ? g[i + q] * mk[i + q] : g[i + q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) s += gg[q] * gg[q];
    }
    s = block_sum<float, 4>(s, scratch);
    if (threadIdx.x == 0) a.work[blk] = s;
    if (blk == (int)gridDim.x - 1 && (int)threadIdx.x < a.pad) a.work[gridDim.x + threadIdx.x] = 0.f;
}

// work: rows x 64 partials (zero padded); cols = 64 floats behind them
__global__ __launch_bounds__(1024) void grad_norm_finalize_kernel(float* work, int rows, float max_norm, float* norm, float* grad_scale) {
    __shared__ float part[3][16][64];
    float* cols = work + (size_t)rows * 64;
    float* const out[3] = {cols, nullptr, nullptr};
    reduce_partials_body(work, 64, 0, rows, 64, 1, out, 0, part);
    if (threadIdx.x < 64) {                                   // the lanes of wave 0 wrote cols[lane] themselves
        const float ss = wave_sum(cols[threadIdx.x]);
        if (threadIdx.x == 0) {
            const float nrm = sqrtf(ss), c = max_norm / (nrm + 1e-6f);
            norm[0] = nrm;
            grad_scale[0] = c > 1.f ? 1.f : c;                // (a NaN norm compares false and stays NaN, as torch.clamp keeps it)
        }
    }
}

struct CopyKArgs { lbbnn_copy_list_t l; int first[LBBNN_ADAM_MAX_TENSORS + 1]; };

__global__ __launch_bounds__(256) void multi_copy_kernel(const CopyKArgs ka) {
    const LBBNN_CONST_AS CopyKArgs& a = *kernarg_as<CopyKArgs>();
    const int blk = blockIdx.x;
    int lo = 0, hi = a.l.n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.first[mid] <= blk) lo = mid; else hi = mid; }
    float* __restrict__ d = a.l.dst[lo];
    const float* __restrict__ sp = a.l.src[lo];
    const int64_t n = a.l.numel[lo], base = (int64_t)(blk - a.first[lo]) * CHUNK;
    const bool vec = ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(sp)) & 15u) == 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + (int64_t)(threadIdx.x + 256 * k) * 4;
        if (i >= n) break;
        if (vec && i + 4 <= n) {
            *reinterpret_cast<float4*>(d + i) = sp ? *reinterpret_cast<const float4*>(sp + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int64_t q = i; q < n && q < i + 4; ++q) d[q] = sp ? sp[q] : 0.f;
        }
    }
}

}  // namespace

extern "C" int lbbnn_adam_step(const lbbnn_adam_list_t* list, float lr, float beta1, float beta2, float eps, float weight_decay,
                               float* step, int advance, void* stream) {
    if (!list || !step) return LBBNN_E_NULL;
    if (list->n < 0 || list->n > LBBNN_ADAM_MAX_TENSORS) return LBBNN_E_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (list->n > 0) {
        AdamKArgs ka;
        ka.l = *list;
        int nb = 0;
        for (int i = 0; i < list->n; ++i) {
            if (!list->p[i] || !list->g[i] || !list->m[i] || !list->v[i]) return LBBNN_E_NULL;
            if (list->numel[i] <= 0) return LBBNN_E_SHAPE;
            ka.first[i] = nb;
            nb += (int)((list->numel[i] + CHUNK - 1) / CHUNK);
        }
        for (int i = list->n; i <= LBBNN_ADAM_MAX_TENSORS; ++i) ka.first[i] = nb;
        ka.lr = lr; ka.b1 = beta1; ka.b2 = beta2; ka.eps = eps; ka.wd = weight_decay; ka.step = step;
        hipLaunchKernelGGL(adam_kernel, dim3(nb), dim3(256), 0, s, ka);
    }
    if (advance) hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, s, step);
    return (int)hipGetLastError();
}

// list checks shared by the two list entry points: 0, or the LBBNN_E_* code; fills first[] and the workgroup count
// (update: p and group are checked; moments: m and v too -- Adam's; SGD reads no v and takes m[i] == NULL)
static int groups_list_blocks(const lbbnn_adam_group_list_t* list, bool update, bool moments, int n_groups, int* first, int64_t* blocks) {
    if (list->n < 0 || list->n > LBBNN_ADAM_GROUPS_MAX_TENSORS) return LBBNN_E_SHAPE;
    int64_t nb = 0;
    for (int i = 0; i < list->n; ++i) {
        if (!list->g[i] || (update && !list->p[i]) || (moments && (!list->m[i] || !list->v[i]))) return LBBNN_E_NULL;
        if (list->numel[i] <= 0 || (update && (list->group[i] < 0 || list->group[i] >= n_groups))) return LBBNN_E_SHAPE;
        first[i] = (int)nb;
        nb += (list->numel[i] + CHUNK - 1) / CHUNK;
        if (nb > 0x7fffffff) return LBBNN_E_SHAPE;
    }
    for (int i = list->n; i <= LBBNN_ADAM_GROUPS_MAX_TENSORS; ++i) first[i] = (int)nb;
    *blocks = nb;
    return 0;
}

// the Adam list step, unguarded (guard == NULL) or guarded
static int adam_groups_launch(const lbbnn_adam_group_list_t* list, const lbbnn_adam_hyper_t* hyper, float* step, int n_groups,
                              const float* grad_scale, uint32_t* ticket, int advance, const int32_t* guard, int64_t* skipped,
                              void* stream) {
    if (!list || !hyper || !step || (advance && !ticket)) return LBBNN_E_NULL;
    if (n_groups < 1 || n_groups > 65536) return LBBNN_E_SHAPE;
    GroupsKArgs ka;
    int64_t nb = 0;
    const int rc = groups_list_blocks(list, true, true, n_groups, ka.first, &nb);
    if (rc) return rc;
    if (nb == 0 && !advance) return 0;
    ka.l = *list;
    ka.hyper = hyper; ka.step = step; ka.grad_scale = grad_scale; ka.ticket = ticket;
    ka.n_groups = n_groups; ka.advance = advance ? 1 : 0;
    ka.guard = guard; ka.skipped = reinterpret_cast<long long*>(skipped);
    const dim3 grid((unsigned)(nb > 0 ? nb : 1));
    if (guard) hipLaunchKernelGGL(adam_groups_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), ka);
    else hipLaunchKernelGGL(adam_groups_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), ka);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_adam_step_groups(const lbbnn_adam_group_list_t* list, const lbbnn_adam_hyper_t* hyper, float* step,
                                      int n_groups, const float* grad_scale, uint32_t* ticket, int advance, void* stream) {
    return adam_groups_launch(list, hyper, step, n_groups, grad_scale, ticket, advance, nullptr, nullptr, stream);
}

extern "C" int lbbnn_adam_step_groups_guarded(const lbbnn_adam_group_list_t* list, const lbbnn_adam_hyper_t* hyper, float* step,
                                              int n_groups, const float* grad_scale, uint32_t* ticket, int advance,
                                              const int32_t* guard, int64_t* skipped, void* stream) {
    if (!guard) return LBBNN_E_NULL;
    return adam_groups_launch(list, hyper, step, n_groups, grad_scale, ticket, advance, guard, skipped, stream);
}

static int sgd_groups_launch(const lbbnn_adam_group_list_t* list, const lbbnn_sgd_hyper_t* hyper, float* step, int n_groups,
                             const float* grad_scale, uint32_t* ticket, int advance, const int32_t* guard, int64_t* skipped,
                             void* stream) {
    if (!list || !hyper || !step || (advance && !ticket)) return LBBNN_E_NULL;
    if (n_groups < 1 || n_groups > 65536) return LBBNN_E_SHAPE;
    SgdKArgs ka;
    int64_t nb = 0;
    const int rc = groups_list_blocks(list, true, false, n_groups, ka.first, &nb);
    if (rc) return rc;
    if (nb == 0 && !advance) return 0;
    ka.l = *list;
    ka.hyper = hyper; ka.step = step; ka.grad_scale = grad_scale; ka.ticket = ticket;
    ka.n_groups = n_groups; ka.advance = advance ? 1 : 0;
    ka.guard = guard; ka.skipped = reinterpret_cast<long long*>(skipped);
    const dim3 grid((unsigned)(nb > 0 ? nb : 1));
    if (guard) hipLaunchKernelGGL(sgd_groups_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), ka);
    else hipLaunchKernelGGL(sgd_groups_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), ka);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_sgd_step_groups(const lbbnn_adam_group_list_t* list, const lbbnn_sgd_hyper_t* hyper, float* step,
                                     int n_groups, const float* grad_scale, uint32_t* ticket, int advance, void* stream) {
    return sgd_groups_launch(list, hyper, step, n_groups, grad_scale, ticket, advance, nullptr, nullptr, stream);
}

extern "C" int lbbnn_sgd_step_groups_guarded(const lbbnn_adam_group_list_t* list, const lbbnn_sgd_hyper_t* hyper, float* step,
                                             int n_groups, const float* grad_scale, uint32_t* ticket, int advance,
                                             const int32_t* guard, int64_t* skipped, void* stream) {
    if (!guard) return LBBNN_E_NULL;
    return sgd_groups_launch(list, hyper, step, n_groups, grad_scale, ticket, advance, guard, skipped, stream);
}

extern "C" int64_t lbbnn_grad_sumsq_workspace(int64_t partials) {
    if (partials < 0) return 0;
    return ((partials + 63) / 64) * 64 + 64;
}

extern "C" int lbbnn_grad_sumsq(const lbbnn_adam_group_list_t* list, float* work, int64_t work_offset, int64_t finalize_count,
                                float max_norm, float* norm, float* grad_scale, void* stream) {
    if (!list || !work || (finalize_count > 0 && (!norm || !grad_scale))) return LBBNN_E_NULL;
    if (work_offset < 0 || finalize_count < 0) return LBBNN_E_SHAPE;
    SumsqKArgs ka;
    int64_t nb = 0;
    const int rc = groups_list_blocks(list, false, false, 0, ka.first, &nb);
    if (rc) return rc;
    if (finalize_count > 0 && (finalize_count != work_offset + nb || !(max_norm > 0.f) || finalize_count > 0x7fffffff)) return LBBNN_E_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nb > 0) {
        ka.l = *list;
        ka.work = work + work_offset;
        ka.pad = (int)(((work_offset + nb + 63) / 64) * 64 - (work_offset + nb));
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nb), dim3(256), 0, s, ka);
    }
    if (finalize_count > 0)
        hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(1024), 0, s, work, (int)((finalize_count + 63) / 64), max_norm, norm,
                           grad_scale);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_multi_copy(const lbbnn_copy_list_t* list, void* stream) {
    if (!list) return LBBNN_E_NULL;
    if (list->n < 0 || list->n > LBBNN_ADAM_MAX_TENSORS) return LBBNN_E_SHAPE;
    if (list->n == 0) return 0;
    CopyKArgs ka;
    ka.l = *list;
    int nb = 0;
    for (int i = 0; i < list->n; ++i) {
        if (!list->dst[i]) return LBBNN_E_NULL;
        if (list->numel[i] <= 0) return LBBNN_E_SHAPE;
        ka.first[i] = nb;
        nb += (int)((list->numel[i] + CHUNK - 1) / CHUNK);
    }
    for (int i = list->n; i <= LBBNN_ADAM_MAX_TENSORS; ++i) ka.first[i] = nb;
    hipLaunchKernelGGL(multi_copy_kernel, dim3(nb), dim3(256), 0, static_cast<hipStream_t>(stream), ka);
    return (int)hipGetLastError();
}
