// Local explanations of a frozen posterior-mean forward (gfx950), see include/lbbnn.h: logits = J(b) x + k(b) exactly, because
// the forward is a ReLU chain on fixed operands.  The backward sweep keeps G as a (B * C', width) fp32 matrix; its matrix
// products are lbbnn_lrt_gemm (mean only) on transposed fp32 operands, and everything between two products is here.
//
//   explain_step_kernel -- lbbnn_explain_step, three modes.  ONE WAVE PER INPUT ROW b (four rows per 256-thread workgroup): a
//     lane owns the float4 column groups lane, lane + 64, ... of the row.  The activation row h[b] (finish: x[b]) is read once
//     and serves the C' <= 16 rows of G that share it; the C' bias dots / row sums live in registers and are reduced with the
//     fixed-order wave_sum, so the intercept and the residual are the same bits on every run.  No atomics, no LDS.
//       seed:   G[b, c, j] = W_L[t(b, c), j] * [h[b, j] > 0], intercept = b_L[t] + <G, bias>, active count, masks (optional)
//       mask:   G[b, c, j] *= [h[b, j] > 0] in place, intercept += <G, bias>, active count, masks (optional)
//       finish: contributions[b, c, map[i]] = G[b, c, i] * x[b, i]; residual = logits[b, t] - (row sum + intercept).  Depth 1
//               (no G): the row of G is the row t of W_L itself and intercept = b_L[t] is written here.
//     Rows are read as float4 when the width, every row stride and every base allow it, element by element otherwise.
//   explain_totals_kernel / explain_totals_reduce_kernel -- lbbnn_explain_totals: per-workgroup fp64 column partials of the
//     contributions and of their absolute values (a workgroup owns a block of input rows and 256 columns, a thread one
//     column, rows in order), then ONE workgroup adds the partials block by block into the running totals.  The order of every
//     addition is fixed by the shapes alone (eval_metrics.hip's scheme): no float atomics.
//   explain_operand_kernel -- lbbnn_explain_operand: the fp32 value hi + lo of a bf16 hi | lo operand (exact: both parts lie
//     inside the 24-bit window of the value they split), as plain rows -- what the sweep multiplies by where the forward
//     multiplied by the two planes.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "operand_store.h"

namespace {

using namespace lbbnn;

constexpr int kExRows = 4;                         // input rows (= waves) per workgroup
constexpr int kExNT = 64 * kExRows;
constexpr int kExMaxC = LBBNN_EXPLAIN_MAX_OUTPUTS;
constexpr int kTotCols = 256;                      // columns (= threads) per workgroup of the totals
constexpr int kTotMaxBlocks = 256;                 // row blocks of the totals: bounds the work buffer whatever B is

struct StepArgs {
    float* g; const float* w; const int64_t* targets; const float* h; const float* bias; const float* bias_out;
    float* intercept; int32_t* active; uint8_t* mask_out; const float* logits; const int32_t* map;
    float* contributions; float* residual;
    long long ldg, ldw, ldh, ld_active, ldm, ldl, ldc;
    int mode, B, C, width, w_rows, full_width, vec, vec_bias;
};

// columns 4j .. 4j+3 of a row of `width` elements; elements at or past width read as 0
__device__ __forceinline__ float4 ex_ld4(const float* row, int j, int width, bool vec) {
    if (vec) return reinterpret_cast<const float4*>(row)[j];
    const int k = 4 * j;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < width) v.x = row[k];
    if (k + 1 < width) v.y = row[k + 1];
    if (k + 2 < width) v.z = row[k + 2];
    if (k + 3 < width) v.w = row[k + 3];
    return v;
}
__device__ __forceinline__ void ex_st4(float* row, int j, int width, bool vec, const float4 v) {
    if (vec) { reinterpret_cast<float4*>(row)[j] = v; return; }
    const int k = 4 * j;
    if (k < width) row[k] = v.x;
    if (k + 1 < width) row[k + 1] = v.y;
    if (k + 2 < width) row[k + 2] = v.z;
    if (k + 3 < width) row[k + 3] = v.w;
}

__device__ __forceinline__ int ex_target(const int64_t* targets, size_t b, int n) {
    const int64_t t = targets[b];
    return t < 0 ? 0 : (t >= n ? n - 1 : (int)t);            // (the host side refuses such a target; nothing is read out of range)
}

__global__ __launch_bounds__(kExNT) void explain_step_kernel(const StepArgs a_) {
    const LBBNN_CONST_AS StepArgs* a = kernarg_as<StepArgs>();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long bb = (long long)blockIdx.x * kExRows + wv;
    if (bb >= a->B) return;                                   // (whole waves leave: no barrier below)
    const size_t b = (size_t)bb;
    const int mode = a->mode, C = a->C, width = a->width, nq = (width + 3) >> 2;
    const bool vec = a->vec != 0, vecb = a->vec_bias != 0;
    const bool by_target = a->targets != nullptr;
    const int tb = by_target ? ex_target(a->targets, b, a->w_rows) : 0;
    const float* const hrow = a->h + b * (size_t)a->ldh;
    float acc[kExMaxC];
#pragma unroll
    for (int c = 0; c < kExMaxC; ++c) acc[c] = 0.f;

    if (mode == LBBNN_EXPLAIN_FINISH) {
        const bool from_w = a->g == nullptr;
        const int32_t* const map = a->map;
        const bool vecc = vec && !map;                        // (vec: the host side also checked contributions and ldc)
        for (int j = lane; j < nq; j += 64) {
            const float4 xv = ex_ld4(hrow, j, width, vec);
#pragma unroll
            for (int c = 0; c < kExMaxC; ++c) {
                if (c >= C) continue;                            // wave-uniform
                const int t = by_target ? tb : c;
                const size_t r = b * (size_t)C + c;
                const float4 gv = from_w ? ex_ld4(a->w + (size_t)t * a->ldw, j, width, vec) : ex_ld4(a->g + r * a->ldg, j, width, vec);
                // the products as they are stored: the row sum adds the fp32 contributions themselves
                const float4 p = make_float4(__fmul_rn(gv.x, xv.x), __fmul_rn(gv.y, xv.y), __fmul_rn(gv.z, xv.z), __fmul_rn(gv.w, xv.w));
                float* const crow = a->contributions + r * a->ldc;
                if (map) {
                    const int k = 4 * j, F = a->full_width;
                    if (k < width) crow[clamped_index(map, k, F)] = p.x;
                    if (k + 1 < width) crow[clamped_index(map, k + 1, F)] = p.y;
                    if (k + 2 < width) crow[clamped_index(map, k + 2, F)] = p.z;
                    if (k + 3 < width) crow[clamped_index(map, k + 3, F)] = p.w;
                } else {
                    ex_st4(crow, j, width, vecc, p);
                }
                acc[c] = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc[c], p.x), p.y), p.z), p.w);
            }
        }
#pragma unroll
        for (int c = 0; c < kExMaxC; ++c) {
            if (c >= C) continue;
            const float s = wave_sum(acc[c]);
            if (lane == 0) {
                const int t = by_target ? tb : c;
                const size_t r = b * (size_t)C + c;
                float ic;
                if (from_w) { ic = a->bias_out[t]; a->intercept[r] = ic; }
                else ic = a->intercept[r];
                a->residual[r] = a->logits[b * (size_t)a->ldl + t] - (s + ic);
            }
        }
        return;
    }

    const bool seed = mode == LBBNN_EXPLAIN_SEED;
    int cnt = 0;
    for (int j = lane; j < nq; j += 64) {
        const float4 hv = ex_ld4(hrow, j, width, vec);        // past the width: 0, so not active
        const float4 bv = ex_ld4(a->bias, j, width, vecb);
        const bool mx = hv.x > 0.f, my = hv.y > 0.f, mz = hv.z > 0.f, mw = hv.w > 0.f;
        cnt += (int)mx + (int)my + (int)mz + (int)mw;
        if (a->mask_out) {
            uint8_t* const mrow = a->mask_out + b * (size_t)a->ldm;
            const int k = 4 * j;
            if (k < width) mrow[k] = mx;
            if (k + 1 < width) mrow[k + 1] = my;
            if (k + 2 < width) mrow[k + 2] = mz;
            if (k + 3 < width) mrow[k + 3] = mw;
        }
#pragma unroll
        for (int c = 0; c < kExMaxC; ++c) {
            if (c >= C) continue;                                // wave-uniform
            const int t = by_target ? tb : c;
            float* const grow = a->g + (b * (size_t)C + c) * a->ldg;
            float4 gv = seed ? ex_ld4(a->w + (size_t)t * a->ldw, j, width, vec) : ex_ld4(grow, j, width, vec);
            gv = make_float4(mx ? gv.x : 0.f, my ? gv.y : 0.f, mz ? gv.z : 0.f, mw ? gv.w : 0.f);
            ex_st4(grow, j, width, vec, gv);
            acc[c] = fmaf(gv.w, bv.w, fmaf(gv.z, bv.z, fmaf(gv.y, bv.y, fmaf(gv.x, bv.x, acc[c]))));
        }
    }
    const int total = (int)wave_sum((float)cnt);              // per-lane counts are < 2^24: their float sum is exact
    if (lane == 0) a->active[b * (size_t)a->ld_active] = total;
#pragma unroll
    for (int c = 0; c < kExMaxC; ++c) {
        if (c >= C) continue;
        const float s = wave_sum(acc[c]);
        if (lane == 0) {
            const size_t r = b * (size_t)C + c;
            const float base = seed ? a->bias_out[by_target ? tb : c] : a->intercept[r];
            a->intercept[r] = base + s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ totals
// rows of input per block of the totals: 64, or more when B is large enough that 64 would exceed kTotMaxBlocks blocks
inline int tot_rows_per_block(long long B) {
    const long long r = (B + kTotMaxBlocks - 1) / kTotMaxBlocks;
    return (int)(r < 64 ? 64 : r);
}
inline int tot_blocks(long long B) { const int r = tot_rows_per_block(B); return (int)((B + r - 1) / r); }

struct TotArgs {
    const float* contributions; const int64_t* targets; double* sum; double* abs_sum; int64_t* rows; double* work;
    long long ldc;
    int B, C, I, rpb, nblk;
};
// work: [nblk][2][C][I] doubles, then [nblk][C] int64 row counts

__global__ __launch_bounds__(kTotCols) void explain_totals_kernel(const TotArgs a_) {
    const LBBNN_CONST_AS TotArgs* a = kernarg_as<TotArgs>();
    const int tid = threadIdx.x, blk = blockIdx.x;
    const int C = a->C, I = a->I;
    const int col = (int)blockIdx.y * kTotCols + tid;
    const long long b0 = (long long)blk * a->rpb;
    const int nb = (int)((a->B - b0) < a->rpb ? (a->B - b0) : a->rpb);
    const int64_t* const tg = a->targets;
    const size_t CI = (size_t)C * I;
    double* const wp = a->work + (size_t)blk * 2 * CI;
    if (col < I) {
        for (int cls = 0; cls < C; ++cls) {
            double s = 0.0, ab = 0.0;
            for (int k = 0; k < nb; ++k) {                    // rows in order: the partial is the same bits on every run
                const size_t b = (size_t)(b0 + k);
                size_t r;
                if (tg) {
                    if (ex_target(tg, b, C) != cls) continue; // (uniform over the workgroup)
                    r = b;
                } else {
                    r = b * (size_t)C + cls;
                }
                const double v = (double)a->contributions[r * a->ldc + col];
                s += v; ab += fabs(v);
            }
            wp[(size_t)cls * I + col] = s;
            wp[CI + (size_t)cls * I + col] = ab;
        }
    }
    if (blockIdx.y == 0 && tid < C) {
        long long n = nb;
        if (tg) {
            n = 0;
            for (int k = 0; k < nb; ++k) n += ex_target(tg, (size_t)(b0 + k), C) == tid ? 1 : 0;
        }
        reinterpret_cast<int64_t*>(a->work + (size_t)a->nblk * 2 * CI)[(size_t)blk * C + tid] = n;
    }
}

__global__ __launch_bounds__(1024) void explain_totals_reduce_kernel(const TotArgs a_) {
    const LBBNN_CONST_AS TotArgs* a = kernarg_as<TotArgs>();
    const int tid = threadIdx.x, C = a->C, nblk = a->nblk;
    const size_t CI = (size_t)C * a->I;
    for (size_t e = tid; e < 2 * CI; e += 1024) {
        double s = 0.0;
        for (int blk = 0; blk < nblk; ++blk) s += a->work[(size_t)blk * 2 * CI + e];      // block by block: a fixed order
        double* const dst = e < CI ? a->sum + e : a->abs_sum + (e - CI);
        *dst += s;
    }
    if (tid < C) {
        const int64_t* const cnt = reinterpret_cast<const int64_t*>(a->work + (size_t)nblk * 2 * CI);
        int64_t n = 0;
        for (int blk = 0; blk < nblk; ++blk) n += cnt[(size_t)blk * C + tid];
        a->rows[tid] += n;
    }
}

// ------------------------------------------------------------------------------------------------ hi + lo of a split operand
__device__ __forceinline__ float bf16_val(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

__global__ __launch_bounds__(256) void explain_operand_kernel(const uint16_t* __restrict__ op, float* __restrict__ out, int ld,
                                                              long long items) {
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int n8 = ld >> 3;
    const long long o = it / n8;
    const int k0 = 8 * (int)(it - o * n8);
    const uint16_t* const p = op + split_hi_index((size_t)o, k0, ld);
    const uint4 hi = *reinterpret_cast<const uint4*>(p), lo = *reinterpret_cast<const uint4*>(p + kSplitLoOffset);
    const uint32_t h[4] = {hi.x, hi.y, hi.z, hi.w}, l[4] = {lo.x, lo.y, lo.z, lo.w};
    float w[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w[2 * q] = bf16_val(h[q] & 0xFFFFu) + bf16_val(l[q] & 0xFFFFu);
        w[2 * q + 1] = bf16_val(h[q] >> 16) + bf16_val(l[q] >> 16);
    }
    store8(out, (size_t)o, k0, ld, w);
}

}  // namespace

extern "C" int lbbnn_explain_step(const lbbnn_explain_step_args_t* p, void* stream) {
    if (!p) return LBBNN_E_NULL;
    const lbbnn_explain_step_args_t& d = *p;
    const bool finish = d.mode == LBBNN_EXPLAIN_FINISH, seed = d.mode == LBBNN_EXPLAIN_SEED, mask = d.mode == LBBNN_EXPLAIN_MASK;
    const bool from_w = seed || (finish && !d.g);
    if (!d.h || !d.intercept) return LBBNN_E_NULL;
    if (finish) {
        if (!d.logits || !d.contributions || !d.residual) return LBBNN_E_NULL;
    } else {
        if (!d.g || !d.bias || !d.active) return LBBNN_E_NULL;
    }
    if (from_w && (!d.w || !d.bias_out)) return LBBNN_E_NULL;
    if (!finish && !seed && !mask) return LBBNN_E_SHAPE;
    if (d.B < 0 || d.width < 1 || d.C < 1 || d.C > LBBNN_EXPLAIN_MAX_OUTPUTS) return LBBNN_E_SHAPE;
    if ((long long)d.B * d.C > LBBNN_EXPLAIN_MAX_ROWS) return LBBNN_E_SHAPE;
    if (d.ldh < d.width || (d.g && d.ldg < d.width)) return LBBNN_E_SHAPE;
    if (d.targets && d.C != 1) return LBBNN_E_SHAPE;
    if (from_w || finish) {
        if (d.w_rows < 1 || (!d.targets && d.C > d.w_rows)) return LBBNN_E_SHAPE;     // rows out of range
    }
    if (from_w && d.ldw < d.width) return LBBNN_E_SHAPE;
    if (!finish && (d.ld_active < 1 || (d.mask_out && d.ldm < d.width))) return LBBNN_E_SHAPE;
    if (finish) {
        if (d.ldl < d.w_rows) return LBBNN_E_SHAPE;
        if (d.map ? d.full_width < d.width : d.full_width != d.width) return LBBNN_E_SHAPE;
        if (d.ldc < d.full_width) return LBBNN_E_SHAPE;
    }
    if (!aligned4(d.g) || !aligned4(d.w) || !aligned4(d.h) || !aligned4(d.bias) || !aligned4(d.bias_out) || !aligned4(d.intercept) ||
        !aligned4(d.active) || !aligned4(d.logits) || !aligned4(d.map) || !aligned4(d.contributions) || !aligned4(d.residual))
        return LBBNN_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(d.targets) & 7u) return LBBNN_E_ALIGN;
    if (d.B == 0) return 0;
    StepArgs a = {};
    a.g = d.g; a.w = d.w; a.targets = mask ? nullptr : d.targets; a.h = d.h; a.bias = d.bias; a.bias_out = d.bias_out; a.intercept = d.intercept;
    a.active = d.active; a.mask_out = finish ? nullptr : d.mask_out; a.logits = d.logits; a.map = finish ? d.map : nullptr;
    a.contributions = d.contributions; a.residual = d.residual;
    a.ldg = d.ldg; a.ldw = d.ldw; a.ldh = d.ldh; a.ld_active = d.ld_active; a.ldm = d.ldm; a.ldl = d.ldl; a.ldc = d.ldc;
    a.mode = d.mode; a.B = d.B; a.C = d.C; a.width = d.width; a.w_rows = d.w_rows; a.full_width = d.full_width;
    // float4 rows: the width, every row stride and every base the kernel reads or writes as a row
    bool vec = (d.width % 4 == 0) && aligned16(d.h) && (d.ldh % 4 == 0);
    if (d.g) vec = vec && aligned16(d.g) && (d.ldg % 4 == 0);
    if (from_w) vec = vec && aligned16(d.w) && (d.ldw % 4 == 0);
    if (finish && !d.map) vec = vec && aligned16(d.contributions) && (d.ldc % 4 == 0);
    a.vec = vec ? 1 : 0;
    a.vec_bias = (!finish && d.width % 4 == 0 && aligned16(d.bias)) ? 1 : 0;
    const long long wgs = ((long long)d.B + kExRows - 1) / kExRows;
    hipLaunchKernelGGL(explain_step_kernel, dim3((unsigned)wgs), dim3(kExNT), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

extern "C" int64_t lbbnn_explain_work_bytes(int B, int C, int I) {
    if (B < 1 || C < 1 || C > LBBNN_EXPLAIN_MAX_OUTPUTS || I < 1 || (long long)B * C > LBBNN_EXPLAIN_MAX_ROWS) return 0;
    const long long nblk = tot_blocks(B);
    return nblk * (2LL * C * I * 8 + (long long)C * 8);
}

extern "C" int lbbnn_explain_totals(const float* contributions, int64_t ldc, const int64_t* targets, int B, int C, int I,
                                    double* sum, double* abs_sum, int64_t* rows, void* work, void* stream) {
    if (!contributions || !sum || !abs_sum || !rows || !work) return LBBNN_E_NULL;
    if (B < 0 || C < 1 || C > LBBNN_EXPLAIN_MAX_OUTPUTS || I < 1 || ldc < I) return LBBNN_E_SHAPE;
    if ((long long)B * (targets ? 1 : C) > LBBNN_EXPLAIN_MAX_ROWS) return LBBNN_E_SHAPE;
    if (!aligned4(contributions)) return LBBNN_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(targets) & 7u) || (reinterpret_cast<uintptr_t>(sum) & 7u) || (reinterpret_cast<uintptr_t>(abs_sum) & 7u) ||
        (reinterpret_cast<uintptr_t>(rows) & 7u) || (reinterpret_cast<uintptr_t>(work) & 7u)) return LBBNN_E_ALIGN;
    if (B == 0) return 0;
    TotArgs a = {};
    a.contributions = contributions; a.targets = targets; a.sum = sum; a.abs_sum = abs_sum; a.rows = rows;
    a.work = static_cast<double*>(work); a.ldc = ldc; a.B = B; a.C = C; a.I = I;
    a.rpb = tot_rows_per_block(B); a.nblk = tot_blocks(B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(explain_totals_kernel, dim3(a.nblk, (I + kTotCols - 1) / kTotCols), dim3(kTotCols), 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(explain_totals_reduce_kernel, dim3(1), dim3(1024), 0, s, a);
    return (int)hipGetLastError();
}

extern "C" int lbbnn_explain_operand(const void* op, int O, int I, int ld, float* out, void* stream) {
    if (!op || !out) return LBBNN_E_NULL;
    if (O < 1 || I < 1 || ld < I) return LBBNN_E_SHAPE;
    if ((ld & 31) || !aligned16(op) || !aligned16(out)) return LBBNN_E_ALIGN;
    const long long items = (long long)O * (ld >> 3);
    const long long blocks = (items + 255) / 256;
    if (blocks > 0x7FFFFFFFLL) return LBBNN_E_SHAPE;
    hipLaunchKernelGGL(explain_operand_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t*>(op), out, ld, items);
    return (int)hipGetLastError();
}
