// lbbnn_gate_structure (include/lbbnn.h): the posterior over network structures.  Per sample the hard gates of every layer are
// drawn from Philox -- the draw of lbbnn_gate_sample_draw / lbbnn_gate_members, u < sigmoid_ref(lambdal) -- and the backward
// `any` sweep of evaluate.live_structure runs on them in the same pass: no gate is ever stored.  Integers only.
//
// ONE launch for the whole network, one workgroup of 256 threads per sample.  The need vectors of two adjacent boundaries sit
// in static LDS as bytes (2 x 4096).  Layers run last to first.  A work unit is (column group g of 4 consecutive columns, row
// slice r): it walks rows r, r + R, ... with ONE Philox call per row (counter (o, g): the four uniforms of its columns), keeps
// its columns' need bytes and its counters in registers, and the R slices of a group are ORed through LDS once per layer
// (R > 1 only; the host picks R per layer so that the G * R units fill the 256 threads, R * G <= 1024).  No atomics in the
// sweep; every weight is drawn, needed row or not (kept counts them).  The totals over samples are integer atomicAdd: the
// same bits on every run.
//
// Measured and not kept: four samples per workgroup sharing each lambdal load and its sigmoid (need bit s of
// a byte = sample s).  Same bits; a workgroup then takes 3.9 ms where this one takes 1.65 ms on 784-1200-1200-10, which loses
// at S = 10 and 100 and is level at S = 1000.
#include "lbbnn_device.h"
#include "lbbnn_internal.h"
#include "operand_store.h"

namespace {

using namespace lbbnn;

constexpr int kGsThreads = 256;
constexpr int kGsWaves = kGsThreads / 64;
constexpr int kGsMaxWidth = LBBNN_STRUCTURE_MAX_WIDTH;       // 4096 units per boundary
constexpr int kGsMaxUnits = 1024;                            // G * R of a layer: its slices' need words fill `part`

struct StructLayer {
    const float* lambdal;
    int O, I, ld;
    uint32_t stream;         // LBBNN_STREAM_GATE * 64 + layer_id
    int R;                   // row slices per column group
    int vec;                 // rows readable as float4: I % 4 == 0, ld % 4 == 0, base 16-B aligned
    int need_off;            // first unit of boundary l (this layer's columns) in a row of need_out
    int unit_off;            // the same in unit_count (hidden boundaries only; unused for l = 0)
};

struct StructLaunch {
    StructLayer l[LBBNN_STRUCTURE_MAX_LAYERS];
    int n, width;            // width: units of all n + 1 boundaries = the row length of need_out
    const uint64_t* rng;
    int32_t* kept; int32_t* needed; int32_t* active;
    int32_t* feature_count; int32_t* unit_count;
    uint8_t* need_out;
};

__device__ __forceinline__ uint32_t pick_word(const Philox4& r, int k) { return k == 0 ? r.x : k == 1 ? r.y : k == 2 ? r.z : r.w; }

__global__ __launch_bounds__(kGsThreads) void gate_structure_kernel(const StructLaunch a_) {
    __shared__ uint32_t need[2][kGsMaxWidth / 4];            // [boundary & 1][unit / 4]: one byte (0 / 1) per unit
    __shared__ uint32_t part[kGsMaxUnits];                   // [r * G + g]: slice r's need word of column group g
    __shared__ int red[3][kGsWaves];
    const LBBNN_CONST_AS StructLaunch* a = kernarg_as<StructLaunch>();
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = a->n, W = a->width;
    const size_t s = blockIdx.x;                             // this workgroup's sample; the grid is `samples` wide
    const uint64_t seed = a->rng[0], offs = a->rng[1] + (uint64_t)s;
    uint8_t* const need_row = a->need_out ? a->need_out + s * W : nullptr;

    // boundary n: every output unit is needed
    {
        const LBBNN_CONST_AS StructLayer& L = a->l[n - 1];
        const int On = L.O, off = L.need_off + L.I;          // off + On == W
        uint8_t* const nb = reinterpret_cast<uint8_t*>(need[n & 1]);
        for (int j = tid; j < On; j += kGsThreads) {
            nb[j] = 1;
            if (need_row) need_row[off + j] = 1;
        }
        if (tid == 0) a->needed[s * (n + 1) + n] = On;
    }
    __syncthreads();

    for (int l = n - 1; l >= 0; --l) {                       // (uniform per workgroup)
        const LBBNN_CONST_AS StructLayer& L = a->l[l];
        const float* const lam = L.lambdal;
        const int O = L.O, I = L.I, ld = L.ld, R = L.R, vec = L.vec;
        const uint32_t stream = L.stream;
        const int G = (I + 3) >> 2, U = G * R;               // U <= kGsMaxUnits
        const uint8_t* const nrow = reinterpret_cast<const uint8_t*>(need[(l + 1) & 1]);      // rows: boundary l + 1
        uint32_t* const ncol = need[l & 1];                                                  // columns: boundary l
        int kept = 0, act = 0, cnt = 0;

        for (int u = tid; u < U; u += kGsThreads) {
            const int r = u / G, g = u - r * G, i0 = 4 * g;
            uint32_t cn = 0;                                 // byte k: the need of column i0 + k
            for (int o = r; o < O; o += R) {
                const float* const row = lam + (size_t)o * ld;
                float lm[4] = {0.f, 0.f, 0.f, 0.f};
                if (vec) {                                   // I % 4 == 0: i0 + 3 < I
                    const float4 v = *reinterpret_cast<const float4*>(row + i0);
                    lm[0] = v.x; lm[1] = v.y; lm[2] = v.z; lm[3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (i0 + k < I) lm[k] = row[i0 + k];
                }
                const Philox4 p = philox_bits4(seed, offs, stream, (uint64_t)o, (uint32_t)g);
                const uint32_t nd = nrow[o];                 // 0 / 1
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // a column past I draws its word and stores nothing
                    const uint32_t gm = (i0 + k < I && uniform24(pick_word(p, k)) < sigmoid_ref(lm[k])) ? 1u : 0u;
                    kept += (int)gm;
                    act += (int)(gm & nd);
                    cn |= (gm & nd) << (8 * k);
                }
            }
            if (R == 1) ncol[g] = cn;                        // g < G <= 1024
            else part[u] = cn;                               // u < U <= 1024
        }
        __syncthreads();
        if (R > 1) {
            for (int g = tid; g < G; g += kGsThreads) {
                uint32_t cn = 0;
                for (int r = 0; r < R; ++r) cn |= part[r * G + g];
                ncol[g] = cn;
            }
            __syncthreads();
        }

        // boundary l: its needed count, its totals over samples, its need row
        int32_t* const total = l == 0 ? a->feature_count : (a->unit_count ? a->unit_count + L.unit_off : nullptr);
        for (int g = tid; g < G; g += kGsThreads) {
            const uint32_t cn = ncol[g];
            cnt += __popc(cn);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = 4 * g + k;
                const uint32_t b = (cn >> (8 * k)) & 1u;
                if (i >= I) continue;
                if (total && b) atomicAdd(total + i, 1);
                if (need_row) need_row[L.need_off + i] = (uint8_t)b;
            }
        }
        {                                                    // every lane of every wave takes part
            const int k1 = wave_sum(kept), a1 = wave_sum(act), c1 = wave_sum(cnt);
            if (lane == 0) { red[0][wv] = k1; red[1][wv] = a1; red[2][wv] = c1; }
        }
        __syncthreads();
        if (tid < 3) {
            int v = 0;
#pragma unroll
            for (int w = 0; w < kGsWaves; ++w) v += red[tid][w];
            if (tid == 0) a->kept[s * n + l] = v;
            else if (tid == 1) a->active[s * n + l] = v;
            else a->needed[s * (n + 1) + l] = v;
        }
        // the next layer's sweep ends in a barrier before `red` is written again, and reads need[(l + 1) & 1] no more
    }
}

// row slices of a layer: the R in 1 .. min(O, 32) with G * R <= kGsMaxUnits that wastes the fewest thread slots -- of the
// ceil(G * R / 256) passes, and of the longest slice against the even share of the rows (the smallest such R on a tie)
int pick_slices(int O, int I) {
    const int G = (I + 3) / 4;
    int best = 1;
    double best_fill = 0.0;
    for (int R = 1; R <= 32 && R <= O && G * R <= kGsMaxUnits; ++R) {
        const int U = G * R, passes = (U + kGsThreads - 1) / kGsThreads;
        const double fill = ((double)U / (passes * kGsThreads)) * ((double)O / R) / (double)((O + R - 1) / R);
        if (fill > best_fill + 1e-9) { best_fill = fill; best = R; }
    }
    return best;
}

int checked_width(const lbbnn_structure_desc_t* layers, int n, int64_t* width) {
    if (!layers) return LBBNN_E_NULL;
    if (n < 1 || n > LBBNN_STRUCTURE_MAX_LAYERS) return LBBNN_E_SHAPE;
    int64_t w = 0;
    for (int l = 0; l < n; ++l) {
        const lbbnn_structure_desc_t& d = layers[l];
        if (!d.lambdal) return LBBNN_E_NULL;
        if (d.O < 1 || d.O > kGsMaxWidth || d.I < 1 || d.I > kGsMaxWidth) return LBBNN_E_SHAPE;
        if (d.ld < d.I) return LBBNN_E_SHAPE;
        if (l && d.I != layers[l - 1].O) return LBBNN_E_SHAPE;
        if (!aligned4(d.lambdal)) return LBBNN_E_ALIGN;
        w += d.I;
    }
    *width = w + layers[n - 1].O;
    return 0;
}

}  // namespace

extern "C" int64_t lbbnn_gate_structure_width(const lbbnn_structure_desc_t* layers, int n) {
    int64_t w = 0;
    return checked_width(layers, n, &w) == 0 ? w : 0;
}

extern "C" int lbbnn_gate_structure(const lbbnn_structure_desc_t* layers, int n, int samples, const uint64_t* rng,
                                    int32_t* kept, int32_t* needed, int32_t* active, int32_t* feature_count,
                                    int32_t* unit_count, uint8_t* need_out, void* stream) {
    if (!layers || !kept || !needed || !active || !feature_count) return LBBNN_E_NULL;
    if (n < 1 || n > LBBNN_STRUCTURE_MAX_LAYERS || samples < 1 || samples > 65535) return LBBNN_E_SHAPE;
    int64_t width = 0;
    const int rc = checked_width(layers, n, &width);
    if (rc) return rc;
    if (!aligned4(kept) || !aligned4(needed) || !aligned4(active) || !aligned4(feature_count) || !aligned4(unit_count))
        return LBBNN_E_ALIGN;
    if (!rng) return LBBNN_E_NOISE;
    StructLaunch a{};
    int off = 0;
    for (int l = 0; l < n; ++l) {
        const lbbnn_structure_desc_t& d = layers[l];
        StructLayer& L = a.l[l];
        L.lambdal = d.lambdal; L.O = d.O; L.I = d.I; L.ld = d.ld;
        L.stream = LBBNN_STREAM_GATE * 64u + d.layer_id;
        L.R = pick_slices(d.O, d.I);
        L.vec = (d.I % 4) == 0 && (d.ld % 4) == 0 && aligned16(d.lambdal);
        L.need_off = off;
        L.unit_off = l ? off - layers[0].I : 0;
        off += d.I;
    }
    a.n = n; a.width = (int)width; a.rng = rng;
    a.kept = kept; a.needed = needed; a.active = active;
    a.feature_count = feature_count; a.unit_count = unit_count; a.need_out = need_out;
    hipLaunchKernelGGL(gate_structure_kernel, dim3((unsigned)samples), dim3(kGsThreads), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
