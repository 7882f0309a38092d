// Host-only check of the single dual-moment GEMM's entry points under sanitizers: the early-return rows of
// tests/test_capi_symbols.py (test_gemm_entry_points_early_return_codes, test_round3_entry_points_argument_checks) made through
// lbbnn_lrt_gemm and lbbnn_lrt_gemm_ex from a program of its own.  Every call is refused (or is an empty batch) before anything
// is launched, so it needs no device.  Build and run from csrc/ (never loaded into Python):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         ../../tools/gemm_return_codes.cpp lrt_gemm.hip lrt_gemm_f16.hip mnf_flow.hip prepare.hip weight_pass.hip \
//         -o /tmp/gemm_return_codes && /tmp/gemm_return_codes
// Prints one line per table and "all codes as expected"; exit status 1 on the first wrong code.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "../include/lbbnn.h"

namespace {

void* const F = reinterpret_cast<void*>(4096);        // never dereferenced
void* const ODD = reinterpret_cast<void*>(4100);      // off 16 bytes
constexpr int RELU = 0x1, MEAN = 0x2, SPLIT = 0x4, LSM = 0x8, SINGLE = 0x10, HALF = 0x20, UNKNOWN = 0x200;
constexpr int WIDE = 0x20000000;                      // a row stride whose second row lies past the 32-bit buffer offsets

lbbnn_layer_desc_t g_one[5], g_want_kl[5];

// one dual-moment product that would launch: every row below breaks it
lbbnn_gemm_desc_t base() {
    lbbnn_gemm_desc_t d{};
    d.x = F; d.ldx = 8; d.e_w = F; d.var_w = F; d.ld = 32; d.eps = static_cast<const float*>(F);
    d.out = static_cast<float*>(F); d.ldo = 24; d.B = 4; d.I = 8; d.O = 24;
    return d;
}

using Change = std::function<void(lbbnn_gemm_desc_t&)>;
struct Row { Change change; int code; };

int positional(const lbbnn_gemm_desc_t& d) {
    return lbbnn_lrt_gemm(static_cast<const float*>(d.x), d.ldx, d.e_w, d.var_w, d.ld, d.bias_mean, d.bias_var, d.var_scale, d.eps,
                          d.rng, d.rng_stream, d.row_offset, d.out, d.ldo, d.B, d.I, d.O, d.flags, nullptr);
}
int descriptor(const lbbnn_gemm_desc_t& d) { return lbbnn_lrt_gemm_ex(&d, nullptr); }

#define ROW(code, ...) Row{[](lbbnn_gemm_desc_t& d) { __VA_ARGS__; }, code}

// the dispatch's early returns, in its order (_DISPATCH of the test)
std::vector<Row> dispatch() {
    return {
        ROW(0, d.B = 0; d.x = nullptr),
        ROW(-1, d.x = nullptr; d.B = -1), ROW(-1, d.e_w = nullptr), ROW(-1, d.out = nullptr),
        ROW(-2, d.B = -1; d.flags = UNKNOWN), ROW(-2, d.I = 0), ROW(-2, d.O = 0), ROW(-2, d.ldx = 4), ROW(-2, d.ldo = 8),
        ROW(-4, d.flags = UNKNOWN; d.var_w = nullptr),
        ROW(-4, d.flags = HALF | SPLIT; d.var_w = nullptr),
        ROW(-4, d.flags = HALF | SINGLE | SPLIT | MEAN),
        ROW(-4, d.flags = LSM; d.var_w = nullptr),
        ROW(-4, d.flags = LSM | RELU; d.O = 8; d.ldo = 8; d.var_w = nullptr),
        ROW(-4, d.flags = SINGLE; d.var_w = nullptr),
        ROW(-1, d.var_w = nullptr; d.eps = nullptr),
        ROW(-5, d.eps = nullptr; d.ld = 30),
        ROW(-3, d.ld = 30; d.e_w = ODD), ROW(-3, d.ld = 0; d.flags = SPLIT; d.O = 16),
        ROW(-3, d.e_w = ODD; d.flags = SPLIT; d.O = 16), ROW(-3, d.var_w = ODD),
        ROW(-3, d.flags = SPLIT; d.O = 16; d.ldo = 16; d.ldx = WIDE),
        ROW(-3, d.flags = SPLIT; d.I = 12; d.ldx = 12), ROW(-3, d.flags = SPLIT; d.x = ODD),
        ROW(-2, d.flags = SPLIT; d.B = 2; d.ldx = WIDE),
        ROW(-2, d.flags = SPLIT; d.O = 1 << 24; d.ldo = 1 << 24),
    };
}

int run(const char* what, const std::vector<Row>& rows, size_t from, const Change& form, int (*call)(const lbbnn_gemm_desc_t&)) {
    for (size_t i = from; i < rows.size(); ++i) {
        lbbnn_gemm_desc_t d = base();
        form(d);
        rows[i].change(d);
        const int rc = call(d);
        if (rc != rows[i].code) {
            std::printf("%s: row %zu returned %d, expected %d\n", what, i, rc, rows[i].code);
            return 1;
        }
    }
    std::printf("%-44s %zu rows\n", what, rows.size() - from);
    return 0;
}

}  // namespace

int main() {
    g_want_kl[0].want_kl = 1;
    const Change none = [](lbbnn_gemm_desc_t&) {};
    const Change fin = [](lbbnn_gemm_desc_t& d) { d.layers = g_one; d.n_layers = 1; };
    const std::vector<Row> disp = dispatch();
    std::vector<Row> std_out = {ROW(-4, d.flags = MEAN; d.std_out = static_cast<float*>(F); d.x = nullptr)};
    std_out.insert(std_out.end(), disp.begin(), disp.end());
    std::vector<Row> finalize = {
        ROW(-2, d.n_layers = -1; d.advance = 1), ROW(-2, d.layers = nullptr; d.advance = 1),
        ROW(-1, d.advance = 1; d.flags = MEAN; d.std_out = static_cast<float*>(F)),
        ROW(-4, d.flags = MEAN; d.std_out = static_cast<float*>(F); d.n_layers = 0; d.x = nullptr),
        ROW(-4, d.flags = MEAN; d.std_out = static_cast<float*>(F); d.layers = g_want_kl),
        ROW(-1, d.n_layers = 0; d.layers = nullptr; d.x = nullptr), ROW(0, d.n_layers = 0; d.layers = nullptr; d.B = 0),
        ROW(-2, d.n_layers = 5; d.x = nullptr), ROW(-1, d.layers = g_want_kl; d.x = nullptr),
        ROW(-1, d.kl_total = static_cast<float*>(F); d.x = nullptr),
    };
    finalize.insert(finalize.end(), disp.begin() + 1, disp.end());
    // what only the row-scaled fp16 format has, on a descriptor without LBBNN_F_F16S (each also invalid later: no x);
    // LBBNN_F_SPLIT16 on one with it; a NULL descriptor
    const std::vector<Row> formats = {
        ROW(-4, d.x = nullptr; d.flags = LBBNN_F_VAR1), ROW(-4, d.x = nullptr; d.flags = LBBNN_F_XPLANES),
        ROW(-4, d.x = nullptr; d.flags = SPLIT | LBBNN_F_VAR1),
        ROW(-4, d.x = nullptr; d.mean_scale = static_cast<float*>(F)), ROW(-4, d.x = nullptr; d.wvar_scale = static_cast<float*>(F)),
        ROW(-4, d.x = nullptr; d.flags = SPLIT; d.out_planes = F), ROW(-4, d.x = nullptr; d.head_out = static_cast<float*>(F)),
        ROW(-4, d.x = nullptr; d.flags = LBBNN_F_F16S | SPLIT),
        ROW(-1, d.flags = LBBNN_F_F16S),                                  // the fp16 branch: no scales
        ROW(-2, d.flags = LBBNN_F_F16S; d.mean_scale = d.wvar_scale = static_cast<float*>(F); d.O = 10),
    };
    int bad = lbbnn_lrt_gemm_ex(nullptr, nullptr) != -1;
    bad = bad || run("lbbnn_lrt_gemm", disp, 0, none, positional);
    bad = bad || run("lbbnn_lrt_gemm_ex (plain product)", disp, 0, none, descriptor);
    bad = bad || run("lbbnn_lrt_gemm_ex std_out", std_out, 0, none, descriptor);
    bad = bad || run("lbbnn_lrt_gemm_ex finalize", finalize, 0, fin, descriptor);
    bad = bad || run("lbbnn_lrt_gemm_ex formats", formats, 0, none, descriptor);
    std::printf(bad ? "a code differs\n" : "all codes as expected\n");
    return bad;
}
