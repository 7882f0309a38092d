"""Case table of the dual-moment GEMM's kernel instantiations (csrc/lrt_gemm.hip), shared by
tests/test_gemm_variants_host.py, tests/test_gemm_variants_gpu.py and tests/test_vd_ensemble_gpu.py.

``ops.lrt_gemm_plan`` (lbbnn_lrt_gemm_plan) names the instantiation a call takes: family (skinny / staged / dma / split), tile,
x loads, mean-only, products per moment, fp16, fan-out.  ``CASES`` holds, for every instantiation a single launch can reach,
the smallest shapes that reach it; ``FAMILIES`` holds the rows of the fan-out / members test, one or more per fan-out
instantiation.  Every shape follows from the dispatcher's thresholds:

  O <= 16                                   skinny kernel; 1280 k per batch of its 16 waves, so I = 1284 needs a second batch
  ceil(O / 80) * ceil(B / 128) >= 256       large tile (80 x 128) -- B = 1921, O = 1201: 16 x 16 = 256; B = 1920: 240, small
  (split: ... and B >= 96)
  I % 4 == 0, ldx % 4 == 0, x 16-B aligned  vector x loads; with I % 16 == 0 the LDS-DMA kernel, else register-staged
  F_SPLIT16                                 I % 8 == 0 and vector x, else LBBNN_E_ALIGN; K step 32 (I = 40: K tail, 64: none)
  O % 4 == 0 (and ldo % 4 == 0, aligned)    float4 epilogue stores -- O = 84 / 1204 against 83 / 1201

Everything here runs on the CPU and imports neither torch nor the library.
"""
from typing import NamedTuple

F_RELU, F_MEAN_ONLY, F_SPLIT16, F_LOG_SOFTMAX, F_SINGLE16, F_HALF16 = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20

# the bars of the project's own GEMM tests: fp32 (tests/test_parity_gpu.py TIGHT, plus conftest.elementwise_violation <= 1),
# bf16x3 (test_split_gemm_vs_fp64: dual, mean-only), single-product bf16 / fp16 (tests/test_vd_ensemble_gpu.py BARS)
TIGHT = 5e-6
BARS = {("fp32", False): TIGHT, ("fp32", True): TIGHT, ("bf16x3", False): 2e-5, ("bf16x3", True): 5e-5,
        ("bf16", False): 2e-2, ("fp16", False): 2e-3}


class Variant(NamedTuple):
    family: str
    large_tile: bool
    xvec: bool
    mean_only: bool
    products: int
    half: bool
    fan: bool

    @property
    def name(self):
        bits = [self.family, "large" if self.large_tile else ("small" if self.family != "skinny" else ""),
                "xvec" if self.xvec else "xscalar", "mean" if self.mean_only else "dual"]
        if self.family == "split":
            bits.append("fp16" if self.half else ("bf16x%d" % self.products))
        if self.fan:
            bits.append("fan")
        return "-".join(b for b in bits if b)


def variant_of(plan) -> Variant:
    """The Variant of an ops.GemmPlan (everything but the kernel id)."""
    return Variant(plan.family, plan.large_tile, plan.xvec, plan.mean_only, plan.products, plan.half, plan.fan)


def mode_flags(mode: str, mean_only: bool) -> int:
    """The flag bits ops.lrt_gemm sets for an arithmetic mode."""
    f = F_MEAN_ONLY if mean_only else 0
    if mode != "fp32":
        f |= F_SPLIT16
        if mode in ("bf16", "fp16") and not mean_only:
            f |= F_SINGLE16 | (F_HALF16 if mode == "fp16" else 0)
    return f


class Case(NamedTuple):
    """One single launch.  x layout: "pad4": a view of a wider buffer with ldx = I + 4 on a 16-B boundary; "pad3": ldx = I + 3;
    "offset": ldx = I + 4 and the base 4 bytes past a 16-B boundary (column slice starting at 1); "odd": ldx = I + 1."""
    B: int
    I: int
    O: int
    mode: str                 # "fp32" | "bf16x3" | "bf16" | "fp16"
    mean_only: bool
    layout: str
    relu: bool
    variant: Variant

    @property
    def id(self):
        return "%s-B%d-I%d-O%d-%s%s" % (self.variant.name, self.B, self.I, self.O, self.layout, "-relu" if self.relu else "")

    @property
    def ldx(self):
        return self.I + {"pad4": 4, "offset": 4, "pad3": 3, "odd": 1}[self.layout]

    @property
    def x_aligned(self):
        return self.layout != "offset"

    @property
    def flags(self):
        return mode_flags(self.mode, self.mean_only) | (F_RELU if self.relu else 0)

    @property
    def bar(self):
        return BARS[(self.mode, self.mean_only)]


def _v(family, large, xvec, mean, products=1, half=False, fan=False):
    return Variant(family, large, xvec, mean, products, half, fan)


def _cases():
    out = []

    def add(B, I, O, mode, mean, layout, relu, variant):
        out.append(Case(B, I, O, mode, mean, layout, relu, variant))

    # ---- skinny (O <= 16): O in {3, 10, 16}, I in {18 (scalar x, K tail), 20 (vector x), 1284 (second 1280-wide batch)}
    add(37, 18, 3, "fp32", False, "pad4", False, _v("skinny", False, False, False))
    add(37, 18, 16, "fp32", False, "pad3", True, _v("skinny", False, False, False))
    add(37, 20, 10, "fp32", False, "pad4", True, _v("skinny", False, True, False))
    add(37, 1284, 16, "fp32", False, "pad4", False, _v("skinny", False, True, False))
    add(37, 18, 10, "fp32", True, "pad4", False, _v("skinny", False, False, True))
    add(37, 20, 16, "fp32", True, "pad4", True, _v("skinny", False, True, True))
    add(37, 1284, 3, "fp32", True, "pad4", False, _v("skinny", False, True, True))
    add(37, 32, 16, "fp32", False, "offset", False, _v("skinny", False, False, False))
    # ---- tiled fp32, per tile: small (37 x 83 / 84), its upper boundary (1920 x 1201), large (1921 x 1201 / 1204)
    for (B, O1, O2, large) in ((37, 83, 84, False), (1921, 1201, 1204, True)):
        # register-staged: I = 18 scalar x loads and a K tail; I = 20 vector x, one full chunk and a tail
        add(B, 18, O1, "fp32", False, "pad4", False, _v("staged", large, False, False))
        add(B, 18, O2, "fp32", False, "pad3", True, _v("staged", large, False, False))
        add(B, 18, O2, "fp32", True, "pad4", False, _v("staged", large, False, True))
        add(B, 20, O1, "fp32", False, "pad4", True, _v("staged", large, True, False))
        add(B, 20, O2, "fp32", False, "pad4", False, _v("staged", large, True, False))
        add(B, 20, O1, "fp32", True, "pad4", False, _v("staged", large, True, True))
        # a width the DMA kernel would take, in a layout it cannot: misaligned base, odd row stride
        add(B, 32, O2, "fp32", False, "offset", False, _v("staged", large, False, False))
        add(B, 32, O1, "fp32", False, "odd", True, _v("staged", large, False, False))
        add(B, 32, O2, "fp32", True, "odd", False, _v("staged", large, False, True))
        # LDS-DMA: I = 32 two chunks; 48 three, so both LDS buffers are used again
        add(B, 32, O1, "fp32", False, "pad4", False, _v("dma", large, True, False))
        add(B, 48, O2, "fp32", False, "pad4", True, _v("dma", large, True, False))
        add(B, 48, O1, "fp32", True, "pad4", False, _v("dma", large, True, True))
        add(B, 32, O2, "fp32", True, "pad4", True, _v("dma", large, True, True))
        # 16-bit split: I = 40 a K tail (operand_ld(40) - 40 = 24 >= 8 zero floats), I = 64 none
        add(B, 40, O1, "bf16x3", False, "pad4", False, _v("split", large, True, False, 3))
        add(B, 64, O2, "bf16x3", False, "pad4", True, _v("split", large, True, False, 3))
        add(B, 40, O2, "bf16x3", True, "pad4", False, _v("split", large, True, True, 3))
        add(B, 64, O1, "bf16x3", True, "pad4", True, _v("split", large, True, True, 3))
        add(B, 40, O2, "bf16", False, "pad4", False, _v("split", large, True, False, 1))
        add(B, 64, O1, "bf16", False, "pad4", True, _v("split", large, True, False, 1))
        add(B, 40, O1, "fp16", False, "pad4", True, _v("split", large, True, False, 1, True))
        add(B, 64, O2, "fp16", False, "pad4", False, _v("split", large, True, False, 1, True))
    # ---- one row below the large tile: 15 x 16 = 240 workgroups, small tile at the same O
    add(1920, 18, 1201, "fp32", False, "pad4", False, _v("staged", False, False, False))
    add(1920, 20, 1201, "fp32", True, "pad4", False, _v("staged", False, True, True))
    add(1920, 48, 1201, "fp32", False, "pad4", True, _v("dma", False, True, False))
    add(1920, 40, 1201, "bf16x3", False, "pad4", False, _v("split", False, True, False, 3))
    return out


CASES = _cases()

# inputs the split kernels must refuse (LBBNN_E_ALIGN = -3): the eligible width in the two ineligible layouts
SPLIT_REJECTED = [dict(B=96, I=32, O=84, ldx=36, x_aligned=False), dict(B=96, I=32, O=84, ldx=33, x_aligned=True)]

# lbbnn_matmul_splitk (mean-only bf16x3 with kchunk): planned at I = 200, kchunk = 64 (four slabs, the last a K tail of 8)
SPLITK = dict(B=37, I=200, O=84, kchunk=64, variant=_v("split", False, True, True, 3))

# Kernel families of the fan-out / members test (tests/test_vd_ensemble_gpu.py): (name, B, I, O, mode, relu); x is dense
# (ldx = I) and aligned there.  FAMILY_VARIANTS: the fan-out instantiation each row reaches.
FAMILIES = [
    ("fp32 register-staged", 33, 50, 37, "fp32", True),           # x rows not float4-aligned
    ("fp32 register-staged, I % 16 != 0", 70, 36, 120, "fp32", False),
    ("fp32 register-staged, large tile, scalar x", 1921, 18, 1201, "fp32", True),
    ("fp32 register-staged, large tile, vector x", 1921, 20, 1201, "fp32", False),
    ("fp32 LDS-DMA", 100, 784, 120, "fp32", True),
    ("fp32 LDS-DMA, large tile", 2048, 64, 1280, "fp32", False),
    ("bf16x3", 100, 256, 200, "bf16x3", True),
    ("bf16x3, K tail", 45, 200, 120, "bf16x3", False),
    ("bf16x3, large tile", 2048, 64, 1280, "bf16x3", True),
    ("bf16 single", 100, 256, 200, "bf16", True),
    ("bf16 single, large tile", 2048, 64, 1280, "bf16", False),
    ("fp16 single", 100, 256, 200, "fp16", False),
    ("fp16 single, large tile", 2048, 64, 1280, "fp16", True),
    ("skinny O <= 16", 40, 64, 8, "fp32", False),
    ("skinny O <= 16, unaligned rows", 33, 50, 3, "fp32", True),
]

FAMILY_VARIANTS = {
    "fp32 register-staged": _v("staged", False, False, False, fan=True),
    "fp32 register-staged, I % 16 != 0": _v("staged", False, True, False, fan=True),
    "fp32 register-staged, large tile, scalar x": _v("staged", True, False, False, fan=True),
    "fp32 register-staged, large tile, vector x": _v("staged", True, True, False, fan=True),
    "fp32 LDS-DMA": _v("dma", False, True, False, fan=True),
    "fp32 LDS-DMA, large tile": _v("dma", True, True, False, fan=True),
    "bf16x3": _v("split", False, True, False, 3, fan=True),
    "bf16x3, K tail": _v("split", False, True, False, 3, fan=True),
    "bf16x3, large tile": _v("split", True, True, False, 3, fan=True),
    "bf16 single": _v("split", False, True, False, 1, fan=True),
    "bf16 single, large tile": _v("split", True, True, False, 1, fan=True),
    "fp16 single": _v("split", False, True, False, 1, True, fan=True),
    "fp16 single, large tile": _v("split", True, True, False, 1, True, fan=True),
    "skinny O <= 16": _v("skinny", False, True, False, fan=True),
    "skinny O <= 16, unaligned rows": _v("skinny", False, False, False, fan=True),
}
FAN_MEMBERS = 5            # members of the fan-out / members test

# The grid the host tier sweeps the plan over to build the set of reachable instantiations: every threshold of the
# dispatcher from both sides, up to B ~ 4100, I ~ 2100, O ~ 6900.
SWEEP_B = (1, 16, 37, 95, 96, 128, 129, 384, 1920, 1921, 4100)
SWEEP_I = (1, 6, 7, 8, 16, 18, 20, 24, 32, 33, 40, 64, 200, 1000, 1280, 1284, 2100)
SWEEP_O = (1, 3, 16, 17, 80, 81, 84, 1201, 1204, 1280, 6900)
EXPECTED_INSTANTIATIONS = 38
