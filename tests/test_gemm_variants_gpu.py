"""GPU tier of the dual-moment GEMM's variant matrix: every kernel instantiation of csrc/lrt_gemm.hip that a single launch can
reach (tests/gemm_variant_cases.py; the host tier proves the table complete) runs once at the smallest shape that reaches it
and is compared with fp64 of

    out = x e_w^T + b_m + sqrt(x^2 var_w^T * vs + b_v) * eps   (ReLU where set),     std = sqrt(x^2 var_w^T * vs + b_v)

computed from the fp32 source values.  x and the output are views of NaN-filled buffers (row strides I + 4 / O + 4, one extra
row): a K tail or a tile bound that reads or writes one element too far shows as a NaN inside, or as a changed bit outside.
Then the epilogue matrix per family on the small tile (absent operands, ReLU, std_out, in-kernel noise, log-softmax, the
combine form, split-K) and std_out on a 4-byte boundary.  Every line ``GEMMVAR ...`` printed is a measured error."""
import zlib

import pytest
import torch

import gemm_variant_cases as gv
from conftest import elementwise_violation, rel_err

pytestmark = pytest.mark.gpu

NOISE_STREAM, NOISE_ROW0 = 9, 1000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


# ----------------------------------------------------------------------------------------------- inputs and reference
class Problem:
    """fp32 sources of one case on the CPU (seeded by the case), the device operands from the project's own writers, x as a
    view of a NaN-filled buffer in the case's layout."""

    def __init__(self, bnn, dev, B, I, O, mode, layout, key):
        ops = bnn.ops
        g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
        self.B, self.I, self.O, self.mode = B, I, O, mode
        self.x = 2 * torch.rand(B, I, generator=g) - 1
        if mode in ("bf16", "fp16"):            # the single-product forms are variational dropout's: theta, theta^2
            theta = 0.2 * torch.rand(I, O, generator=g) - 0.1
            self.layer = bnn.vd.BayesianLayer(I, O).to(dev)
            with torch.no_grad():
                self.layer.theta.copy_(theta)
            self.ew, self.vw = theta.t().contiguous(), theta.t().contiguous() ** 2
            self.e_w, self.var_w = self.layer._operands(True, mode == "fp16")
        else:
            self.ew = 0.2 * (torch.rand(O, I, generator=g) - 0.5)
            self.vw = 1e-4 * torch.rand(O, I, generator=g)
            split = mode == "bf16x3"
            self.e_w = ops.format_operand(self.ew.to(dev), split=split)
            self.var_w = ops.format_operand(self.vw.to(dev), split=split)
        self.bm = 0.2 * (torch.rand(O, generator=g) - 0.5)
        self.bv = 1e-4 * torch.rand(O, generator=g)
        self.vs = 0.05 + 0.45 * torch.rand(O, generator=g)
        self.eps = torch.randn(B, O, generator=g)
        pad = {"pad4": 4, "offset": 4, "pad3": 3, "odd": 1}[layout]
        c0 = 1 if layout == "offset" else 0
        self.xbuf = torch.full((B + 1, I + pad), float("nan"), device=dev)
        self.xd = self.xbuf[:B, c0:c0 + I]
        self.xd.copy_(self.x)
        assert self.xd.stride(0) == I + pad and (self.xd.data_ptr() % 16 == 0) == (layout != "offset")
        self.dev = dev
        self.d = {k: getattr(self, k).to(dev) for k in ("bm", "bv", "vs", "eps")}

    def plan(self, ops, flags):
        return ops.lrt_gemm_plan(self.B, self.I, self.O, ldx=self.xd.stride(0), x_aligned=self.xd.data_ptr() % 16 == 0,
                                 flags=flags)

    def ref(self, *, mean_only=False, relu=False, bm=True, bv=True, vs=True, eps=None):
        """(out, std) in fp64; eps: (B, O) tensor, default the case's explicit draw."""
        x = self.x.double()
        out = x @ self.ew.double().T
        if bm:
            out = out + self.bm.double()
        std = None
        if not mean_only:
            var = (x ** 2) @ self.vw.double().T
            if vs:
                var = var * self.vs.double()
            if bv:
                var = var + self.bv.double()
            std = torch.sqrt(var)
            out = out + std * (self.eps if eps is None else eps).double().cpu()
        return (torch.relu(out) if relu else out), std

    def launch(self, ops, *, mean_only=False, relu=False, bm=True, bv=True, vs=True, eps="explicit", rng=None,
               log_softmax=False, std_out=None, want_std=True):
        """One ops.lrt_gemm into a NaN-filled (B + 1, O + 4) buffer; returns (out view, std_out, buffer)."""
        B, O = self.B, self.O
        buf = torch.full((B + 1, O + 4), float("nan"), device=self.dev)
        out = buf[:B, :O]
        if std_out is None and want_std and not mean_only:
            std_out = torch.full((B, O), float("nan"), device=self.dev)
        mode = self.mode
        kw = {}
        if not mean_only:
            kw = dict(bias_var=self.d["bv"] if bv else None, var_scale=self.d["vs"] if vs else None,
                      eps=self.d["eps"] if isinstance(eps, str) else eps, rng=rng, rng_stream=NOISE_STREAM,
                      row_offset=NOISE_ROW0, std_out=std_out)
        ops.lrt_gemm(self.xd, self.e_w, self.var_w, I=self.I, O=O, bias_mean=self.d["bm"] if bm else None, relu=relu,
                     mean_only=mean_only, log_softmax=log_softmax, split=mode != "fp32", single=mode in ("bf16", "fp16"),
                     half=mode == "fp16", out=out, **kw)
        torch.cuda.synchronize()
        return out, std_out, buf


def _only_the_view_was_written(buf, B, O):
    """Inside B x O every value is finite; outside it every bit is still the fill's."""
    assert torch.isfinite(buf[:B, :O]).all()
    fill = torch.full((1,), float("nan"), device=buf.device).view(torch.int32)
    bits = buf.clone()
    bits[:B, :O] = float("nan")
    assert bool((bits.view(torch.int32) == fill).all())


def _check(tag, what, got, ref, mode, mean_only):
    """The mode's bar (fp32: the relative bar and the element-wise one); prints the figures before asserting."""
    r = rel_err(got, ref)
    v = elementwise_violation(got, ref)
    print("GEMMVAR %s | %s | %s%s | rel_err %.3e | elementwise %.3f" % (tag, what, mode, " mean-only" if mean_only else "", r, v))
    assert r < gv.BARS[(mode, mean_only)], (tag, what, r)
    if mode == "fp32":
        assert v <= 1, (tag, what, v)


# ----------------------------------------------------------------------------------------------- every instantiation once
@pytest.mark.parametrize("c", gv.CASES, ids=[c.id for c in gv.CASES])
def test_variant_vs_fp64(bnn, dev, c):
    ops = bnn.ops
    p = Problem(bnn, dev, c.B, c.I, c.O, c.mode, c.layout, c.id)
    assert gv.variant_of(p.plan(ops, c.flags)) == c.variant
    out, std, buf = p.launch(ops, mean_only=c.mean_only, relu=c.relu)
    _only_the_view_was_written(buf, c.B, c.O)
    ref, ref_std = p.ref(mean_only=c.mean_only, relu=c.relu)
    _check(c.id, "out", out, ref, c.mode, c.mean_only)
    if not c.mean_only:
        assert torch.isfinite(std).all()
        _check(c.id, "std_out", std, ref_std, c.mode, c.mean_only)


# ----------------------------------------------------------------------------------------------- epilogue matrix, small tile
# (family, I, mode, O): O = 84 / 16 take the float4 stores, 83 / 10 / 3 the scalar ones
EPILOGUE = [("skinny", 20, "fp32", 16), ("skinny", 20, "fp32", 10), ("skinny", 18, "fp32", 3),
            ("staged", 20, "fp32", 84), ("staged", 18, "fp32", 83), ("dma", 48, "fp32", 84), ("dma", 48, "fp32", 83),
            ("split", 40, "bf16x3", 84), ("split", 40, "bf16x3", 83)]
EPI_IDS = ["%s-I%d-O%d" % (f, i, o) for f, i, _, o in EPILOGUE]
EPI_B = 37


@pytest.fixture(scope="module")
def epi(bnn, dev):
    cache = {}

    def get(family, I, mode, O):
        key = (family, I, mode, O)
        if key not in cache:
            p = Problem(bnn, dev, EPI_B, I, O, mode, "pad4", "epilogue-%s-%d-%d" % (family, I, O))
            assert p.plan(bnn.ops, gv.mode_flags(mode, False)).family == family
            cache[key] = (p, p.launch(bnn.ops))                 # the base run: every operand present, explicit eps, no ReLU
        return cache[key]
    return get


@pytest.mark.parametrize("family,I,mode,O", EPILOGUE, ids=EPI_IDS)
@pytest.mark.parametrize("absent", ["bias_mean", "bias_var", "var_scale", "all"])
def test_epilogue_absent_operands(bnn, dev, epi, family, I, mode, O, absent):
    p, (out0, std0, _) = epi(family, I, mode, O)
    tag = "epilogue-%s-I%d-O%d" % (family, I, O)
    on = dict(bm=absent not in ("bias_mean", "all"), bv=absent not in ("bias_var", "all"), vs=absent not in ("var_scale", "all"))
    out, std, buf = p.launch(bnn.ops, **on)
    _only_the_view_was_written(buf, p.B, O)
    ref, ref_std = p.ref(**on)
    _check(tag, "no %s: out" % absent, out, ref, mode, False)
    _check(tag, "no %s: std_out" % absent, std, ref_std, mode, False)
    assert not torch.equal(out, out0)                           # the operand is really read when present
    ref0, ref_std0 = p.ref()
    _check(tag, "all present: out", out0, ref0, mode, False)
    _check(tag, "all present: std_out", std0, ref_std0, mode, False)


@pytest.mark.parametrize("family,I,mode,O", EPILOGUE, ids=EPI_IDS)
def test_epilogue_relu_and_std_out(bnn, dev, epi, family, I, mode, O):
    p, (out0, std0, _) = epi(family, I, mode, O)
    tag = "epilogue-%s-I%d-O%d" % (family, I, O)
    out, std, buf = p.launch(bnn.ops, relu=True)
    _only_the_view_was_written(buf, p.B, O)
    _check(tag, "relu: out", out, p.ref(relu=True)[0], mode, False)
    assert torch.equal(out, torch.relu(out0)) and bool((out0 < 0).any())
    assert torch.equal(std, std0)                               # sqrt(var) is stored before the ReLU
    # without std_out the output is the same bits
    out_n, _, _ = p.launch(bnn.ops, want_std=False)
    assert torch.equal(out_n, out0)
    # mean-only: out = x e_w^T + b_m
    out_m, _, buf_m = p.launch(bnn.ops, mean_only=True)
    _only_the_view_was_written(buf_m, p.B, O)
    _check(tag, "mean-only: out", out_m, p.ref(mean_only=True)[0], mode, True)


@pytest.mark.parametrize("family,I,mode,O", EPILOGUE, ids=EPI_IDS)
def test_epilogue_inkernel_noise(bnn, dev, epi, family, I, mode, O):
    """The in-kernel Philox draw at row_offset = 1000: fp64 with ops.philox_normal's values at the same stream and row base,
    and bitwise the explicit-eps launch of those values -- output and std_out."""
    ops = bnn.ops
    p, (_, std0, _) = epi(family, I, mode, O)
    tag = "epilogue-%s-I%d-O%d" % (family, I, O)
    bnn.manual_seed(77, 5)
    rng = ops.RngState.get(dev).t[:2].clone()
    out, std, buf = p.launch(ops, eps=None, rng=rng)
    _only_the_view_was_written(buf, p.B, O)
    eps = ops.philox_normal(rng, NOISE_STREAM, p.B, O, row_base=NOISE_ROW0)
    assert torch.isfinite(eps).all() and 0.5 < float(eps.std()) < 1.5
    ref, _ = p.ref(eps=eps.cpu())
    _check(tag, "in-kernel noise: out", out, ref, mode, False)
    out_e, std_e, _ = p.launch(ops, eps=eps)
    assert torch.equal(out, out_e)
    assert torch.equal(std, std_e) and torch.equal(std, std0)   # std_out does not depend on the noise or its source


@pytest.mark.parametrize("O,I", [(3, 18), (10, 20), (16, 1284)])
@pytest.mark.parametrize("mean_only", [False, True], ids=["dual", "mean"])
def test_skinny_log_softmax(bnn, dev, O, I, mean_only):
    p = Problem(bnn, dev, EPI_B, I, O, "fp32", "pad4", "log-softmax-%d-%d" % (O, I))
    assert p.plan(bnn.ops, gv.F_LOG_SOFTMAX | (gv.F_MEAN_ONLY if mean_only else 0)).family == "skinny"
    out, std, buf = p.launch(bnn.ops, mean_only=mean_only, log_softmax=True)
    _only_the_view_was_written(buf, p.B, O)
    ref, ref_std = p.ref(mean_only=mean_only)
    tag = "log-softmax-O%d-I%d" % (O, I)
    _check(tag, "out", out, torch.log_softmax(ref, dim=1), "fp32", mean_only)
    if not mean_only:
        _check(tag, "std_out", std, ref_std, "fp32", False)     # the training head: sqrt(var), not the logits


@pytest.mark.parametrize("family,I,mode", [("staged", 18, "fp32"), ("staged", 20, "fp32"), ("dma", 48, "fp32"), ("split", 40, "bf16x3")])
@pytest.mark.parametrize("O", [84, 83])
def test_combine_epilogue(bnn, dev, family, I, mode, O):
    """lbbnn_lrt_gemm_combine: out = comb_add + 2 comb_x (.) (x e_w^T) against fp64; comb_x and comb_add / out are views
    with row stride O + 4 of NaN-filled buffers."""
    ops = bnn.ops
    B = EPI_B
    p = Problem(bnn, dev, B, I, O, mode, "pad4", "combine-%s-%d-%d" % (family, I, O))
    assert p.plan(ops, gv.mode_flags(mode, True)).family == family
    g = torch.Generator().manual_seed(O + I)
    cx, ca = torch.rand(B, O, generator=g), torch.randn(B, O, generator=g)
    xbuf = torch.full((B + 1, O + 4), float("nan"), device=dev)
    abuf = torch.full((B + 1, O + 4), float("nan"), device=dev)
    xbuf[:B, :O] = cx.to(dev)
    abuf[:B, :O] = ca.to(dev)
    got = ops.lrt_gemm_combine(p.xd, p.e_w, K=I, N=O, comb_x=xbuf[:B, :O], comb_add=abuf[:B, :O], split=mode != "fp32")
    torch.cuda.synchronize()
    _only_the_view_was_written(abuf, B, O)
    ref = ca.double() + 2 * cx.double() * (p.x.double() @ p.ew.double().T)
    _check("combine-%s-I%d-O%d" % (family, I, O), "out", got, ref, mode, True)


def test_splitk_slabs_sum_to_product(bnn, dev):
    ops = bnn.ops
    k = gv.SPLITK
    B, I, O, kchunk = k["B"], k["I"], k["O"], k["kchunk"]
    p = Problem(bnn, dev, B, I, O, "bf16x3", "pad4", "splitk")
    plan = ops.lrt_gemm_plan(B, I, O, ldx=p.xd.stride(0), flags=gv.F_MEAN_ONLY | gv.F_SPLIT16, kchunk=kchunk)
    assert gv.variant_of(plan) == k["variant"]
    slabs = ops.matmul_splitk(p.xd, p.e_w, K=I, N=O, kchunk=kchunk)
    torch.cuda.synchronize()
    S = -(-I // kchunk)
    assert slabs.shape == (S, B, O) and torch.isfinite(slabs).all()
    x, w = p.x.double(), p.ew.double()
    _check("splitk-I%d-k%d" % (I, kchunk), "sum of slabs", slabs.double().sum(0), x @ w.T, "bf16x3", True)
    for z in range(S):
        sl = slice(z * kchunk, min((z + 1) * kchunk, I))
        _check("splitk-I%d-k%d" % (I, kchunk), "slab %d" % z, slabs[z], x[:, sl] @ w[:, sl].T, "bf16x3", True)


# ----------------------------------------------------------------------------------------------- std_out on a 4-byte boundary
@pytest.mark.parametrize("family,I,mode,O", [("skinny", 20, "fp32", 16), ("staged", 20, "fp32", 84), ("dma", 48, "fp32", 84),
                                             ("split", 40, "bf16x3", 84)], ids=["skinny", "staged", "dma", "split"])
def test_std_out_one_float_into_a_flat_buffer(bnn, dev, epi, family, I, mode, O):
    """O, ldo, out and eps all allow float4 stores; std_out starts one float into a flat buffer.  The store decision looks at
    std_out's own alignment: its values are right and the guard floats before and after it are untouched; out is unchanged."""
    p, (out0, std0, _) = epi(family, I, mode, O)
    B = p.B
    flat = torch.full((B * O + 2,), float("nan"), device=dev)
    std = flat[1:1 + B * O].view(B, O)
    assert std.data_ptr() % 16 == 4 and std.is_contiguous()
    out, _, buf = p.launch(bnn.ops, std_out=std)
    _only_the_view_was_written(buf, B, O)
    fill = torch.full((1,), float("nan"), device=dev).view(torch.int32)
    guards = flat.view(torch.int32)[[0, B * O + 1]]
    assert bool((guards == fill).all())
    assert torch.isfinite(std).all()
    _check("std-out-misaligned-%s" % family, "std_out", std, p.ref()[1], mode, False)
    assert torch.equal(std, std0) and torch.equal(out, out0)
