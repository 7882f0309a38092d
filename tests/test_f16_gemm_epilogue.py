"""GPU tier: the epilogue of the row-scaled fp16 moment GEMM (lrt_gemm_f16.hip) with its operands staged once per workgroup.

The per-feature constants (bias_mean, bias_var, var_scale x wvar_scale, mean_scale) and the head fold's weight fragments
reach the epilogue through an image in the K-step buffer that is idle during the last step; the noise may be drawn ahead
of the K loop.  What can go wrong is an index, a fill value, a tail or a race -- so the cases are the shapes at which the
kernel takes another path (one K step, two, many; o tiles with a partial last one; O no multiple of 80, 16 or 4; a B tail;
both tile configurations; x as fp32 rows and as planes; one and three variance products), checked
  * against fp64 formed from the same operands at the bars of tests/test_f16_gemm.py (restated below), and
  * bit for bit between calls that must agree: in-kernel noise against the same draws handed in, an omitted optional array
    against an explicit array of its fill value, misaligned per-feature vectors against aligned ones, a folded head
    against its launch-plan replay.
"fp16x3f" (one variance product) is held to its fp64 bar where the format applies it, rows of at least
ops.F16_VAR1_MIN_I weights; the bitwise checks run both forms at every shape."""
import pytest
import torch

from conftest import elementwise_violation, rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

BARS = {"fp16x3": (2e-6, 1e-6), "fp16x3f": (4e-5, 3e-5)}      # tests/test_f16_gemm.py: (max-norm bar, atol fraction)

SHAPES = [(128, 32, 80),        # one K step: the image goes to the buffer no step ever used
          (128, 64, 80),        # two K steps
          (257, 288, 168),      # three o tiles, the last partial; a B tail; I >= 256: the 3 + 1 form applies
          (37, 96, 40), (64, 40, 17), (1, 8, 24)]   # O no multiple of 80 / 16 / 4, the small-tile kernel, a K tail
PRECS = ["fp16x3", "fp16x3f"]
VAR1_MIN_I = 256                # ops.F16_VAR1_MIN_I: shorter rows keep three variance products under "fp16x3f" (layers._split):
# the single product's 2^-12 roundings average out as 1 / sqrt(I) and sit above the bar on short rows (tools/gemm16_fuzz.py)
FP64_CASES = [(B, I, O, prec) for (B, I, O) in SHAPES for prec in PRECS if prec == "fp16x3" or I >= VAR1_MIN_I]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


_CASES = {}


def _case(bnn, dev, B, I, O, prec):
    """Operands of one (shape, form), made once and left unchanged: K1's row-scaled fp16 operands, x as rows and as planes,
    the fp64 operands they came from, a per-feature var_scale of exact powers of two and explicit draws."""
    key = (B, I, O, prec)
    if key in _CASES:
        return _CASES[key]
    ops = bnn.ops
    g = torch.Generator().manual_seed(1000 * B + 10 * I + O)
    x = torch.rand(B, I, generator=g)
    p = orc.init_mnf_params(I, O, g)
    z = 1 + 0.1 * torch.randn(I, generator=g)
    d = {k: v.to(dev) for k, v in p.items()}
    ld = ops.operand_ld(I)
    ws = {"e_w": torch.empty(O, ld, device=dev), "var_w": torch.empty(O, ld, device=dev), "bias_var": torch.empty(O, device=dev),
          "e_scale": torch.empty(O, device=dev), "v_scale": torch.empty(O, device=dev)}
    ops.weight_pass(d["weight_mu"], d["weight_rho"], d["lambdal"], z_fwd=z.to(dev), bias_rho=d["bias_rho"],
                    priors=bnn.Priors(), e_w=ws["e_w"], var_w=ws["var_w"], bias_var=ws["bias_var"],
                    split=3 if prec == "fp16x3f" else 2, e_scale=ws["e_scale"], v_scale=ws["v_scale"])
    alpha = orc.alpha_of(p["lambdal"].double()); sigma = orc.sigma_of(p["weight_rho"].double())
    xd = x.to(dev)
    c = {"x": {"f32": xd, "planes": ops.format_x(xd)}, "x64": x.double(), "ws": ws, "bias_mu": d["bias_mu"],
         "ew": p["weight_mu"].double() * alpha * z.double(), "vw": sigma ** 2 * alpha ** 2,
         "bm64": p["bias_mu"].double(), "bv64": orc.sigma_of(p["bias_rho"].double()) ** 2,
         "vscale": (2.0 ** torch.randint(-2, 3, (O,), generator=g).float()).to(dev),
         "eps": torch.randn(B, O, generator=g).to(dev)}
    _CASES[key] = c
    return c


def _gemm(bnn, c, prec, xsrc, I, O, **kw):
    ws = c["ws"]
    kw.setdefault("bias_mean", c["bias_mu"])
    kw.setdefault("bias_var", ws["bias_var"])
    e_scale, v_scale = kw.pop("e_scale", ws["e_scale"]), kw.pop("v_scale", ws["v_scale"])
    return bnn.ops.lrt_gemm16(c["x"][xsrc], ws["e_w"], ws["var_w"], e_scale, v_scale, I=I, O=O,
                              var1=(prec == "fp16x3f"), x_planes=(xsrc == "planes"), **kw)


@pytest.mark.parametrize("B,I,O,prec", FP64_CASES)
@pytest.mark.parametrize("xsrc", ["f32", "planes"])
def test_epilogue_vs_fp64(bnn, dev, B, I, O, prec, xsrc):
    """mean + sqrt(var) eps with every per-feature array present (var_scale included), ReLU off and on, against fp64."""
    assert bnn.ops.F16_VAR1_MIN_I == VAR1_MIN_I
    c = _case(bnn, dev, B, I, O, prec)
    x64 = c["x64"]
    var = ((x64 ** 2) @ c["vw"].T) * c["vscale"].cpu().double() + c["bv64"]
    ref = x64 @ c["ew"].T + c["bm64"] + var.sqrt() * c["eps"].cpu().double()
    bar, atol = BARS[prec]
    for relu in (False, True):
        out, _ = _gemm(bnn, c, prec, xsrc, I, O, var_scale=c["vscale"], eps=c["eps"], relu=relu)
        r = ref.clamp_min(0) if relu else ref
        e = rel_err(out, r)
        v = elementwise_violation(out, r, rtol=1e-4, atol_frac=atol)
        print("B %d I %d O %d %s %s relu %d: rel err %.3e (bar %.1e), element-wise %.3f" % (B, I, O, prec, xsrc, relu, e, bar, v))
        assert e < bar, e
        assert v <= 1.0, v


@pytest.mark.parametrize("B,I,O", SHAPES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("xsrc", ["f32", "planes"])
def test_in_kernel_noise_equals_the_same_draws_handed_in(bnn, dev, B, I, O, prec, xsrc):
    """rng (nonzero offset, stream and row offset) == eps = philox_normal(...), bit for bit: out with ReLU off and on,
    std_out, the planes with and without the fp32 copy."""
    ops = bnn.ops
    c = _case(bnn, dev, B, I, O, prec)
    rng = torch.tensor([4321, 9, 0, 0], dtype=torch.int64, device=dev)
    stream, row0 = 7, 13
    eps = ops.philox_normal(rng, stream, B, O, row0)
    kr = dict(rng=rng, rng_stream=stream, row_offset=row0, var_scale=c["vscale"])
    ke = dict(eps=eps, var_scale=c["vscale"])
    for relu in (False, True):
        std_r, std_e = torch.empty(B, O, device=dev), torch.empty(B, O, device=dev)
        out_r, _ = _gemm(bnn, c, prec, xsrc, I, O, relu=relu, std_out=std_r, **kr)
        out_e, _ = _gemm(bnn, c, prec, xsrc, I, O, relu=relu, std_out=std_e, **ke)
        assert torch.equal(out_r, out_e), relu
        assert torch.equal(std_r, std_e), relu
        assert bool((out_r != 0).any())
    if O % 8 == 0:
        pl = [torch.zeros(B, ops.plane_ld(O), device=dev) for _ in range(3)]
        out_r, _ = _gemm(bnn, c, prec, xsrc, I, O, relu=True, out_planes=pl[0], **kr)
        none, _ = _gemm(bnn, c, prec, xsrc, I, O, relu=True, out_planes=pl[1], want_out=False, **kr)
        _gemm(bnn, c, prec, xsrc, I, O, relu=True, out_planes=pl[2], want_out=False, **ke)
        assert none is None
        assert torch.equal(pl[0], ops.format_x(out_r)) and torch.equal(pl[1], pl[0]) and torch.equal(pl[2], pl[0])


@pytest.mark.parametrize("B,I,O", SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_omitted_arrays_equal_explicit_fill_values(bnn, dev, B, I, O, prec):
    """bias_mean / bias_var / var_scale left out one at a time == an explicit array of the fill value (0, 0, 1), bitwise."""
    c = _case(bnn, dev, B, I, O, prec)
    zeros, ones = torch.zeros(O, device=dev), torch.ones(O, device=dev)
    base = dict(bias_mean=c["bias_mu"], bias_var=c["ws"]["bias_var"], var_scale=c["vscale"], eps=c["eps"])
    for name, fill in (("bias_mean", zeros), ("bias_var", zeros), ("var_scale", ones)):
        for xsrc in ("f32", "planes"):
            std_a, std_b = torch.empty(B, O, device=dev), torch.empty(B, O, device=dev)
            a, _ = _gemm(bnn, c, prec, xsrc, I, O, std_out=std_a, **dict(base, **{name: None}))
            b, _ = _gemm(bnn, c, prec, xsrc, I, O, std_out=std_b, **dict(base, **{name: fill}))
            assert torch.equal(a, b), (name, xsrc)
            assert torch.equal(std_a, std_b), (name, xsrc)


@pytest.mark.parametrize("B,I,O", SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_misaligned_feature_vectors_give_the_same_bits(bnn, dev, B, I, O, prec):
    """Every per-feature vector as a view one float into its buffer (16-B misaligned) == the aligned call, bitwise."""
    c = _case(bnn, dev, B, I, O, prec)
    ws = c["ws"]

    def off1(t):
        buf = torch.empty(O + 5, device=dev)
        buf[1:O + 1] = t
        v = buf[1:O + 1]
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    vec = dict(bias_mean=c["bias_mu"], bias_var=ws["bias_var"], var_scale=c["vscale"], e_scale=ws["e_scale"], v_scale=ws["v_scale"])
    ref, _ = _gemm(bnn, c, prec, "f32", I, O, eps=c["eps"], relu=True, **vec)
    every, _ = _gemm(bnn, c, prec, "f32", I, O, eps=c["eps"], relu=True, **{k: off1(v) for k, v in vec.items()})
    assert torch.equal(every, ref)
    for name in vec:
        one, _ = _gemm(bnn, c, prec, "planes", I, O, eps=c["eps"], relu=True, **dict(vec, **{name: off1(vec[name])}))
        refp, _ = _gemm(bnn, c, prec, "planes", I, O, eps=c["eps"], relu=True, **vec)
        assert torch.equal(one, refp), name


# ------------------------------------------------------------------------------------------------------------- head fold
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dims,B", [((64, 80, 10), 100), ((96, 168, 16), 37), ((300, 100, 3), 200),
                                    ((32, 64, 80, 10), 100), ((40, 96, 168, 16), 37), ((64, 304, 100, 3), 200)])
def test_head_fold_network_folded_unfolded_and_plan(bnn, dev, prec, dims, B, monkeypatch):
    """A hidden layer followed by a <= 16-class head: the forward with the head folded into the GEMM's epilogue against the
    head as its own launch (bar of test_head_fold_equals_the_unfolded_forward), KL bit-identical; and a recorded launch
    plan replays the eager forward bit for bit.  The two-layer networks run whichever path the network's dispatch gives
    them; the three-layer ones (same hidden width and classes behind one more layer) must take the fold, which shows as a
    different arithmetic: not the same bits as the head's own launch."""
    from bnn_amd import graphs, layers as L
    torch.manual_seed(3)
    net = bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
    net.set_precision(prec)
    x = torch.rand(B, dims[0], device=dev)
    res = {}
    for fold in (True, False):
        monkeypatch.setattr(L, "_HEAD_FOLD", fold)
        with torch.no_grad():
            bnn.manual_seed(7, 5)
            out = net(x, sample=True).clone()
            res[fold] = (out, net.kl().clone())
    bar, atol = BARS[prec]
    e = rel_err(res[True][0], res[False][0])
    print("dims %s B %d %s: folded against unfolded %.3e (bar %.1e)" % (dims, B, prec, e, bar))
    assert torch.isfinite(res[True][0]).all()
    assert e < bar, e
    assert elementwise_violation(res[True][0], res[False][0].double(), rtol=1e-4, atol_frac=atol) <= 1.0
    assert torch.equal(res[True][1], res[False][1])
    assert float((res[True][0].exp().sum(dim=1) - 1).abs().max()) < 1e-5
    if len(dims) == 4:
        assert net.l2._split_now >= 2 and net.l3._split_now == 0
        assert not torch.equal(res[True][0], res[False][0])
    monkeypatch.setattr(L, "_HEAD_FOLD", True)
    with torch.no_grad():
        plan = graphs.LaunchPlan(net, x, sample=True)
        bnn.manual_seed(7, 5)
        o, k = plan()
        assert torch.equal(o, res[True][0]) and torch.equal(k, res[True][1])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,I,O,C", [(100, 64, 80, 10), (37, 96, 168, 16), (200, 304, 100, 3)])
def test_head_fold_entry_point_vs_fp64(bnn, dev, prec, B, I, O, C):
    """The fold through the C ABI (so it cannot be skipped by the network's dispatch): log_softmax of the head's moments,
    formed in fp64 from the relu activations the same call returns unfolded, at the format's bar; in-kernel noise in the
    folded call == the same draws handed in."""
    ops = bnn.ops
    c = _case(bnn, dev, B, I, O, prec)
    g = torch.Generator().manual_seed(B + I + O + C)
    ldh = ops.operand_ld(O)
    he = torch.zeros(C, ldh); hv = torch.zeros(C, ldh)
    he[:, :O] = 0.1 * torch.randn(C, O, generator=g)
    hv[:, :O] = 1e-3 * torch.rand(C, O, generator=g)
    hbm, hbv = 0.1 * torch.randn(C, generator=g), 1e-3 * torch.rand(C, generator=g)
    heps = torch.randn(B, C, generator=g)
    rng = torch.tensor([99, 3, 0, 0], dtype=torch.int64, device=dev)
    eps = ops.philox_normal(rng, 5, B, O, 0)
    h1, _ = _gemm(bnn, c, prec, "planes", I, O, eps=eps, relu=True)

    def folded(**noise):
        head = {"e_w": he.to(dev), "var_w": hv.to(dev), "bias_mean": hbm.to(dev), "bias_var": hbv.to(dev), "eps": heps.to(dev),
                "out": torch.empty(B, C, device=dev), "slab": torch.empty(ops.head_slab_floats(B, O), device=dev), "log_softmax": True}
        _gemm(bnn, c, prec, "planes", I, O, relu=True, want_out=False, head=head, **noise)
        return head["out"]

    got = folded(eps=eps)
    h64 = h1.cpu().double()
    logits = h64 @ he[:, :O].double().T + hbm.double() + ((h64 ** 2) @ hv[:, :O].double().T + hbv.double()).sqrt() * heps.double()
    ref = torch.log_softmax(logits, dim=1)
    bar, atol = BARS[prec]
    e = rel_err(got, ref)
    print("B %d I %d O %d C %d %s: folded head against fp64 %.3e (bar %.1e)" % (B, I, O, C, prec, e, bar))
    assert e < bar, e
    assert elementwise_violation(got, ref, rtol=1e-4, atol_frac=atol) <= 1.0
    assert torch.equal(folded(rng=rng, rng_stream=5, row_offset=0), got)
