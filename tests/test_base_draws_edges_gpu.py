"""GPU tier: the baseline LBBNN's in-kernel draws (K6 / K6b draw mode) and batched ensemble (lbbnn_gate_members) at the shapes,
temperatures and flags where they can go wrong, against references that share no code with the kernels: Philox words
regenerated through the pinned test entry points, torch's RelaxedBernoulli formula in fp64 (base_draw_ref._relaxed, pinned to
torch by tests/test_base_draws_host.py) and fp64 autograd of oracle.lbbnn_oracle.base_forward."""
import numpy as np
import pytest
import torch

from base_draw_ref import (F32, _Alpha32, _chain, _relaxed, _rng, alpha32_ulps, exact_of, gate_clamp_classes, layer_draws,
                           layer_oracle, net_elbo_oracle, net_eval_oracle)
from conftest import rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TIGHT = 5e-6          # fp32 outputs (the bars of tests/test_base_hip_draws_gpu.py and test_base_ensemble_gpu.py)
SPLIT = 2e-5          # bf16x3 outputs; also lp / lq
GRAD = {"fp32": 2e-4, "bf16x3": 5e-4}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture
def temper(bnn):
    old = bnn.distributions.TEMPER_PRIOR

    def set_(t):
        bnn.distributions.TEMPER_PRIOR = t
    yield set_
    bnn.distributions.TEMPER_PRIOR = old


@pytest.fixture
def prec(bnn):
    """Set the process precision for one test, fp32 restored after."""
    def set_(p):
        bnn.set_precision(p)
    yield set_
    bnn.set_precision("fp32")


def _net(bnn, dev, dims, hard, seed=0, lam=2.5):
    torch.manual_seed(seed)
    net = bnn.base.BayesianNetwork(dims).to(dev)
    with torch.no_grad():
        for l in (net.l1, net.l2, net.l3):
            if lam:
                l.lambdal.uniform_(-lam, lam)
            l.gamma.exact = hard
    return net


def _layers(net):
    return (net.l1, net.l2, net.l3)


# ============================================================================================== A. layer draw path vs fp64
A_SHAPES = [(1, 1, 1), (7, 37, 300), (64, 784, 600), (16, 1030, 513), (4, 4100, 40)]
A_CASES = [(s, reg, lam, "fp32", ()) for s in A_SHAPES for reg in ("T0.5", "T0.001", "hard") for lam in ("unit", "wide")]
A_CASES += [((64, 784, 600), reg, lam, "bf16x3", ()) for reg in ("T0.5", "T0.001", "hard") for lam in ("unit", "wide")]
A_CASES += [((7, 37, 300), "T0.5", "unit", "fp32", (e,)) for e in ("weight_prior", "bias_prior", "gamma_prior")]
A_CASES += [((4099, 64, 40), "T0.5", "unit", p, ()) for p in ("fp32", "bf16x3")]


def _a_id(c):
    (B, I, O), reg, lam, p, ex = c
    return "%dx%dx%d-%s-%s-%s%s" % (B, I, O, reg, lam, p, "".join("-" + e for e in ex))


@pytest.mark.parametrize("case", A_CASES, ids=[_a_id(c) for c in A_CASES])
def test_layer_draw_step_vs_fp64_autograd(bnn, dev, temper, prec, case):
    (B, I, O), regime, lam, precision, exact = case
    ops = bnn.ops
    assert ops.split_eligible(I, O) == ((I, O) in ((784, 600), (64, 40)))   # the bf16x3 cases are the eligible shapes
    T = 0.001 if regime == "T0.001" else 0.5
    hard = regime == "hard"
    temper(T)
    torch.manual_seed(I * 7 + O)
    layer = bnn.base.BayesianLinear(I, O, 1)
    with torch.no_grad():
        if lam == "wide":
            layer.lambdal.uniform_(-8, 8)          # (the default U(0, 1) keeps alpha in (0.5, 0.73): no clamp of alpha)
    layer = layer.to(dev).train()
    layer.gamma.exact = hard
    for e in exact:
        getattr(layer, e).exact = True
    L = layer._layer_id
    x = torch.rand(B, I, generator=torch.Generator().manual_seed(B + I)).to(dev).requires_grad_(True)
    rng = _rng(dev, 2024 + O, 17 + I)
    prec(precision)
    out, lp, lq = layer.sample_forward(x, rng=rng)
    ((out ** 2).sum() + (lq - lp) / 600).backward()
    prec("fp32")
    # the Gamma precisions: element 0 of the tau_w stream and element o of the tau_b stream, over the rates -- bit for bit
    assert torch.equal(layer.tau_w, ops.philox_std_gamma(rng, ops.STREAM_GAMMA_W * 64 + L, layer.weight_a, layer.weight_b))
    assert torch.equal(layer.tau_b, ops.philox_std_gamma(rng, ops.STREAM_GAMMA_B * 64 + L, layer.bias_a, layer.bias_b))
    d = layer_draws(ops, layer, rng, T)        # every draw regenerated; the oracle never sees the layer's own copies
    assert alpha32_ulps(layer.alpha, layer.lambdal) <= 4      # two roundings of expf and the division: a few ulps
    P64 = {n: getattr(layer, n).detach().double().cpu().requires_grad_(True) for n in layer._names}
    x64 = x.detach().double().cpu().requires_grad_(True)
    alpha = layer.alpha.double().cpu()
    hard_g = (d["u"] < alpha).double() if hard else None
    o, lp64, lq64, cg = layer_oracle(x64, P64, d, T, hard_g, exact_of(layer), alpha32=layer.alpha)
    ((o ** 2).sum() + (lq64 - lp64) / 600).backward()
    g_k = layer.gammas.double().cpu()
    inside, outside = gate_clamp_classes(alpha, d["u"], T)
    if hard:
        assert torch.equal(g_k, hard_g)
    else:
        # fp32 logit sum: a few ulps of each of its four terms, times 1/T, times dc/dz = c (1 - c); plus an ulp of the clamp
        c = cg.detach()
        p, uc = alpha.clamp(F32.eps, 1 - F32.eps), d["u"].clamp(F32.eps, 1 - F32.eps)
        terms = uc.log().abs() + (-uc).log1p().abs() + p.log().abs() + (-p).log1p().abs()
        bound = c * (1 - c) * 8 * F32.eps * terms / T + 2 * F32.eps
        assert bool(((g_k - c).abs() <= bound).all()), float(((g_k - c).abs() / bound).max())
        assert torch.equal(g_k[outside], c[outside])          # beyond a clamp: the clamp constants exactly
    assert rel_err(out, o) < (TIGHT if precision == "fp32" else SPLIT)
    assert rel_err(lp, lp64) < SPLIT and rel_err(lq, lq64) < SPLIT
    tol = GRAD[precision]
    assert rel_err(x.grad, x64.grad) < tol
    for name, prm in layer.named_parameters():
        assert P64[name].grad is not None, name
        if name == "lambdal" and regime == "T0.001":
            continue
        assert rel_err(prm.grad, P64[name].grad) < tol, name
    if regime != "T0.001":
        return
    # d lambdal element by element: where the gate is inside its clamps (and near them, where the fp32 and fp64 sides may
    # differ) the full fp64 autograd gradient; beyond a clamp the Bernoulli log_prob term alone, al (1 - al) d lq / d al
    g_l = layer.lambdal.grad.double().cpu()
    lam64 = P64["lambdal"].detach().clone().requires_grad_(True)
    (orc.bernoulli_log_prob(cg.detach(), _Alpha32.apply(lam64, alpha), layer.gamma.exact) / 600).backward()
    rest = ~outside
    if rest.any():
        assert rel_err(g_l[rest], P64["lambdal"].grad[rest]) < tol
    if outside.any():
        assert rel_err(g_l[outside], lam64.grad[outside]) < tol
    if O * I >= 10000:
        assert int(inside.sum()) >= 20, int(inside.sum())     # not vacuous: gates that carry the 1/T derivative


# ============================================================================================== B. network, default T
@pytest.mark.parametrize("hard", [False, True], ids=["relaxed", "hard"])
def test_network_lambdal_grad_vs_differentiable_torch_path(bnn, dev, hard):
    ops = bnn.ops
    T = bnn.distributions.TEMPER_PRIOR
    assert T == 0.001
    torch.manual_seed(0)
    net = bnn.base.BayesianNetwork().to(dev).train()
    layers = _layers(net)
    for l in layers:
        l.gamma.exact = hard
    g = torch.Generator().manual_seed(5)
    x = torch.rand(100, 1, 28, 28, generator=g).to(dev)
    y = torch.randint(0, 10, (100,), generator=g).to(dev)
    st = ops.RngState.get(dev)
    rng0 = st.t[:2].clone()
    loss_h, lp_h, lq_h, nll_h = net.sample_elbo(x, y, draws="hip")
    loss_h.backward()
    names = ("weight_mu", "weight_rho", "bias_mu", "bias_rho", "pa", "pb", "lambdal")
    gh = [{n: getattr(l, n).grad.clone() for n in names} for l in layers]
    us = []
    for l in layers:
        O, I, L = l.out_features, l.in_features, l._layer_id
        l.noise = {"eps_w": ops.philox_normal(rng0, ops.STREAM_EPS_W * 64 + L, O, I),
                   "eps_b": ops.philox_normal(rng0, ops.STREAM_EPS_B * 64 + L, 0, O),
                   "tau_w": l.tau_w.clone(), "tau_b": l.tau_b.clone()}
        u = ops.philox_uniform(rng0, ops.STREAM_GATE * 64 + L, O, I)
        us.append(u)
        if hard:
            gm = l.gammas.clone()
            l.gamma.rsample = (lambda gm=gm: gm)
        else:
            l.gamma.rsample = (lambda l=l, u=u: _relaxed(torch.sigmoid(l.lambdal), u, T))    # differentiable gates
    net.zero_grad()
    loss_t, lp_t, lq_t, nll_t = net.sample_elbo(x, y)
    loss_t.backward()
    for h, t, what in ((loss_h, loss_t, "loss"), (lp_h, lp_t, "lp"), (lq_h, lq_t, "lq"), (nll_h, nll_t, "nll")):
        assert rel_err(h.detach(), t.detach()) < SPLIT, what
    for li, l in enumerate(layers):
        for n in names[:-1]:
            assert rel_err(gh[li][n], getattr(l, n).grad) < 5e-4, (li, n)
        a, b = gh[li]["lambdal"].double().cpu(), l.lambdal.grad.double().cpu()
        if hard:
            assert rel_err(a, b) < 5e-4, li
            continue
        inside, outside = gate_clamp_classes(torch.sigmoid(l.lambdal.detach().double().cpu()), us[li].double().cpu(), T)
        assert int(inside.sum()) >= 20, (li, int(inside.sum()))
        assert rel_err(a[~outside], b[~outside]) < 5e-4, li
        assert rel_err(a[outside], b[outside]) < 5e-4, li
    for l in layers:
        l.noise = None
        del l.gamma.rsample


# ============================================================================================== C. samples > 1
def test_three_samples_are_the_mean_of_three_single_samples(bnn, dev, temper):
    temper(0.5)
    ops = bnn.ops
    net = _net(bnn, dev, (200, 64, 48, 10), False, seed=3).train()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(32, 200, generator=g).to(dev)
    y = torch.randint(0, 10, (32,), generator=g).to(dev)
    st = ops.RngState.get(dev)
    ops.manual_seed(17, 40)
    r3 = net.sample_elbo(x, y, 3, draws="hip")
    r3[0].backward()
    assert int(st.t[1]) == 43
    g3 = {n: p.grad.clone() for n, p in net.named_parameters()}
    ops.manual_seed(17, 40)
    vals, grads = [], []
    for _ in range(3):
        net.zero_grad()
        r = net.sample_elbo(x, y, 1, draws="hip")
        r[0].backward()
        vals.append([t.detach().double() for t in r])
        grads.append({n: p.grad.double().clone() for n, p in net.named_parameters()})
    assert int(st.t[1]) == 43
    for k, what in enumerate(("loss", "log_prior", "log_q", "nll")):
        mean = sum(v[k] for v in vals) / 3
        assert rel_err(r3[k].detach(), mean) < 1e-6, what
    for n in g3:
        assert rel_err(g3[n], sum(gr[n] for gr in grads) / 3) < 1e-6, n


# ============================================================================================== D. every members width
D_NETS = [(1096, 300, 37, 10), (4096, 2049, 600, 10)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("hard", [True, False], ids=["hard", "relaxed"])
@pytest.mark.parametrize("dims", D_NETS, ids=["ld1120", "ld4096"])
def test_ensemble_at_every_gate_members_width(bnn, dev, temper, prec, dims, hard, precision):
    ops = bnn.ops
    temper(0.5)
    lds = [ops.operand_ld(d) for d in dims[:3]]
    assert 1024 < max(lds) <= 2048 or max(lds) == 4096            # gate_members_kernel<2> and <4>
    assert {d % 4 == 0 for d in dims[:3]} == {True, False}       # vector and scalar loads in one launch
    assert ops.split_eligible(dims[0], dims[1]) and not ops.split_eligible(dims[1], dims[2])
    net = _net(bnn, dev, dims, hard, seed=11)
    B, S = 6, 3
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(12)).to(dev)
    prec(precision)
    ops.manual_seed(13, 40)
    st = ops.RngState.get(dev)
    r = bnn.evaluate.base_ensemble(net, x, S, keep_gates=True)
    assert int(st.t[1]) == 40 + S
    for m in range(S):
        rng = _rng(dev, 13, 40 + m)
        with torch.no_grad():
            ref = _chain(net, x, rng)
        assert torch.equal(r["outputs"][m], ref), (m, float((r["outputs"][m] - ref).abs().max()))
        for k, l in enumerate(_layers(net)):
            gk = r["gates"][k][m]
            assert torch.equal(gk, l.gammas), (m, k)                # the chain just drew them at this offset
            u = ops.philox_uniform(rng, ops.STREAM_GATE * 64 + l._layer_id, l.out_features, l.in_features)
            if hard:
                assert torch.equal(gk, (u < l.alpha).float())
            else:
                assert float((gk - _relaxed(l.alpha, u, 0.5)).abs().max()) < 1e-4
            assert float((r["gate_rows"][k][m].double() - gk.double().sum(1)).abs().max()) < 1e-3
    h64 = net_eval_oracle(ops, net, x, _rng(dev, 13, 40), [r["gates"][k][0] for k in range(3)])
    assert rel_err(r["outputs"][0], h64) < (TIGHT if precision == "fp32" else SPLIT)


# ============================================================================================== E. the C API
E_SPECS = [(37, 29, False), (1096, 40, True), (300, 17, False), (64, 300, True)]     # (I, O, split): ld 64, 1120, 320, 64


def _split_decode(buf, O, ld):
    """(S, O, ld) fp32-sized split buffer -> (hi, lo) as (S, O, ld) bf16 values in fp64 (lbbnn_device.h split_hi_index)."""
    w = buf.view(torch.int16).cpu().numpy().view(np.uint16)                 # (S, O, 2 ld)
    k = np.arange(ld)
    at = (k >> 5) * 64 + ((k >> 3) & 3) * 16 + (k & 7)
    hi, lo = w[:, :, at], w[:, :, at + 8]
    f = lambda h: torch.from_numpy((h.astype(np.uint32) << 16).view(np.float32).astype(np.float64))
    return f(hi), f(lo)


@pytest.mark.parametrize("mode", ["hard", "relaxed", "mpm"])
def test_gate_members_c_api_descriptor_counts(bnn, dev, temper, mode):
    ops, lib = bnn.ops, bnn._lib
    T = 0.5
    temper(T)
    torch.manual_seed(21)
    layers = []
    for I, O, split in E_SPECS:
        l = bnn.base.BayesianLinear(I, O, 1).to(dev)
        with torch.no_grad():
            l.lambdal.uniform_(-2.5, 2.5)
        l.gamma.exact = mode == "hard"
        assert ops.split_eligible(I, O) == split
        layers.append(l)
    S, seed, off = 3, 31, 7
    rng = _rng(dev, seed, off)
    gates = ops.GATES_MPM if mode == "mpm" else ops.GATES_SAMPLE

    def launch(idx):
        descs = (lib.GateMemberDesc * len(idx))()
        bufs = [layers[j]._fill_member_desc(descs[k], S, E_SPECS[j][2], rows=True, keep_gates=True) for k, j in enumerate(idx)]
        for b in bufs:
            for t in b.values():
                t.fill_(float("nan"))
        lib.check(lib.lib().lbbnn_gate_members(descs, len(idx), S, gates, T, rng.data_ptr(), 1, ops._stream()),
                  "lbbnn_gate_members")
        return bufs
    single = [launch([j])[0] for j in range(4)]
    for idx in ([1, 0], [0, 1, 2, 3], [3, 2, 1, 0]):
        for k, b in zip(idx, launch(idx)):
            for n in ("w", "bias", "rows", "gates"):
                assert torch.equal(b[n].view(torch.int32), single[k][n].view(torch.int32)), (idx, k, n)
    for j, (I, O, split) in enumerate(E_SPECS):
        l, b = layers[j], single[j]
        ld = ops.operand_ld(I)
        P = {n: getattr(l, n).detach().double().cpu() for n in ("weight_mu", "weight_rho", "bias_mu", "bias_rho")}
        sg, sb = orc.sigma_of(P["weight_rho"]), orc.sigma_of(P["bias_rho"])
        alpha = torch.sigmoid(l.lambdal.detach()).double().cpu()
        for m in range(S):
            rm = _rng(dev, seed, off + m)
            L = l._layer_id
            ew = ops.philox_normal(rm, ops.STREAM_EPS_W * 64 + L, O, I).double().cpu()
            eb = ops.philox_normal(rm, ops.STREAM_EPS_B * 64 + L, 0, O).double().cpu()
            gk = b["gates"][m].double().cpu()
            if mode == "mpm":
                far = (alpha - 0.5).abs() > 1e-6
                assert torch.equal(gk[far], (alpha > 0.5).double()[far])
            else:
                u = ops.philox_uniform(rm, ops.STREAM_GATE * 64 + L, O, I).double().cpu()
                if mode == "hard":
                    far = (u - alpha).abs() > 1e-6
                    assert torch.equal(gk[far], (u < alpha).double()[far])
                else:
                    assert float((gk - _relaxed(alpha, u, T)).abs().max()) < 1e-4
            assert float((b["rows"][m].double().cpu() - gk.sum(1)).abs().max()) < 1e-3
            ref = gk * (P["weight_mu"] + sg * ew)
            scale = P["weight_mu"].abs() + (sg * ew).abs()
            if split:
                hi, lo = _split_decode(b["w"], O, ld)
                assert (hi[m, :, I:] == 0).all() and (lo[m, :, I:] == 0).all()
                # hi + lo keeps 16 of fp32's 24 significand bits: within 2^-15 of the magnitude
                assert float(((hi[m, :, :I] + lo[m, :, :I]) - ref).abs().sub(2.0 ** -15 * scale).max()) <= 0
            else:
                w = b["w"][m].double().cpu()
                assert (w[:, I:] == 0).all()
                assert float(((w[:, :I] - ref).abs() - 4 * 2.0 ** -23 * scale).max()) <= 0
            bias_ref, b_scale = P["bias_mu"] + sb * eb, P["bias_mu"].abs() + (sb * eb).abs()
            assert float(((b["bias"][m].double().cpu() - bias_ref).abs() - 4 * 2.0 ** -23 * b_scale).max()) <= 0


# ============================================================================================== F. many members, batches, inputs, heads
@pytest.mark.parametrize("dims", [(50, 37, 29, 3), (784, 400, 600, 10)], ids=["50-37-29-3", "784-400-600-10"])
def test_two_hundred_members_in_one_launch(bnn, dev, temper, dims):
    temper(0.5)
    ops, ev = bnn.ops, bnn.evaluate
    net = _net(bnn, dev, dims, False, seed=23)
    x = torch.rand(4, dims[0], generator=torch.Generator().manual_seed(24)).to(dev)
    S = 200
    ops.manual_seed(25, 3)
    r = ev.base_ensemble(net, x, S)
    ops.manual_seed(25, 3)
    r7 = ev.base_ensemble(net, x, S, max_members=7)
    assert torch.equal(r["outputs"], r7["outputs"])
    for k in range(3):
        assert torch.equal(r["gate_rows"][k], r7["gate_rows"][k]), k
    for m in (0, 127, 128, 129, 199):
        with torch.no_grad():
            ref = _chain(net, x, _rng(dev, 25, 3 + m))
        assert torch.equal(r["outputs"][m], ref), m
        for k, l in enumerate(_layers(net)):
            assert float((r["gate_rows"][k][m].double() - l.gammas.double().sum(1)).abs().max()) < 1e-3, (m, k)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B", [1, 4099])
def test_ensemble_batch_edges(bnn, dev, temper, prec, B, precision):
    temper(0.5)
    ops = bnn.ops
    dims = (96, 64, 40, 10)
    net = _net(bnn, dev, dims, False, seed=27)
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(B)).to(dev)
    prec(precision)
    ops.manual_seed(29, 0)
    r = bnn.evaluate.base_ensemble(net, x, 3, keep_gates=True)
    for m in range(3):
        with torch.no_grad():
            assert torch.equal(r["outputs"][m], _chain(net, x, _rng(dev, 29, m))), m
    h64 = net_eval_oracle(ops, net, x, _rng(dev, 29, 0), [r["gates"][k][0] for k in range(3)])
    assert rel_err(r["outputs"][0], h64) < (TIGHT if precision == "fp32" else SPLIT)


@pytest.mark.parametrize("layout", ["misaligned", "strided"])
def test_awkward_inputs_under_bf16x3(bnn, dev, temper, prec, layout):
    temper(0.5)
    ops = bnn.ops
    dims, B = (96, 64, 40, 10), 9
    net = _net(bnn, dev, dims, False, seed=31)
    g = torch.Generator().manual_seed(32)
    if layout == "misaligned":
        x = torch.rand(B * 96 + 1, generator=g).to(dev)[1:].view(B, 96)
        assert x.data_ptr() % 16 != 0
    else:
        x = torch.rand(B, 99, generator=g).to(dev)[:, :96]
        assert x.stride(0) % 4 != 0
    prec("bf16x3")
    ops.manual_seed(33, 0)
    r = bnn.evaluate.base_ensemble(net, x, 3, keep_gates=True)
    for m in range(3):
        with torch.no_grad():
            assert torch.equal(r["outputs"][m], _chain(net, x, _rng(dev, 33, m))), m
    h64 = net_eval_oracle(ops, net, x, _rng(dev, 33, 0), [r["gates"][k][0] for k in range(3)])
    assert rel_err(r["outputs"][0], h64) < SPLIT


@pytest.mark.parametrize("dims", [(50, 37, 29, 20), (784, 400, 600, 20)], ids=["50-37-29-20", "784-400-600-20"])
def test_heads_wider_than_sixteen_classes(bnn, dev, temper, dims):
    temper(0.5)
    ops = bnn.ops
    net = _net(bnn, dev, dims, False, seed=35).train()
    g = torch.Generator().manual_seed(36)
    B = 12
    x = torch.rand(B, dims[0], generator=g).to(dev)
    y = torch.randint(0, dims[-1], (B,), generator=g).to(dev)
    # the training step against fp64 autograd on the regenerated draws
    ops.manual_seed(37, 5)
    loss, lp, lq, nll = net.sample_elbo(x, y, draws="hip", num_batches=600)
    loss.backward()
    l64, lp64, lq64, nll64, P = net_elbo_oracle(ops, net, x, y, _rng(dev, 37, 5), 0.5, 600)
    l64.backward()
    for a, b, what in ((loss, l64, "loss"), (lp, lp64, "lp"), (lq, lq64, "lq"), (nll, nll64, "nll")):
        assert rel_err(a.detach(), b.detach()) < SPLIT, what
    for k, l in enumerate(_layers(net)):
        for n in l._names:
            assert rel_err(getattr(l, n).grad, P[k][n].grad) < GRAD["fp32"], (k, n)
    # the ensemble: members bitwise the chain, chunking changes no bit, member 0 against the oracle
    net.eval()
    S = 5
    ops.manual_seed(39, 0)
    r = bnn.evaluate.base_ensemble(net, x, S, keep_gates=True)
    assert r["outputs"].shape == (S, B, dims[-1])
    for m in range(S):
        with torch.no_grad():
            assert torch.equal(r["outputs"][m], _chain(net, x, _rng(dev, 39, m))), m
    ops.manual_seed(39, 0)
    r2 = bnn.evaluate.base_ensemble(net, x, S, max_members=2)
    assert torch.equal(r2["outputs"], r["outputs"])
    h64 = net_eval_oracle(ops, net, x, _rng(dev, 39, 0), [r["gates"][k][0] for k in range(3)])
    assert rel_err(r["outputs"][0], h64) < TIGHT


# ============================================================================================== G. layers wider than 4096
def test_ensemble_of_a_network_wider_than_gate_members(bnn, dev, temper):
    temper(0.5)
    ops, ev = bnn.ops, bnn.evaluate
    dims = (4100, 64, 48, 10)
    assert ops.operand_ld(dims[0]) > ops.GATE_MEMBERS_MAX_LD
    net = _net(bnn, dev, dims, False, seed=41)
    B, S = 5, 3
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(42)).to(dev)
    st = ops.RngState.get(dev)
    ops.manual_seed(43, 10)
    r = ev.base_ensemble(net, x, S, keep_gates=True)
    assert set(r) == {"outputs", "gate_rows", "gates"}
    assert int(st.t[1]) == 10 + S
    assert r["outputs"].shape == (S, B, 10)
    for l in _layers(net):
        assert l.log_prior == 0 and l.log_variational_posterior == 0
    for m in range(S):
        rng = _rng(dev, 43, 10 + m)
        with torch.no_grad():
            assert torch.equal(r["outputs"][m], _chain(net, x, rng)), m
        for k, l in enumerate(_layers(net)):
            assert torch.equal(r["gates"][k][m], l.gammas)
            u = ops.philox_uniform(rng, ops.STREAM_GATE * 64 + l._layer_id, l.out_features, l.in_features)
            assert float((r["gates"][k][m] - _relaxed(l.alpha, u, 0.5)).abs().max()) < 1e-4
            assert float((r["gate_rows"][k][m].double() - l.gammas.double().sum(1)).abs().max()) < 1e-3
    h64 = net_eval_oracle(ops, net, x, _rng(dev, 43, 10), [r["gates"][k][0] for k in range(3)])
    assert rel_err(r["outputs"][0], h64) < TIGHT
    ops.manual_seed(43, 10)
    assert torch.equal(ev.base_ensemble(net, x, S, max_members=2)["outputs"], r["outputs"])
    ops.manual_seed(43, 10)
    assert torch.equal(ev.ensemble_forward(net, x, S, batched=False), r["outputs"])
    assert int(st.t[1]) == 10 + S
    assert torch.equal(net.sample_predict(x, rng=_rng(dev, 43, 11)), r["outputs"][1])
    res = ev.ensemble_eval(net, x, None, S)
    assert res["outputs"].shape == (S, B, 10) and res["density"].shape == (S,)
    with pytest.raises(ValueError, match="mpm"):
        ev.base_ensemble(net, x, S, gates="mpm")
