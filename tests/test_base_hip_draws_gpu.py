"""GPU tier of the baseline LBBNN's in-kernel draws (sample_elbo(draws="hip"), include/lbbnn.h lbbnn_gate_sample_draw /
lbbnn_gate_backward_draw): the uniforms are the documented Philox words, the gates are torch's RelaxedBernoulli of them, the
Gamma draws have the right law and the right reparameterised gradient, the layer's forward and backward match fp64 autograd of
the oracle on the same draws, the network step matches the torch-draw step fed the same draws, and the step captures."""
import math

import numpy as np
import pytest
import torch

from base_draw_ref import F32, _GammaRep, _relaxed, _rng
from conftest import rel_err, sub
from oracle import lbbnn_oracle as orc
import philox_ref

pytestmark = pytest.mark.gpu

TIGHT = 5e-6


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
    """Set distributions.TEMPER_PRIOR for one test (read at call time by the hip draws, as by Bernoulli.rsample)."""
    old = bnn.distributions.TEMPER_PRIOR

    def set_(t):
        bnn.distributions.TEMPER_PRIOR = t
    yield set_
    bnn.distributions.TEMPER_PRIOR = old


# ---------------------------------------------------------------------------------------------------------- 1. uniforms
def test_philox_uniform_bit_exact_vs_numpy(bnn, dev):
    for seed, offset, stream, rows, cols, base in ((0, 0, 8 * 64 + 32, 7, 13, 0), (123456789012, 77, 8 * 64 + 5, 33, 130, 9),
                                                   (-5, 2 ** 33 + 1, 8 * 64 + 63, 4, 4, 1000)):
        got = bnn.ops.philox_uniform(_rng(dev, seed, offset), stream, rows, cols, row_base=base).cpu().numpy()
        g = (cols + 3) // 4
        r = np.arange(rows, dtype=np.uint64)[:, None] + np.uint64(base)
        cg = np.arange(g, dtype=np.uint64)[None, :]
        r, cg = np.broadcast_arrays(r, cg)
        k0, k1 = philox_ref.key_of(seed, offset)
        words = philox_ref.philox4x32_10(r & np.uint64(0xFFFFFFFF), r >> np.uint64(32), cg, np.full(r.shape, stream, np.uint64),
                                         k0, k1)
        bits = np.stack(words, axis=-1).reshape(rows, 4 * g)[:, :cols]
        ref = (((bits >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)
        assert np.array_equal(got, ref), (seed, offset)
        assert got.min() > 0 and got.max() < 1


# ---------------------------------------------------------------------------------------------------------- 2. gates
@pytest.mark.parametrize("T", [0.001, 0.5])
def test_gates_are_relaxed_bernoulli_of_the_uniforms(bnn, dev, temper, T):
    temper(T)
    torch.manual_seed(3)
    layer = bnn.base.BayesianLinear(200, 70, 1).to(dev).train()
    with torch.no_grad():
        layer.lambdal.uniform_(-4, 4)
    x = torch.rand(16, 200, device=dev)
    rng = _rng(dev, 42, 5)
    with torch.no_grad():
        layer.sample_forward(x, rng=rng)
    u = bnn.ops.philox_uniform(rng, bnn.ops.STREAM_GATE * 64 + layer._layer_id, 70, 200)
    alpha = layer.alpha
    assert torch.equal(layer.gamma.alpha, alpha)
    assert float((alpha - 1 / (1 + torch.exp(-layer.lambdal.detach()))).abs().max()) < 1e-6
    ref = _relaxed(alpha, u, T)
    assert float((layer.gammas - ref).abs().max()) < 1e-4
    # the hard gate of gamma.exact
    layer.gamma.exact = True
    with torch.no_grad():
        layer.sample_forward(x, rng=rng)
    assert torch.equal(layer.gammas, (u < layer.alpha).float())


# ---------------------------------------------------------------------------------------------------------- 3. Gamma draws
def _ks_distance(x, cdf):
    """Kolmogorov-Smirnov distance of the sample x from the law whose draws below FLT_MIN are clamped to FLT_MIN (torch's
    Gamma.rsample, and the kernels'): cdf above FLT_MIN, an atom of mass cdf(FLT_MIN) at FLT_MIN, nothing below.  Equal to
    scipy's kstest statistic when no draw is clamped."""
    x = np.sort(x)
    n = len(x)
    F = cdf(x)
    F_left = np.where(x <= F32.tiny, 0.0, F)          # left limit: 0 at the atom
    i = np.arange(1, n + 1)
    return max(float((i / n - F).max()), float((F_left - (i - 1) / n).max()))


@pytest.mark.parametrize("a", [0.05, 0.2, 0.9, 1.0, 1.05, 3.0, 30.0, 1000.0])
@pytest.mark.parametrize("b", [0.5, 2.0])
def test_gamma_draws_kolmogorov_smirnov(bnn, dev, a, b):
    from scipy import stats
    N = 2 ** 20
    at = torch.full((N,), a, device=dev)
    bt = torch.full((N,), b, device=dev)
    x = bnn.ops.philox_std_gamma(_rng(dev, 1000 + int(a * 100), int(b * 10)), bnn.ops.STREAM_GAMMA_B * 64 + 7, at, bt)
    x = x.double().cpu().numpy()
    assert np.isfinite(x).all() and (x > 0).all()
    D = _ks_distance(x, stats.gamma(a, scale=1.0 / b).cdf)
    assert D * math.sqrt(N) < 1.95, (a, b, D * math.sqrt(N))


def test_gamma_draw_bad_shape_is_nan(bnn, dev):
    a = torch.tensor([float("nan"), 0.0, -1.0, float("inf"), 2.0], device=dev)
    x = bnn.ops.philox_std_gamma(_rng(dev, 1, 2), 9 * 64, a).cpu()
    assert torch.isnan(x[:4]).all() and torch.isfinite(x[4]) and x[4] > 0


# ---------------------------------------------------------------------------------------------------------- 4. gradient
def test_gamma_grad_vs_incomplete_gamma_and_torch(bnn, dev):
    from scipy import special, stats
    A, X = [], []
    for a in (0.05, 0.2, 0.5, 0.9, 1.0, 1.05, 2.0, 3.0, 8.1, 12.0, 30.0, 100.0, 1000.0):
        for q in (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999):
            x = float(np.float32(stats.gamma.ppf(q, a)))
            if x < F32.tiny:                   # (a = 0.05: the low quantiles are below FLT_MIN, where the draws are clamped)
                continue
            A.append(a)
            X.append(x)
    a64, x64 = np.array(A, np.float32).astype(np.float64), np.array(X, np.float64)
    got = bnn.ops.gamma_grad(torch.tensor(X, device=dev), torch.tensor(A, device=dev)).double().cpu().numpy()
    h = 1e-5 * np.maximum(a64, 1.0)
    dF = (special.gammainc(a64 + h, x64) - special.gammainc(a64 - h, x64)) / (2 * h)
    ref = -dF / stats.gamma.pdf(x64, a64)
    err = np.abs(got - ref) / np.abs(ref)
    assert err.max() < 5e-4, (err.max(), A[int(err.argmax())], X[int(err.argmax())])
    tg = torch._standard_gamma_grad(torch.tensor(A, dtype=torch.float32), torch.tensor(X, dtype=torch.float32)).double().numpy()
    err_t = np.abs(got - tg) / np.abs(tg)
    assert err_t.max() < 1e-3, err_t.max()


# ---------------------------------------------------------------------------------------------------------- 5. layer
@pytest.mark.parametrize("case", ["c0", "c1", "c2"])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_layer_forward_backward_vs_oracle(bnn, dev, golden, temper, case, prec):
    temper(0.5)
    c = golden("base.npz").case(case)
    B, I, O = [int(v) for v in c["shape"]]
    p = sub(c, "p.")
    layer = bnn.base.BayesianLinear(I, O, 1)
    layer.load_state_dict(p)
    layer = layer.to(dev).train()
    L = layer._layer_id
    rng = _rng(dev, 2024, 17)
    x = c["x"].to(dev).requires_grad_(True)
    bnn.set_precision(prec)
    try:
        out, lp, lq = layer.sample_forward(x, rng=rng)
        ((out ** 2).sum() + (lq - lp) / 600).backward()
    finally:
        bnn.set_precision("fp32")
    assert torch.equal(layer.log_prior, lp.detach()) and torch.equal(layer.log_variational_posterior, lq.detach())
    ops = bnn.ops
    u = ops.philox_uniform(rng, ops.STREAM_GATE * 64 + L, O, I).double().cpu()
    eps_w = ops.philox_normal(rng, ops.STREAM_EPS_W * 64 + L, O, I).double().cpu()
    eps_b = ops.philox_normal(rng, ops.STREAM_EPS_B * 64 + L, 0, O).double().cpu()
    P64 = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    x64 = c["x"].double().requires_grad_(True)
    alpha = 1 / (1 + torch.exp(-P64["lambdal"]))
    cg = _relaxed(alpha, u, 0.5)
    tw_x = layer.tau_w.double().cpu() * p["weight_b"].double()
    tb_x = layer.tau_b.double().cpu() * p["bias_b"].double()
    tau_w = _GammaRep.apply(P64["weight_a"], P64["weight_b"], tw_x)
    tau_b = _GammaRep.apply(P64["bias_a"], P64["bias_b"], tb_x)
    assert float((layer.gammas.double().cpu() - cg.detach()).abs().max()) < 1e-5
    o, lp64, lq64 = orc.base_forward(x64, P64, cg, {"eps_w": eps_w, "eps_b": eps_b, "tau_w": tau_w, "tau_b": tau_b},
                                     mode="sample", gamma_alpha=alpha)
    ((o ** 2).sum() + (lq64 - lp64) / 600).backward()
    assert rel_err(out, o) < (TIGHT if prec == "fp32" else 2e-5)
    assert rel_err(lp, lp64) < 2e-5 and rel_err(lq, lq64) < 2e-5
    tol = 2e-4 if prec == "fp32" else 5e-4
    assert rel_err(x.grad, x64.grad) < tol
    for name, prm in layer.named_parameters():
        assert P64[name].grad is not None, name
        assert rel_err(prm.grad, P64[name].grad) < tol, name


# ---------------------------------------------------------------------------------------------------------- 6. network
def test_network_hip_draws_vs_torch_path_on_the_same_draws(bnn, dev):
    torch.manual_seed(0)
    net = bnn.base.BayesianNetwork().to(dev).train()
    g = torch.Generator().manual_seed(5)
    x = torch.rand(100, 1, 28, 28, generator=g).to(dev)
    y = torch.randint(0, 10, (100,), generator=g).to(dev)
    st = bnn.ops.RngState.get(dev)
    rng0 = st.t[:2].clone()
    loss_h, lp_h, lq_h, nll_h = net.sample_elbo(x, y, draws="hip")
    loss_h.backward()
    names = ("weight_mu", "weight_rho", "bias_mu", "bias_rho", "pa", "pb")
    layers = (net.l1, net.l2, net.l3)
    gh = [{n: getattr(l, n).grad.clone() for n in names} for l in layers]
    ops = bnn.ops
    for l in layers:
        O, I, L = l.out_features, l.in_features, l._layer_id
        l.noise = {"eps_w": ops.philox_normal(rng0, ops.STREAM_EPS_W * 64 + L, O, I),
                   "eps_b": ops.philox_normal(rng0, ops.STREAM_EPS_B * 64 + L, 0, O),
                   "tau_w": l.tau_w.clone(), "tau_b": l.tau_b.clone()}
        gm = l.gammas.clone()
        l.gamma.rsample = (lambda gm=gm: gm)
    net.zero_grad()
    loss_t, lp_t, lq_t, nll_t = net.sample_elbo(x, y)
    loss_t.backward()
    for h, t, what in ((loss_h, loss_t, "loss"), (lp_h, lp_t, "lp"), (lq_h, lq_t, "lq"), (nll_h, nll_t, "nll")):
        assert rel_err(h.detach(), t.detach()) < 2e-5, what
    for li, l in enumerate(layers):
        for n in names:
            assert rel_err(gh[li][n], getattr(l, n).grad) < 5e-4, (li, n)
        assert torch.isfinite(l.lambdal.grad).all()


# ---------------------------------------------------------------------------------------------------------- 7. noise
def test_consecutive_calls_differ_and_manual_seed_reproduces(bnn, dev):
    net = bnn.base.BayesianNetwork((784, 64, 48, 10)).to(dev).train()
    x = torch.rand(32, 784, device=dev)
    y = torch.randint(0, 10, (32,), device=dev)

    def call():
        with torch.no_grad():
            loss = net.sample_elbo(x, y, draws="hip")[0]
        return [t.clone() for t in (net.l1.gammas, net.l2.tau_w, net.l3.tau_b, loss)]
    torch.manual_seed(11)
    a = call()
    b = call()
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])
    torch.manual_seed(12)
    call()
    torch.manual_seed(11)
    c = call()
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    # samples > 1: one offset step per sample
    st = bnn.ops.RngState.get(dev)
    off0 = int(st.t[1])
    with torch.no_grad():
        loss3 = net.sample_elbo(x, y, 3, draws="hip")[0]
    assert int(st.t[1]) == off0 + 3 and torch.isfinite(loss3)


# ---------------------------------------------------------------------------------------------------------- 8. graph
def test_graphed_hip_draw_step_equals_eager_subprocess():
    """The draws="hip" step captured with graphs.make_graphed_train_step: 20 replays are bitwise 20 eager steps from the same
    seed and parameters; the loss falls over 30 replays.  Own process (capture wants a clean autograd state)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, copy, torch
sys.path.insert(0, %r)
import bnn_amd
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.base.BayesianNetwork().to(dev).train()
init = copy.deepcopy(net.state_dict())
opt = bnn_amd.optim.Adam(net.parameters(), lr=3e-2)
g = torch.Generator().manual_seed(1)
x = torch.rand(100, 1, 28, 28, generator=g).to(dev); y = torch.randint(0, 10, (100,), generator=g).to(dev)
lf = lambda n, a, b: n.sample_elbo(a, b, draws="hip")[0]
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)

def reset():
    net.load_state_dict(init)
    for s in opt.state.values():
        s["exp_avg"].zero_(); s["exp_avg_sq"].zero_()
    for gr in opt.param_groups:
        gr["step_dev"].zero_()
    bnn_amd.manual_seed(7)

reset()
gl = [float(step(x, y)) for _ in range(20)]
gp = {k: v.detach().clone() for k, v in net.named_parameters()}
reset()
el = []
for _ in range(20):
    opt.zero_grad(set_to_none=True)
    loss = lf(net, x, y)
    loss.backward()
    opt.step()
    el.append(float(loss.detach()))
del loss
torch.cuda.synchronize()
assert gl == el, (gl, el)
for k, v in net.named_parameters():
    assert torch.equal(v.detach(), gp[k]), k
reset()
vals = [float(step(x, y)) for _ in range(30)]
assert all(v == v for v in vals), vals
assert sum(vals[-5:]) < sum(vals[:5]), vals
print("BASEGRAPH_OK", vals[0], vals[-1])
""" % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BASEGRAPH_OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])
