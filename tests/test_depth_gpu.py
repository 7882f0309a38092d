"""GPU tier of LRT / MNF networks of any depth (1 to 16 layers; layers.MAX_DEPTH).

A network of n layers issues its batched C calls in ceil(n / 4) groups of consecutive layers (_lib.layer_groups); the first
group's call takes the Philox snapshot, every group reads it, one call advances the live offset, and for n > 4 the network KL
is lbbnn_kl_total's fp32 left fold of the per-layer values the groups' finalizes wrote side by side.

Shapes: dims = (40,) + hidden + (10,), hidden widths cycling through 32, 24, 48, 40; depths 1, 2, 4, 5, 8, 9, 16 (one layer,
one full group, a group plus one, two groups, two groups plus one, the limit); B in {5, 70}; one depth-5 case whose widths are
no multiples of 4, (33, 17, 9, 21, 13, 3): the path that is not fused.

Parameters: a deep network at its INITIAL values hides its first layers (the output of a default-initialised network of 9
layers moves by 6e-9 when layer 1's weight_mu is scaled by 1.001), so weight_mu ~ N(0, 4 / I), lambdal ~ U(-3, 3) and, MNF,
q0_mean = 1 + 0.1 N(0, 1) (RNVP: divided by 0.55, see Z_SCALE); everything else as constructed.  Every parity test first asserts on the CPU, with the fp64 oracle,
that scaling ANY single layer's weight_mu by 1.01 moves the output by at least twice the bar it is about to apply.

Bars (tests/test_parity_gpu.py): TIGHT = 5e-6 for fp32 at every depth (the oracle in fp32 against itself in fp64 stays below
2.1e-7 / 1.5e-7 for output / KL up to 16 layers); bf16x3 keeps 2e-5 up to 4 layers and TOL = 1e-4, the contract, beyond;
the worst measured value per depth and format is printed."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import elementwise_violation, rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4
TIGHT = 5e-6
HIDDEN = (32, 24, 48, 40)
DEPTHS = (1, 2, 4, 5, 8, 9, 16)
BS = (5, 70)
ODD = (33, 17, 9, 21, 13, 3)
FAMILIES = ("lrt", "Planar", "RNVP")
T = 2

# An RNVP transform as constructed maps z to about 0.75 z (half the entries pass, the others are mixed with sigmoid(s) ~ 0.5
# towards a shift ~ 0), so two of them leave z ~ 0.55 q0_mean (measured with the oracle: 0.44 ... 0.64 per layer) and the
# signal of a 16-layer network shrinks by 0.55^16 = 7e-5: scaling layer 1's weight_mu by 1.01 then moves the output by 2e-7.
# q0_mean is divided by that factor for RNVP, so that z is around 1 there too, as it is for planar flows (0.98 ... 1.02).
Z_SCALE = {"Planar": 1.0, "RNVP": 1.0 / 0.55}

_CACHE = {}          # CPU side of every case (parameters, draws, fp64 results): built once, shared, never changed


def dims_of(n):
    return (40,) + tuple(HIDDEN[i % 4] for i in range(n - 1)) + (10,)


def bar_of(prec, n):
    if prec == "fp32":
        return TIGHT
    return {"bf16x3": 2e-5, "fp16x3f": 4e-5}[prec] if n <= 4 else TOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture
def precision(bnn):
    def set_(p):
        bnn.set_precision(p)
    yield set_
    bnn.set_precision("fp32")


def layers_of(net):
    return [getattr(net, "l%d" % (i + 1)) for i in range(len(net.dims) - 1)]


# The seed of the parameter draws: picked, among 2000, 2100, ..., as the first for which the precondition above holds for
# every case of this file (it is asserted in every parity test; the worst case is always 16 layers at B = 5).
PARAM_SEED = 3000


def make_net(bnn, family, dims, seed=None):
    """A network on the CPU with the parameters of the module docstring."""
    torch.manual_seed(1000 + len(dims) if seed is None else seed)
    if family == "lrt":
        net = bnn.lrt.BayesianNetwork(dims)
    else:
        net = bnn.mnf.BayesianNetwork(dims, T, z_flow_type=family, r_flow_type=family)
    assert len(net.dims) == len(dims) and hasattr(net, "l%d" % (len(dims) - 1))
    g = torch.Generator().manual_seed(PARAM_SEED + len(dims))
    with torch.no_grad():
        for l in layers_of(net):
            O, I = l.out_features, l.in_features
            l.weight_mu.copy_(torch.randn(O, I, generator=g) * (2.0 / math.sqrt(I)))
            l.lambdal.copy_(torch.empty(O, I).uniform_(-3, 3, generator=g))
            if family != "lrt":
                l.q0_mean.copy_(Z_SCALE[family] * (1.0 + 0.1 * torch.randn(I, generator=g)))
    return net


def _draws(family, dims, B, g):
    noises = []
    for I, O in zip(dims[:-1], dims[1:]):
        n = {"eps_out": torch.randn(B, O, generator=g)}
        if family != "lrt":
            n.update(eps_z=torch.randn(1, I, generator=g), eps_z2=torch.randn(1, I, generator=g),
                     eps_act=torch.randn(O, generator=g))
        if family == "RNVP":
            bern = lambda: torch.bernoulli(torch.full((I,), 0.5), generator=g)
            n.update(zmask=[bern() for _ in range(T)], zmask2=[bern() for _ in range(T)], rmask=[bern() for _ in range(T)])
        noises.append(n)
    return noises


def _f64(v):
    return [m.double() for m in v] if isinstance(v, list) else v.double()


def oracle_forward(family, x, P, noises):
    """(log-probabilities, [per-layer KL]) of the oracle in the dtype of its inputs."""
    h, kls = x.reshape(x.shape[0], -1), []
    for i, (p, n) in enumerate(zip(P, noises)):
        if family == "lrt":
            h, k, _ = orc.lrt_forward(h, p, n["eps_out"])
        else:
            h, k, _ = orc.mnf_forward(h, p, orc.flow_from_state("z_flow", family, p, T),
                                      orc.flow_from_state("r_flow", family, p, T), n)
        kls.append(k)
        if i < len(P) - 1:
            h = torch.relu(h)
    return torch.log_softmax(h, dim=1), kls


def case(bnn, family, dims, B):
    """The CPU side of one (family, dims, B): the network, its fp64 parameters, the draws, the fp64 oracle's output and KLs,
    and ``shift``: the smallest move of the output, over the layers, when one layer's weight_mu is scaled by 1.01."""
    key = (family, tuple(dims), B)
    if key not in _CACHE:
        net = make_net(bnn, family, dims)
        g = torch.Generator().manual_seed(3000 + 7 * len(dims) + B)
        x = torch.rand(B, dims[0], generator=g)
        noises = _draws(family, dims, B, g)
        P = [{k: v.detach().double() for k, v in l.state_dict().items()} for l in layers_of(net)]
        n64 = [{k: _f64(v) for k, v in n.items()} for n in noises]
        with torch.no_grad():
            ref_out, ref_kls = oracle_forward(family, x.double(), P, n64)
            shifts = []
            for i in range(len(P)):
                Q = list(P)
                Q[i] = dict(P[i], weight_mu=P[i]["weight_mu"] * 1.01)
                shifts.append(rel_err(oracle_forward(family, x.double(), Q, n64)[0], ref_out))
        _CACHE[key] = dict(net=net, x=x, noises=noises, P=P, n64=n64, ref_out=ref_out, ref_kls=ref_kls, shift=min(shifts))
    return _CACHE[key]


def on_device(c, dev, train=True):
    """A device copy of the case's network with the case's draws injected."""
    import copy
    net = copy.deepcopy(c["net"]).to(dev)
    net.train(train)
    for l, n in zip(layers_of(net), c["noises"]):
        l.noise = {k: ([m.to(dev) for m in v] if isinstance(v, list) else v.to(dev)) for k, v in n.items()}
    return net


def left_fold(kls):
    """((0 + k0) + k1) + ... in fp32 on the values' own device."""
    t = torch.zeros((), dtype=torch.float32, device=kls[0].device)
    for k in kls:
        t = t + k
    return t


# --------------------------------------------------------------------------- 1. forward and KL against the fp64 oracle
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("n", DEPTHS)
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_and_kl_vs_fp64_oracle(bnn, dev, precision, family, n, B, prec):
    dims = dims_of(n)
    c = case(bnn, family, dims, B)
    bar = bar_of(prec, n)
    assert c["shift"] >= 2 * bar, (c["shift"], bar)           # a wrong layer would show: asserted before anything runs
    net = on_device(c, dev)
    precision(prec)
    with torch.no_grad():
        out = net(c["x"].to(dev), sample=True)
        total = net.kl()
    ls = layers_of(net)
    e_out = rel_err(out, c["ref_out"])
    e_kls = [rel_err(l.kl, k) for l, k in zip(ls, c["ref_kls"])]
    e_kl = rel_err(total, sum(c["ref_kls"]))
    print("depth-vs-fp64 %s n=%d B=%d %s out %.3g kl %.3g worst layer kl %.3g (shift %.3g)"
          % (family, n, B, prec, e_out, e_kl, max(e_kls), c["shift"]))
    assert out.shape == (B, 10) and bool(torch.isfinite(out).all())
    assert e_out < bar, e_out
    assert max(e_kls) < bar, e_kls
    assert e_kl < bar, e_kl
    if n > 4:
        assert torch.equal(total, left_fold([l.kl for l in ls]))     # lbbnn_kl_total: the fp32 left fold, bit for bit


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("family", FAMILIES)
def test_widths_that_are_no_multiples_of_4_vs_fp64_oracle(bnn, dev, precision, family, B, prec):
    """Depth 5 with widths (33, 17, 9, 21, 13, 3): no layer takes the split kernels or the row weight pass."""
    c = case(bnn, family, ODD, B)
    bar = bar_of(prec, 5)
    assert c["shift"] >= 2 * bar, (c["shift"], bar)
    net = on_device(c, dev)
    precision(prec)
    with torch.no_grad():
        out = net(c["x"].to(dev), sample=True)
        total = net.kl()
    ls = layers_of(net)
    e_out, e_kl = rel_err(out, c["ref_out"]), rel_err(total, sum(c["ref_kls"]))
    e_kls = [rel_err(l.kl, k) for l, k in zip(ls, c["ref_kls"])]
    print("depth-vs-fp64 odd widths %s B=%d %s out %.3g kl %.3g worst layer kl %.3g (shift %.3g)"
          % (family, B, prec, e_out, e_kl, max(e_kls), c["shift"]))
    assert e_out < bar and max(e_kls) < bar and e_kl < bar, (e_out, e_kls, e_kl)
    assert torch.equal(total, left_fold([l.kl for l in ls]))


# --------------------------------------------------------------------------- 2. in-kernel draws are per layer
def test_in_kernel_draws_are_per_layer(bnn, dev):
    """Layer i of a deep network draws what a stand-alone layer with id i draws at the forward's offset: regenerating every
    layer's eps_out from the offset before the forward and injecting them gives the in-kernel forward bit for bit."""
    ops = bnn.ops
    dims, B = (40, 32, 32, 32, 32, 32, 10), 70
    net = make_net(bnn, "lrt", dims).to(dev).train()
    ls = layers_of(net)
    assert [l._layer_id for l in ls] == list(range(6))
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(5)).to(dev)
    bnn.manual_seed(21, 9)
    st = ops.RngState.get(dev)
    with torch.no_grad():
        start = st.t[:2].clone()
        out = net(x, sample=True).clone()
        kl = net.kl().clone()
        assert int(st.t[1]) == int(start[1]) + 1                    # advanced once, by one
        st.t[:2].copy_(start)
        eps = [ops.philox_normal(st.t, ops.STREAM_EPS_OUT * 64 + i, B, l.out_features, row_base=l.row_offset)
               for i, l in enumerate(ls)]
        for a in range(len(eps)):
            for b in range(a + 1, len(eps)):
                if eps[a].shape == eps[b].shape:
                    assert not torch.equal(eps[a], eps[b]), (a, b)
        for l, e in zip(ls, eps):
            l.noise = {"eps_out": e}
        out2 = net(x, sample=True)
        assert torch.equal(out2, out) and torch.equal(net.kl(), kl)


# --------------------------------------------------------------------------- 3. recorded, captured and eager agree bitwise
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("n", [5, 9])
@pytest.mark.parametrize("family", FAMILIES)
def test_launch_plan_and_graph_replay_equal_the_eager_sequence_bitwise(bnn, dev, precision, family, n, prec):
    """From the same Philox {seed, offset}: call k of graphs.LaunchPlan and replay k of the captured forward give the k-th
    eager forward's output, per-layer KLs and total bit for bit, an in-place parameter change between calls included."""
    from bnn_amd import graphs, ops
    dims, B = dims_of(n), 70
    precision(prec)
    net = make_net(bnn, family, dims).to(dev).train()
    ls = layers_of(net)
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(6)).to(dev)
    st = ops.RngState.get(dev)
    bnn.manual_seed(31, 4)
    with torch.no_grad():
        net(x, sample=True); torch.cuda.synchronize()
        start = st.t[:2].clone()
        orig = net.l2.bias_mu.detach().clone()
        eager = []
        for k in range(3):
            if k == 2:
                net.l2.bias_mu.add_(0.25)
            o = net(x, sample=True)
            eager.append((o.clone(), net.kl().clone(), [l.kl.clone() for l in ls]))
        assert int(st.t[1]) == int(start[1]) + 3
        assert not torch.equal(eager[0][0], eager[1][0])
        for e in eager:
            assert torch.equal(e[1], left_fold(e[2]))
        net.l2.bias_mu.copy_(orig)
        torch.cuda.synchronize()
        plan = graphs.LaunchPlan(net, x, sample=True)
        print("launch plan %s n=%d %s: %d C calls" % (family, n, prec, len(plan)))
        st.t[:2].copy_(start)
        for k in range(3):
            if k == 2:
                net.l2.bias_mu.add_(0.25)
            out, kl = plan()
            torch.cuda.synchronize()
            assert torch.equal(out, eager[k][0]) and torch.equal(kl, eager[k][1]) and torch.equal(net.kl(), eager[k][1]), k
            assert all(torch.equal(l.kl, e) for l, e in zip(ls, eager[k][2])), k
        net.l2.bias_mu.copy_(orig)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gout = net(x, sample=True)
            gkl = net.kl()
        st.t[:2].copy_(start)
        for k in range(3):
            if k == 2:
                net.l2.bias_mu.add_(0.25)
            g.replay(); torch.cuda.synchronize()
            assert torch.equal(gout, eager[k][0]) and torch.equal(gkl, eager[k][1]), k


# --------------------------------------------------------------------------- 4. training
@pytest.mark.parametrize("family", ["lrt", "Planar"])
def test_training_step_gradients_vs_fp64_autograd(bnn, dev, family):
    """One step's gradients of a five-layer network against autograd of the oracle in fp64, at the bars of
    test_planar_backward_all_hip_vs_oracle_autograd / test_lrt_backward_vs_oracle_autograd: TOL for the output and the input
    gradient, 5e-5 for every parameter's gradient.  net.kl() of the training forward is the left fold too."""
    n, B = 5, 70
    dims = dims_of(n)
    c = case(bnn, family, dims, B)
    assert c["shift"] >= 2 * TOL, c["shift"]
    net = on_device(c, dev)
    wgt = torch.randn(B, 10, generator=torch.Generator().manual_seed(5))
    xg = c["x"].to(dev).requires_grad_(True)
    out = net(xg, sample=True)
    total = net.kl()
    ls = layers_of(net)
    assert torch.equal(total.detach(), left_fold([l.kl.detach() for l in ls]))
    ((out * wgt.to(dev)).sum() + total / 60).backward()
    P = [{k: v.clone().requires_grad_(True) for k, v in p.items()} for p in c["P"]]
    xc = c["x"].double().requires_grad_(True)
    o, kls = oracle_forward(family, xc, P, c["n64"])
    ((o * wgt.double()).sum() + sum(kls) / 60).backward()
    assert rel_err(out.detach(), o.detach()) < TOL
    assert rel_err(total.detach(), sum(kls).detach()) < TOL
    assert rel_err(xg.grad, xc.grad) < TOL
    worst = 0.0
    for i, (l, p) in enumerate(zip(ls, P)):
        for name, prm in l.named_parameters():
            ref = p[name].grad
            if ref is None or float(ref.abs().max()) == 0.0:
                assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, (i, name)
                continue
            e = rel_err(prm.grad, ref)
            worst = max(worst, e)
            assert e < 5e-5, (i, name, e)
    print("depth training gradients %s n=%d worst parameter gradient rel_err %.3g" % (family, n, worst))
    del out, total, o


def test_graphed_train_step_equals_eager_at_depth_5_subprocess():
    """graphs.make_graphed_train_step on a five-layer MNF network: 6 replays are bitwise 6 eager steps from the same seed and
    parameters (losses and every parameter).  Own process (capture wants a clean autograd state)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, copy, torch
sys.path.insert(0, %r)
import bnn_amd
from bnn_amd import layers
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.mnf.BayesianNetwork((40, 32, 24, 48, 40, 10), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
assert len(net._layers()) == 5
init = copy.deepcopy(net.state_dict())
opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-3)
g = torch.Generator().manual_seed(1)
x = torch.rand(70, 40, generator=g).to(dev); y = torch.randint(0, 10, (70,), generator=g).to(dev)
lf = lambda n, a, b: torch.nn.functional.nll_loss(n(a, sample=True), b, reduction="sum") + n.kl() / 100
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)

def reset():
    net.load_state_dict(init)
    for s in opt.state.values():
        s["exp_avg"].zero_(); s["exp_avg_sq"].zero_()
    for gr in opt.param_groups:
        gr["step_dev"].zero_()
    bnn_amd.manual_seed(7)

reset()
gl = [float(step(x, y)) for _ in range(6)]
gp = {k: v.detach().clone() for k, v in net.named_parameters()}
reset()
el = []
for _ in range(6):
    opt.zero_grad(set_to_none=True)
    loss = lf(net, x, y)
    with layers.vector_backward_overlap():
        loss.backward()
    opt.step()
    el.append(float(loss.detach()))
del loss
torch.cuda.synchronize()
assert gl == el, (gl, el)
assert len(set(gl)) == 6
for k, v in net.named_parameters():
    assert torch.equal(v.detach(), gp[k]), k
print("DEPTHGRAPH_OK", gl[0], gl[-1])
""" % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEPTHGRAPH_OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])


# --------------------------------------------------------------------------- 5. evaluation stack
SEED, OFF = 3, 5


def _eval_net(bnn, dev, family, n):
    return make_net(bnn, family, dims_of(n)).to(dev).eval()


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("n", [5, 9])
@pytest.mark.parametrize("family", ["lrt", "Planar"])
def test_batched_ensemble_and_alpha_model_equal_the_loop_bitwise(bnn, dev, precision, family, n, prec):
    ev = bnn.evaluate
    net = _eval_net(bnn, dev, family, n)
    precision(prec)
    st = bnn.ops.RngState.get(dev)
    fz = ev.freeze(net)
    assert fz.n_layers == n and len(fz.kept) == n and len(fz.kept_rows) == n
    total = sum(a * b for a, b in zip(net.dims[:-1], net.dims[1:]))
    assert fz.density == sum(int((l.lambdal > 0).sum()) for l in layers_of(net)) / total
    for B, S in [(70, 6), (5, 3)]:
        x = torch.rand(B, 40, generator=torch.Generator().manual_seed(B)).to(dev)
        bnn.manual_seed(SEED, OFF)
        loop = ev.ensemble_forward(net, x, S, batched=False)
        assert int(st.t[1]) == OFF + S
        bnn.manual_seed(SEED, OFF)
        bat = ev.ensemble_forward(net, x, S, batched=True)
        assert int(st.t[1]) == OFF + S
        bnn.manual_seed(SEED, OFF)
        frz = fz.ensemble(x, S)
        assert int(st.t[1]) == OFF + S
        assert loop.shape == (S, B, 10) and not torch.equal(loop[0], loop[1])
        assert torch.equal(bat, loop), (B, S)
        assert torch.equal(frz, bat), (B, S)
    # refresh() follows an in-place change of the LAST group's layer
    with torch.no_grad():
        layers_of(net)[-1].weight_mu.mul_(1.5)
    bnn.manual_seed(SEED, OFF)
    stale = fz.ensemble(x, S)
    assert torch.equal(stale, frz)
    fz.refresh()
    bnn.manual_seed(SEED, OFF)
    fresh = fz.ensemble(x, S)
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(fresh, ev.ensemble_forward(net, x, S, batched=True)) and not torch.equal(fresh, stale)


def _mpm_lambdal(net, seed=7):
    """lambdal ~ U(-3, 3) pushed at least 1e-3 away from 0 (tests/test_frozen_gpu.py); returns the kept masks."""
    g = torch.Generator().manual_seed(seed)
    masks = []
    for l in layers_of(net):
        O, I = l.out_features, l.in_features
        lam = torch.empty(O, I).uniform_(-3, 3, generator=g)
        lam = torch.where(lam.abs() < 2e-3, torch.where(lam < 0, -2e-3, 2e-3), lam)
        lam[0, :] = -2.0
        lam[:, 0] = -2.0
        assert float(lam.abs().min()) >= 1e-3
        with torch.no_grad():
            l.lambdal.copy_(lam)
        keep = lam > 0
        assert 0 < int(keep.sum()) < O * I
        masks.append(keep)
    return masks


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("n", [5, 9])
@pytest.mark.parametrize("family", ["lrt", "Planar"])
def test_mpm_model_vs_fp64_oracle_on_thresholded_gates(bnn, dev, precision, family, n, prec):
    """The median probability model of a deep network against the fp64 oracle with lambdal = +-1000 (alpha exactly 1 / 0), the z
    every member used and eps_out regenerated at the documented stream / offset (tests/test_frozen_gpu.py test 3): TOL and the
    element-wise form.  First, on the CPU: un-gating any single layer moves the oracle output by more than 2 TOL."""
    ev, ops = bnn.evaluate, bnn.ops
    net = _eval_net(bnn, dev, family, n)
    masks = _mpm_lambdal(net)
    precision(prec)
    fz = ev.freeze(net, "mpm")
    assert fz.kept == [int(k.sum()) for k in masks]
    B, S = 70, 3
    x = torch.rand(B, 40, generator=torch.Generator().manual_seed(2)).to(dev)
    bnn.manual_seed(SEED, OFF)
    out = fz.ensemble(x, S, keep_z=True)
    z = fz.last_z
    assert len(z) == n
    ls = layers_of(net)

    def member(m, scale_layer=None):
        rng_m = torch.tensor([SEED, OFF + m, 0, 0], dtype=torch.int64, device=dev)
        P, noise = [], []
        for i, (l, keep) in enumerate(zip(ls, masks)):
            p = {k: getattr(l, k).detach().double().cpu() for k in ("weight_mu", "weight_rho", "bias_mu", "bias_rho")}
            if i == scale_layer:
                p["weight_mu"] = p["weight_mu"] * 1.01
            p["lambdal"] = torch.where(keep, 1000.0, -1000.0).double()
            eps = ops.philox_normal(rng_m, ops.STREAM_EPS_OUT * 64 + l._layer_id, B, l.out_features,
                                    row_base=l.row_offset).double().cpu()
            if family != "lrt":
                p["q0_mean"] = z[i][m].double().cpu()
                p["q0_log_var"] = torch.full_like(p["q0_mean"], -float("inf"))
                noise.append({"eps_z": torch.zeros(1, l.in_features, dtype=torch.float64), "eps_out": eps})
            else:
                noise.append(eps)
            P.append(p)
        if family != "lrt":
            return orc.mnf_network_forward(x.double().cpu(), P, [orc.Flow("Planar", [])] * n, [None] * n, noise,
                                           compute_kl=False)[0]
        return orc.lrt_network_forward(x.double().cpu(), P, noise, compute_kl=False)[0]

    ref0 = member(0)
    shift = min(rel_err(member(0, i), ref0) for i in range(n))
    assert shift >= 2 * TOL, shift
    worst = 0.0
    for m in range(S):
        ref = ref0 if m == 0 else member(m)
        e, v = rel_err(out[m], ref), elementwise_violation(out[m], ref)
        worst = max(worst, e)
        assert e < TOL and v <= 1.0, (m, e, v)
    print("depth mpm-vs-fp64 %s n=%d %s worst rel_err %.3g (shift %.3g)" % (family, n, prec, worst, shift))


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("n", [5, 9])
def test_dense_frozen_model_against_the_loop(bnn, dev, precision, n, prec):
    """freeze(net, dense=True) of a deep RNVP network against the loop of single forwards, both measured against fp64 on the
    same eps_z, masks and eps_out: err_new <= max(bar, 2 * err_loop), the bar of tests/test_frozen_dense_gpu.py test 4."""
    from philox_bits_ref import mask_bits
    ev, ops = bnn.evaluate, bnn.ops
    net = _eval_net(bnn, dev, "RNVP", n)
    ls = layers_of(net)
    precision(prec)
    fz = ev.freeze(net, "alpha", dense=True)
    assert fz.flows == "dense" and fz.n_layers == n
    B, S = 70, 3
    x = torch.rand(B, 40, generator=torch.Generator().manual_seed(2)).to(dev)
    st = ops.RngState.get(dev)
    bnn.manual_seed(SEED, OFF)
    new = fz.ensemble(x, S)
    assert int(st.t[1]) == OFF + S
    bnn.manual_seed(SEED, OFF)
    with torch.no_grad():
        loop = torch.stack([net(x, sample=True) for _ in range(S)])
    assert int(st.t[1]) == OFF + S
    P = [{k: v.detach().double().cpu() for k, v in l.state_dict().items()} for l in ls]
    zf = [orc.flow_from_state("z_flow", "RNVP", p, T) for p in P]
    refs = []
    for m in range(S):
        rng_m = torch.tensor([SEED, OFF + m, 0, 0], dtype=torch.int64, device=dev)
        noise = []
        for l in ls:
            I, O, L = l.in_features, l.out_features, l._layer_id
            mk = torch.from_numpy(mask_bits(SEED, OFF + m, L, I, T))
            noise.append({"eps_z": ops.philox_normal(rng_m, ops.STREAM_EPS_Z * 64 + L, 0, I).double().cpu().reshape(1, I),
                          "zmask": [r.double().reshape(1, I) for r in mk],
                          "eps_out": ops.philox_normal(rng_m, ops.STREAM_EPS_OUT * 64 + L, B, O, row_base=l.row_offset).double().cpu()})
        refs.append(orc.mnf_network_forward(x.double().cpu(), P, zf, [None] * n, noise, compute_kl=False)[0])
    ref = torch.stack(refs)
    e_new, e_loop = rel_err(new, ref), rel_err(loop, ref)
    print("depth dense alpha-vs-loop n=%d %s err_new %.3g err_loop %.3g" % (n, prec, e_new, e_loop))
    assert e_loop < TOL
    assert e_new <= max(bar_of(prec, 1), 2 * e_loop), (e_new, e_loop)


@pytest.mark.parametrize("n", [5, 9])
@pytest.mark.parametrize("family", ["lrt", "Planar"])
def test_ensemble_eval_evaluate_batches_and_graphed_eval_step_agree(bnn, dev, family, n):
    ev = bnn.evaluate
    from bnn_amd import graphs
    net = _eval_net(bnn, dev, family, n)
    B, S = 70, 4
    g = torch.Generator().manual_seed(9)
    x = torch.rand(B, 40, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    bnn.manual_seed(SEED, OFF)
    r = ev.ensemble_eval(net, x, y, S)
    assert r["outputs"].shape == (S, B, 10) and r["density"].shape == (S,)
    assert bool(((r["density"] > 0) & (r["density"] < 1)).all())
    ent = ev.predictive_entropy(r["outputs"])
    assert ent.shape == (B,) and bool(torch.isfinite(ent).all())
    bnn.manual_seed(SEED, OFF)
    res = ev.evaluate_batches(net, [(x, y)], S)
    assert res["rows"] == B and res["correct_ensemble"] == r["correct_ensemble"]
    assert res["correct_posterior_mean"] == r["correct_posterior_mean"]
    # the frozen model: eager pass and the graphed step, from the same offset
    fz = ev.freeze(net)
    bnn.manual_seed(SEED, OFF)
    rf = ev.ensemble_eval(fz, x, y, S)
    assert torch.equal(rf["outputs"], r["outputs"]) and rf["correct_ensemble"] == r["correct_ensemble"]
    bnn.manual_seed(SEED, OFF)
    res_f = ev.evaluate_batches(fz, [(x, y)], S)
    acc = ev.EvalAccumulator(10, S, dev)
    step = graphs.make_graphed_eval_step(fz, x, y, S, acc)
    bnn.manual_seed(SEED, OFF)
    step(x, y)
    res_g = acc.result()
    for k in ("rows", "correct_ensemble", "correct_posterior_mean"):
        assert res_g[k] == res_f[k] == res[k], (k, res_g[k], res_f[k], res[k])
