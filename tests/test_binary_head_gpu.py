"""GPU tier of the binary (sigmoid) head: the four kernels of csrc/binary_head.hip against the float64 restatement
tests/binary_head_ref.py, and the head through every layer that has a multiclass head -- network forward (autograd, fused,
LaunchPlan), the loss hand-over, the captured training step, the ensembles, the frozen model and the device-side metrics.

BARS (float64 of the same expression on the same float32 inputs):
  * probabilities and the 2-class log-probabilities, 1e-6 relative (+ 1e-37): expf and log1pf <= 2 ulp each, the add and the
    divide <= 0.5 each, under 4 ulp = 2.4e-7, with a factor 4 for the device's expf;
  * the loss, 2e-6 * (sum |term| + |kl * scale|): logf / log1pf <= 2 ulp per term, sums in fp64, one final rounding, under 3e-7,
    times 6;
  * g_probs and g_logits, 1e-6 relative (+ 1e-30): a subtraction, two products and a correctly rounded divide, under 4 ulp.
tests/test_binary_head_host.py asserts that the float32 form of the restatement itself stays inside each of them.
Everything that is plumbing (the head inside the network, the hand-over, the captured step, chunking) is held bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import binary_head_ref as ref
import eval_metrics_ref as mref
import eval_uncertainty_ref as uref

pytestmark = pytest.mark.gpu


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


def _lib():
    from bnn_amd import _lib
    return _lib.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _same(a, b):
    """Bit for bit (a NaN equal to a NaN of the same bits)."""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _logits(n, seed):
    """The saturation vector tiled to n values plus N(0, 3) -- the first min(n, 15) values are left at the vector itself."""
    g = torch.Generator().manual_seed(seed)
    reps = -(-n // ref.SATURATION.numel())
    x = ref.SATURATION.repeat(reps)[:n].clone()
    x[15:] += 3.0 * torch.randn(n, generator=g)[15:]
    return x


def _strided(vals, B, O, ld, dev, fill=float("nan")):
    """(B, O) view with row stride ld of a NaN-filled device buffer holding ``vals``."""
    buf = torch.full((B, ld), fill, dtype=torch.float32, device=dev)
    buf[:, :O] = vals.reshape(B, O).to(dev)
    return buf, buf[:, :O]


# ------------------------------------------------------------------------------------------- 1. the head kernel
@pytest.mark.parametrize("pad", (0, 3))
@pytest.mark.parametrize("O", (1, 3))
@pytest.mark.parametrize("B", (1, 3, 257, 1031))
def test_head_kernel_against_float64(bnn, dev, B, O, pad):
    lib, n, ld = _lib(), B * O, O + pad
    x = _logits(n, 100 * B + O)
    xbuf, xv = _strided(x, B, O, ld, dev)
    pbuf = torch.full((B, ld), float("nan"), dtype=torch.float32, device=dev)
    l2 = torch.full((B, 2 + pad), float("nan"), dtype=torch.float32, device=dev) if O == 1 else None
    rc = lib.lbbnn_binary_head(xbuf.data_ptr(), ld, B, O, pbuf.data_ptr(), ld, l2.data_ptr() if O == 1 else None, 2 + pad,
                               _stream(dev))
    assert rc == 0
    p = pbuf[:, :O].cpu()
    p64 = ref.sigmoid(x).reshape(B, O)
    err = float(((p.double() - p64).abs() / (1e-6 * p64 + 1e-37)).max())
    print("binary_head B=%d O=%d ld=%d: worst |p - p64| / bar %.3g" % (B, O, ld, err))
    assert err <= 1.0
    if pad:
        assert bool(torch.isnan(pbuf[:, O:]).all())                              # nothing written between the rows
    if O == 1:
        lp = l2[:, :2].cpu()
        want = ref.logp2(x)
        assert bool(torch.isfinite(lp).all())
        e2 = float(((lp.double() - want).abs() / (1e-6 * want.abs() + 1e-37)).max())
        print("binary_head B=%d ld=%d: worst |logp2 - ref| / bar %.3g" % (B, ld, e2))
        assert e2 <= 1.0
        if pad:
            assert bool(torch.isnan(l2[:, 2:]).all())
        # either output alone gives the same bits
        only2 = torch.empty(B, 2, dtype=torch.float32, device=dev)
        assert lib.lbbnn_binary_head(xbuf.data_ptr(), ld, B, 1, None, 0, only2.data_ptr(), 2, _stream(dev)) == 0
        assert _same(only2, l2[:, :2])
    # in place over the logits: the same bits
    assert lib.lbbnn_binary_head(xbuf.data_ptr(), ld, B, O, xbuf.data_ptr(), ld, None, 0, _stream(dev)) == 0
    assert _same(xbuf[:, :O], pbuf[:, :O])
    # ... and through the Python wrapper
    assert _same(bnn.ops.binary_head(x.reshape(B, O).to(dev)), pbuf[:, :O])


def test_head_kernel_saturates_exactly(bnn, dev):
    x = ref.SATURATION.reshape(-1, 1).to(dev)
    p, lp = bnn.ops.binary_head(x, log_probs=True)
    assert float(p[0]) == 0.0 and float(p[-1]) == 1.0                            # x = -110 / +110
    assert bool((p[ref.SATURATION >= 17] == 1).all())
    assert bool(torch.isfinite(lp).all())
    assert float(lp[-1, 0]) == -110.0 and float(lp[-1, 1]) == 0.0 and float(lp[0, 0]) == 0.0 and float(lp[0, 1]) == -110.0
    assert float((lp.double().exp().sum(1) - 1).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------- 2. the loss
LOSS_SHAPES = ((1, 1), (5, 3), (400, 1), (1031, 1))


def _loss_case(bnn, dev, B, O, pad, targets="01", bad=False):
    """Device probabilities (the head kernel's own fp32 values of the saturation logits) and targets, both with row stride
    O + pad: (p view, y view, p on the CPU, y on the CPU)."""
    n, ld = B * O, O + pad
    x = _logits(n, 7 * B + O)
    p = bnn.ops.binary_head(x.reshape(B, O).to(dev)).cpu()
    if targets == "01":
        y = (torch.arange(n) % 2).float()
    else:
        y = torch.where(torch.arange(n) % 2 == 0, torch.tensor(0.25), torch.tensor(0.75))
    if bad:
        y[1], y[n // 2] = 1.5, float("nan")
    y = y.reshape(B, O)
    _, pv = _strided(p, B, O, ld, dev)
    _, yv = _strided(y, B, O, ld, dev)
    return pv, yv, p, y


def _run_loss(dev, pv, yv, kl, scale, stats=None, accumulate=0):
    B, O = pv.shape
    out = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    rc = _lib().lbbnn_elbo_bce_loss(pv.data_ptr(), pv.stride(0), yv.data_ptr(), yv.stride(0), B, O,
                                    kl.data_ptr() if kl is not None else None, ctypes.c_float(scale), out.data_ptr(),
                                    stats.data_ptr() if stats is not None else None, accumulate, _stream(dev))
    assert rc == 0
    return out


@pytest.mark.parametrize("with_kl", (False, True))
@pytest.mark.parametrize("pad", (0, 3))
@pytest.mark.parametrize("B,O", LOSS_SHAPES)
def test_loss_value_and_counts(bnn, dev, B, O, pad, with_kl):
    bad = (B, O) == (400, 1)                      # this case carries a target of 1.5 and a NaN
    pv, yv, p, y = _loss_case(bnn, dev, B, O, pad, bad=bad)
    kl = torch.tensor(1234.5, device=dev) if with_kl else None
    scale = float(torch.tensor(0.2, dtype=torch.float32))
    st = torch.full((4,), 7, dtype=torch.int32, device=dev)
    got = _run_loss(dev, pv, yv, kl, scale, st, accumulate=0)
    terms = ref.bce_terms(p, y)
    want = float(terms.sum()) + (1234.5 * scale if with_kl else 0.0)
    bar = 2e-6 * (float(terms.abs().sum()) + (abs(1234.5 * scale) if with_kl else 0.0))
    print("elbo_bce_loss B=%d O=%d ld=%d kl=%s: %.9g against %.9g, |diff| %.3g, bar %.3g"
          % (B, O, O + pad, with_kl, float(got), want, abs(float(got) - want), bar))
    assert abs(float(got) - want) <= bar
    counts = ref.stats(p, y)
    assert st.tolist() == counts and counts[1] == B * O                          # accumulate == 0 overwrites the 7s
    assert counts[2] == (2 if bad else 0)
    again = _run_loss(dev, pv, yv, kl, scale, st, accumulate=1)
    assert st.tolist() == [2 * c for c in counts]                                # ... and != 0 adds
    assert _same(got.reshape(1), again.reshape(1))                               # two runs, the same bits
    if bad:
        # the two bad targets add nothing: the loss is the loss without those two elements
        keep = ref.target_ok(y)
        assert abs(float(got) - (float(ref.bce_terms(p[keep], y[keep]).sum()) + (1234.5 * scale if with_kl else 0.0))) <= bar


def test_loss_value_with_soft_targets(bnn, dev):
    pv, yv, p, y = _loss_case(bnn, dev, 400, 1, 3, targets="soft")
    got = float(_run_loss(dev, pv, yv, None, 1.0))
    terms = ref.bce_terms(p, y)
    print("elbo_bce_loss soft targets: %.9g against %.9g, bar %.3g" % (got, float(terms.sum()), 2e-6 * float(terms.abs().sum())))
    assert abs(got - float(terms.sum())) <= 2e-6 * float(terms.abs().sum())


@pytest.mark.parametrize("pad", (0, 3))
@pytest.mark.parametrize("B,O", LOSS_SHAPES)
def test_loss_backward_against_float64(bnn, dev, B, O, pad):
    bad = (B, O) == (400, 1)
    pv, yv, p, y = _loss_case(bnn, dev, B, O, pad, bad=bad)
    scale = float(torch.tensor(0.2, dtype=torch.float32))
    lib = _lib()
    runs = []
    for _ in range(2):
        g = torch.tensor(1.0, device=dev)
        gp, gl = (torch.full((B, O), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
        gk = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        rc = lib.lbbnn_elbo_bce_loss_backward(g.data_ptr(), pv.data_ptr(), pv.stride(0), yv.data_ptr(), yv.stride(0), B, O,
                                              ctypes.c_float(scale), gp.data_ptr(), gl.data_ptr(), gk.data_ptr(), _stream(dev))
        assert rc == 0
        runs.append((gp, gl, gk))
    gp, gl, gk = runs[0]
    assert all(_same(a.reshape(-1), b.reshape(-1)) for a, b in zip(runs[0], runs[1]))            # two runs, the same bits
    wp, wl, wk = ref.backward(1.0, p, y, scale)
    ep = float(((gp.cpu().double() - wp).abs() / (1e-6 * wp.abs() + 1e-30)).max())
    el = float(((gl.cpu().double() - wl).abs() / (1e-6 * wl.abs() + 1e-30)).max())
    print("elbo_bce_loss_backward B=%d O=%d ld=%d: worst error / bar g_probs %.3g g_logits %.3g" % (B, O, O + pad, ep, el))
    assert ep <= 1.0 and el <= 1.0
    assert float(gk) == scale                                                    # g_kl = 1 * kl_scale, exact
    # without g_logits the same g_probs
    gp2 = torch.empty(B, O, dtype=torch.float32, device=dev)
    assert lib.lbbnn_elbo_bce_loss_backward(g.data_ptr(), pv.data_ptr(), pv.stride(0), yv.data_ptr(), yv.stride(0), B, O,
                                            ctypes.c_float(scale), gp2.data_ptr(), None, None, _stream(dev)) == 0
    assert _same(gp2, gp)
    # lbbnn_sigmoid_backward of g_probs is the fused g_logits bit for bit (where the target is valid)
    sb = bnn.ops.sigmoid_backward(gp, pv)
    ok = ref.target_ok(y)
    assert _same(sb.cpu()[ok], gl.cpu()[ok])
    if bad:
        assert bool((gp.cpu()[~ok] == 0).all()) and bool((gl.cpu()[~ok] == 0).all())
    if B * O >= 15:
        # the saturation entries: p == 1 against y = 0 is a g_probs of 1 / 1e-12f and a g_logits of exactly 0
        flat_p, flat_y = p.reshape(-1)[:15], y.reshape(-1)[:15]
        sat = (flat_p == 1) & (flat_y == 0)
        assert bool(sat.any())
        assert bool((gl.cpu().reshape(-1)[:15][sat] == 0).all())
        assert bool((gp.cpu().reshape(-1)[:15][sat] == torch.tensor(1.0) / torch.tensor(1e-12)).all())


# ------------------------------------------------------------------------------------------- 3. the network forward
NETS = {"lrt-20-1": ("lrt", (20, 1)), "mnf-20-1": ("mnf", (20, 1)), "lrt-12-8-1": ("lrt", (12, 8, 1)),
        "mnf-12-8-3": ("mnf", (12, 8, 3)), "mnf-12-8-1": ("mnf", (12, 8, 1)),
        "lrt-8-12-20-1": ("lrt", (8, 12, 20, 1)), "mnf-8-12-20-1": ("mnf", (8, 12, 20, 1))}


def _make(bnn, name, dev, head="sigmoid", seed=11, spread=True):
    family, dims = NETS[name]
    torch.manual_seed(seed)
    if family == "lrt":
        net = bnn.lrt.BayesianNetwork(dims, head=head)
    else:
        net = bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar", head=head)
    if spread:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for l in net._layers():
                l.weight_mu.copy_(torch.randn(l.out_features, l.in_features, generator=g) * (2.0 / l.in_features ** 0.5))
                l.lambdal.copy_(torch.empty(l.out_features, l.in_features).uniform_(-3, 3, generator=g))
                if family == "mnf":
                    l.q0_mean.copy_(1.0 + 0.1 * torch.randn(l.in_features, generator=g))
    return net.to(dev)


def _inject(net, B, dev, seed):
    g = torch.Generator().manual_seed(seed)
    for l in net._layers():
        n = {"eps_out": torch.randn(B, l.out_features, generator=g)}
        if l._mnf:
            n.update(eps_z=torch.randn(1, l.in_features, generator=g), eps_z2=torch.randn(1, l.in_features, generator=g),
                     eps_act=torch.randn(l.out_features, generator=g))
        l.noise = {k: v.to(dev) for k, v in n.items()}


def _per_layer_logits(net, x, sample):
    """The last layer's logits from the per-layer calls.  The layers of a network share ONE Philox offset (their streams differ
    by layer id): the calls here leave the live offset where it is, as the network's own forward does until its last layer."""
    h, layers = x, net._layers()
    try:
        for i, l in enumerate(layers):
            l._advance_rng = False
            h = l(h, sample, _relu=(i < len(layers) - 1))
    finally:
        for l in layers:
            l._advance_rng = True
    return h


@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
@pytest.mark.parametrize("B", (1, 7, 400))
@pytest.mark.parametrize("name", ("lrt-20-1", "mnf-20-1", "lrt-12-8-1", "mnf-12-8-3"))
def test_network_forward_is_the_head_of_the_per_layer_logits(bnn, dev, precision, name, B, prec):
    from bnn_amd import graphs
    dims = NETS[name][1]
    net, twin = _make(bnn, name, dev), _make(bnn, name, dev, head="log_softmax")
    assert net.head == "sigmoid" and twin.head == "log_softmax"
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(B)).to(dev)
    for m in (net, twin):
        m.train()
        _inject(m, B, dev, 5)
    precision(prec)
    for sample in (True, False):
        with torch.no_grad():
            want = bnn.ops.binary_head(_per_layer_logits(net, x, sample))
            out = net(x, sample=sample)                                          # the no-grad fused forward
            kl = net.kl().clone()
            twin(x, sample=sample)
            assert _same(kl.reshape(1), twin.kl().reshape(1))
        assert out.shape == (B, dims[-1]) and _same(out, want), (name, B, prec, sample)
        assert bool(((out >= 0) & (out <= 1)).all())
        out_g = net(x, sample=sample)                                            # the autograd forward
        assert out_g.requires_grad and _same(out_g, want)
        kl_g = net.kl().detach().clone()
        twin_g = twin(x, sample=sample)
        assert _same(kl_g.reshape(1), twin.kl().detach().reshape(1))
        del out_g, twin_g
    with torch.no_grad():
        plan = graphs.LaunchPlan(net, x, sample=True)
        p_out, p_kl = plan()
        assert _same(p_out, bnn.ops.binary_head(_per_layer_logits(net, x, True))) and _same(p_kl.reshape(1), kl.reshape(1))


# ------------------------------------------------------------------------------------------- 4. backward plumbing
@pytest.mark.parametrize("B", (7, 400))
@pytest.mark.parametrize("name", ("lrt-20-1", "mnf-12-8-1"))
def test_loss_hand_over_equals_sigmoid_backward_bitwise(bnn, dev, name, B):
    from bnn_amd import losses
    dims = NETS[name][1]
    net = _make(bnn, name, dev).train()
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, dims[0], generator=g).to(dev)
    y = (torch.rand(B, 1, generator=g) > 0.5).float().to(dev)
    grads = []
    for path in ("A", "B"):
        bnn.manual_seed(5)
        net.zero_grad(set_to_none=True)
        before = dict(losses.HANDOVER)
        out = net(x, sample=True)
        if path == "A":
            loss = bnn.elbo_bce_loss(out, y, net.kl(), 5)
        else:
            loss = torch.nn.BCELoss(reduction="sum")(out.clone(), y) + net.kl() / 5
        loss.backward()
        took = losses.HANDOVER["taken"] - before["taken"]
        ran = losses.HANDOVER["sigmoid_backward"] - before["sigmoid_backward"]
        assert (took, ran) == ((1, 0) if path == "A" else (0, 1)), (path, took, ran)
        grads.append(({k: p.grad.clone() for k, p in net.named_parameters()}, loss.detach().clone()))
        del out, loss
    assert len(losses._HEAD_GRAD) == 0                                           # the entry was taken, nothing is held
    for k in grads[0][0]:
        assert _same(grads[0][0][k].reshape(-1), grads[1][0][k].reshape(-1)), k
        assert bool(torch.isfinite(grads[0][0][k]).all()), k
    assert any(float(v.abs().max()) > 0 for v in grads[0][0].values())
    print("hand-over %s B=%d: loss fused %.9g, torch %.9g" % (name, B, float(grads[0][1]), float(grads[1][1])))


# ------------------------------------------------------------------------------------------- 5. the captured step
def test_graphed_train_step_with_the_fused_loss_equals_eager_subprocess():
    """make_graphed_train_step on LRT (20, 1), B = 400, with elbo_bce_loss and stats: three replays leave the parameters and
    the counts of three eager steps from the same state, bit for bit.  Own process (capture wants a clean autograd state)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, copy, torch
sys.path.insert(0, %r)
import bnn_amd
from bnn_amd import layers
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.lrt.BayesianNetwork((20, 1), head="sigmoid", lambdal_init=(1.5, 2.5)).to(dev).train()
init = copy.deepcopy(net.state_dict())
opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-2)
g = torch.Generator().manual_seed(1)
x = torch.randn(400, 20, generator=g).to(dev); y = (torch.rand(400, 1, generator=g) > 0.5).float().to(dev)
st = torch.zeros(4, dtype=torch.int32, device=dev)
lf = lambda n, a, b: bnn_amd.elbo_bce_loss(n(a, sample=True), b, n.kl(), 5, stats=st)
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)

def reset():
    net.load_state_dict(init)
    for s in opt.state.values():
        s["exp_avg"].zero_(); s["exp_avg_sq"].zero_()
    for gr in opt.param_groups:
        gr["step_dev"].zero_()
    st.zero_()
    bnn_amd.manual_seed(7)

reset()
gl = [float(step(x, y)) for _ in range(3)]
gp = {k: v.detach().clone() for k, v in net.named_parameters()}
gs = st.tolist()
reset()
el = []
for _ in range(3):
    opt.zero_grad(set_to_none=True)
    loss = lf(net, x, y)
    with layers.vector_backward_overlap():
        loss.backward()
    opt.step()
    el.append(float(loss.detach()))
del loss
torch.cuda.synchronize()
assert gl == el, (gl, el)
assert len(set(gl)) == 3
assert gs == st.tolist() and gs[1] == 1200 and 0 < gs[0] <= 1200 and gs[2] == 0 and gs[3] == 0, (gs, st.tolist())
for k, v in net.named_parameters():
    assert torch.equal(v.detach(), gp[k]), k
print("BCEGRAPH_OK", gl, gs)
""" % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BCEGRAPH_OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])
    print(r.stdout.strip().splitlines()[-1])


# ------------------------------------------------------------------------------------------- 6. ensembles
@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
@pytest.mark.parametrize("B,S", ((1, 10), (100, 10), (257, 1), (5, 3)))
@pytest.mark.parametrize("name", ("lrt-20-1", "mnf-12-8-1", "lrt-8-12-20-1", "mnf-8-12-20-1"))
def test_ensembles_agree_and_log_probs_come_from_the_logits(bnn, dev, precision, name, B, S, prec):
    ev = bnn.evaluate
    dims = NETS[name][1]
    net = _make(bnn, name, dev).eval()
    twin = _make(bnn, name, dev, head="log_softmax").eval()
    precision(prec)
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(B)).to(dev)
    st = bnn.ops.RngState.get(dev)
    fz = ev.freeze(net)
    assert fz.head == "sigmoid"

    def run(fn):
        bnn.manual_seed(9)
        out = fn()
        off = st.t.clone()
        return out.clone(), off

    loop, off_l = run(lambda: ev.ensemble_forward(net, x, S, batched=False))
    bat, off_b = run(lambda: ev.ensemble_forward(net, x, S, batched=True))
    frz, off_f = run(lambda: fz.ensemble(x, S))
    _, off_t = run(lambda: ev.ensemble_forward(twin, x, S, batched=True))
    assert torch.equal(off_l, off_b) and torch.equal(off_l, off_f) and torch.equal(off_l, off_t)   # the head draws nothing
    assert loop.shape == bat.shape == frz.shape == (S, B, 1)
    assert bool(((loop >= 0) & (loop <= 1)).all())
    bar = (5e-6 if prec == "fp32" else 2e-5) * float(loop.abs().max())
    d_b, d_f = float((bat - loop).abs().max()), float((frz - loop).abs().max())
    print("ensembles %s B=%d S=%d %s: batched - loop %.3g (bitwise %s), frozen - loop %.3g (bitwise %s), bar %.3g"
          % (name, B, S, prec, d_b, _same(bat, loop), d_f, _same(frz, loop), bar))
    assert d_b <= bar and d_f <= bar
    # the members' logits of the batched form are the loop's bit for bit (test_ensemble_batched_equals_loop_bitwise) and the
    # head is one elementwise kernel over them in both forms: the same bits
    assert _same(bat, loop)
    if S > 1:
        for mm in (2, 3):
            chunked, _ = run(lambda: fz.ensemble(x, S, max_members=mm))
            assert _same(chunked, frz)
    one, _ = run(lambda: fz(x, sample=True))
    assert _same(one, frz[0])
    # log_probs=True: (S, B, 2) from the logits of the same members, by the kernel that makes the probabilities
    for what, fn in (("loop", lambda: ev.ensemble_forward(net, x, S, batched=False, log_probs=True)),
                     ("batched", lambda: ev.ensemble_forward(net, x, S, batched=True, log_probs=True)),
                     ("frozen", lambda: fz.ensemble(x, S, log_probs=True))):
        lp, off = run(fn)
        assert lp.shape == (S, B, 2) and torch.equal(off, off_l) and bool(torch.isfinite(lp).all()), what
        if what == "loop":
            lp_loop = lp
        elif what == "batched":
            assert _same(lp, lp_loop)
        elif S > 1:
            assert _same(run(lambda: fz.ensemble(x, S, max_members=2, log_probs=True))[0], lp)
        assert float((lp.double().exp().sum(-1) - 1).abs().max()) <= 1e-6, what
        # the probabilities of the same call are 1 / (1 + exp(-x)); its logits x = lp[1] - lp[0] up to rounding: the two agree
        probs = {"loop": loop, "batched": bat, "frozen": frz}[what]
        assert float((lp[..., 1:].double().exp() - probs.double()).abs().max()) <= 2e-6, what
    # ... and bitwise lbbnn_binary_head's logp2 of the logits: the twin's single unit is log_softmax'ed to 0, so the logits are
    # taken from the per-layer calls of member 0
    bnn.manual_seed(9)
    with torch.no_grad():
        logits0 = _per_layer_logits(net, x, True)
    lp_loop, _ = run(lambda: ev.ensemble_forward(net, x, S, batched=False, log_probs=True))
    assert _same(lp_loop[0], bnn.ops.binary_head(logits0, log_probs=True, want_probs=False))
    assert _same(loop[0], bnn.ops.binary_head(logits0))


@pytest.mark.parametrize("name", ("lrt-20-1", "mnf-12-8-1"))
def test_frozen_mpm_model_and_refresh(bnn, dev, name):
    ev = bnn.evaluate
    dims = NETS[name][1]
    net = _make(bnn, name, dev).eval()
    x = torch.rand(100, dims[0], generator=torch.Generator().manual_seed(1)).to(dev)
    fz = ev.freeze(net, "mpm")
    assert fz.head == "sigmoid" and fz.gates == "mpm"
    total = sum(a * b for a, b in zip(dims[:-1], dims[1:]))
    kept = [int((l.lambdal > 0).sum()) for l in net._layers()]
    assert fz.kept == kept and fz.density == sum(kept) / total
    bnn.manual_seed(3)
    out = fz.ensemble(x, 4)
    assert out.shape == (4, 100, 1) and bool(((out >= 0) & (out <= 1)).all())
    mean = fz(x, sample=False)
    assert mean.shape == (100, 1) and bool(((mean >= 0) & (mean <= 1)).all())
    with torch.no_grad():
        net.l1.lambdal.fill_(-1.0)
    fz.refresh()
    assert fz.kept[0] == 0 and fz.head == "sigmoid"
    assert fz.ensemble(x, 2, log_probs=True).shape == (2, 100, 2)


# ------------------------------------------------------------------------------------------- 7. metrics
DBL = 1e-12        # tests/test_eval_metrics_gpu.py, tests/test_eval_uncertainty_gpu.py: double sums of exact fp32 terms


def _np(t):
    return t.detach().cpu().numpy()


def _close_sum(got, terms, what):
    terms = np.asarray(terms, dtype=np.float64)
    want = float(terms.sum()) if terms.size else 0.0
    assert np.isfinite(want) and abs(got - want) <= DBL * float(np.abs(terms).sum()), (what, got, want)


def test_metrics_take_the_binary_head_as_two_classes(bnn, dev):
    ev = bnn.evaluate
    S, B = 10, 100
    net = _make(bnn, "lrt-20-1", dev).eval()
    fz = ev.freeze(net)
    g = torch.Generator().manual_seed(2)
    data = [(torch.randn(B, 20, generator=g).to(dev), (torch.rand(B, generator=g) > 0.5).float().to(dev)) for _ in range(2)]
    acc, unc = ev.EvalAccumulator(2, S, dev), ev.UncertaintyAccumulator(2, S, dev)
    rec, rows_u = [], []
    inner, inner_u = acc.update, unc.update

    def update(o, t, mo=None):
        rec.append((o.clone(), t.clone(), None if mo is None else mo.clone()))
        return inner(o, t, mo)

    def update_u(o, t=None):
        rows = inner_u(o, t)
        rows_u.append({k: _np(v) for k, v in rows.items()})
        return rows

    acc.update, unc.update = update, update_u
    bnn.manual_seed(13)
    res = ev.evaluate_batches(fz, data, S, acc=acc, uncertainty=unc)
    assert len(rec) == 2 and all(o.shape == (S, B, 2) and t.dtype == torch.int64 and mo.shape == (B, 2) for o, t, mo in rec)
    # the blocks are the frozen model's 2-class log-probabilities from the same offsets
    bnn.manual_seed(13)
    for (x, y), (o, t, mo) in zip(data, rec):
        assert _same(fz.ensemble(x, S, log_probs=True), o) and torch.equal(t, y.long())
        assert _same(fz(x, sample=False, log_probs=True), mo)
    parts = [mref.metrics(_np(o), _np(t), _np(mo)) for o, t, mo in rec]
    rr = mref.add_totals(parts)
    for k in mref.COUNT_NAMES:
        assert res[k] == rr[k], k
    assert res["rows"] == 2 * B == res["rows_with_target"] and res["bad_targets"] == 0
    assert np.array_equal(res["correct_member"], rr["correct_member"]) and np.array_equal(res["confusion"], rr["confusion"])
    assert res["confusion"].shape == (2, 2)
    _close_sum(res["nll_sum"], rr["nll_terms"], "nll_sum")
    uparts = [uref.totals(r, _np(t), 2, unc.conf_bins, unc.hist_bins) for r, (_, t, _) in zip(rows_u, rec)]
    ur = uref.add_totals(uparts)
    for k in uref.COUNT_NAMES:
        if k not in ("rows", "rows_with_target", "bad_targets"):
            assert res[k] == ur[k], k
    for k in ("bin_rows", "bin_rows_with_target", "bin_correct"):
        assert np.array_equal(res[k], ur[k]), k
    for k in uref.SUM_NAMES:
        _close_sum(res[k + "_sum"], ur["terms"][k], k)
    for i, k in enumerate(uref.SCORES):
        assert np.array_equal(res["histograms"][k]["counts"], ur["hist"][i]), k
    # ensemble_eval speaks the same two classes
    bnn.manual_seed(13)
    r = ev.ensemble_eval(fz, data[0][0], data[0][1], S)
    assert _same(r["outputs"], rec[0][0]) and r["pred_ensemble"].shape == (B,)
    bnn.manual_seed(13)
    r2 = ev.ensemble_eval(net, data[0][0], data[0][1].reshape(B, 1), S)
    assert r2["outputs"].shape == (S, B, 2) and 0 <= r2["correct_ensemble"] <= B


def test_metrics_refuse_a_multi_label_head(bnn, dev):
    ev = bnn.evaluate
    net = _make(bnn, "mnf-12-8-3", dev).eval()
    x, y = torch.rand(8, 12, device=dev), torch.zeros(8, device=dev)
    out = ev.ensemble_forward(net, x, 3)                                         # the head itself works
    assert out.shape == (3, 8, 3) and bool(((out >= 0) & (out <= 1)).all())
    fz = ev.freeze(net)
    assert fz.ensemble(x, 3).shape == (3, 8, 3)
    for model in (net, fz):
        with pytest.raises(ValueError, match="multi-label"):
            ev.evaluate_batches(model, [(x, y)], 3)
        with pytest.raises(ValueError, match="multi-label"):
            ev.ensemble_eval(model, x, y, 3)
        with pytest.raises(ValueError, match="one output unit"):
            ev.ensemble_forward(model, x, 3, log_probs=True)
    with pytest.raises(ValueError, match="multi-label"):
        bnn.graphs.make_graphed_eval_step(fz, x, y, 3, ev.EvalAccumulator(2, 3, dev))
    with pytest.raises(ValueError, match="sigmoid"):
        ev.ensemble_forward(_make(bnn, "lrt-20-1", dev, head="log_softmax").eval(), torch.rand(8, 20, device=dev), 3, log_probs=True)


def test_graphed_eval_step_equals_eager_passes(bnn, dev):
    ev = bnn.evaluate
    S, B = 10, 100
    fz = ev.freeze(_make(bnn, "lrt-20-1", dev).eval())
    g = torch.Generator().manual_seed(4)
    data = [(torch.randn(B, 20, generator=g).to(dev), (torch.rand(B, generator=g) > 0.5).float().to(dev)) for _ in range(2)]
    mk = lambda: (ev.EvalAccumulator(2, S, dev), ev.UncertaintyAccumulator(2, S, dev))
    acc_g, u_g = mk()
    step = bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], S, acc_g, uncertainty=u_g)
    bnn.manual_seed(13)
    got = [{k: v.clone() for k, v in step(x, y).items()} for x, y in data]
    acc_e, u_e = mk()
    bnn.manual_seed(13)
    res_e = ev.evaluate_batches(fz, data, S, acc=acc_e, uncertainty=u_e)
    assert torch.equal(acc_g._totals, acc_e._totals) and torch.equal(u_g._totals, u_e._totals)      # every total, bit for bit
    assert acc_g.updates == 2 == u_g.updates and acc_g.result()["rows"] == 2 * B == res_e["rows"]
    assert acc_g.result()["correct_ensemble"] == res_e["correct_ensemble"]
    assert got[0]["mean_log_probs"].shape == (B, 2) and not torch.equal(got[0]["mean_log_probs"], got[1]["mean_log_probs"])
