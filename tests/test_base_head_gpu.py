"""GPU tier of the baseline network's sigmoid head (base.BayesianNetwork(head="sigmoid"), the simulation study's 20 -> 1 logistic
regression): the new path is pinned, bit for bit, to parts that have their own fp64 tests -- the layers' ``sample_forward``
(tests/test_base_hip_draws_gpu.py), lbbnn_binary_head and the fused BCE loss (tests/test_binary_head_gpu.py) -- then compared
with the torch-draw path on the same draws, and followed through the ensembles, the metrics and a captured training step."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUDY = dict(weight_mu_init=(-0.01, 0.01), lambdal_init=(-0.5, 0.5))
CASES = [((20, 1), 1), ((20, 1), 3), ((20, 1), 400), ((7, 5, 2), 3), ((9, 4, 16), 5)]
PRECS = ("fp32", "bf16x3")                                     # the two precisions of tests/test_binary_head_gpu.py


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


def _make(bnn, dims, dev, seed=11, head="sigmoid"):
    torch.manual_seed(seed)
    kw = STUDY if tuple(dims) == (20, 1) else {}
    return bnn.base.BayesianNetwork(dims, head=head, **kw).to(dev)


def _data(dims, B, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, dims[0], generator=g).to(dev)
    y = (torch.rand(B, dims[-1], generator=g) > 0.5).float()
    return x, (y.reshape(B) if dims[-1] == 1 else y).to(dev)


def _grads(net):
    return {n: p.grad.detach().clone() for n, p in net.named_parameters()}


# ----------------------------------------------------------------------------------------------------- 1. bitwise composition
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dims,B", CASES)
def test_network_is_the_composition_of_its_parts_bitwise(bnn, dev, precision, dims, B, prec):
    from bnn_amd import layers as L, losses, ops
    net = _make(bnn, dims, dev).train()
    x, y = _data(dims, B, dev)
    precision(prec)
    N = 5.0
    st = ops.RngState.get(dev)
    bnn.manual_seed(21)
    rng0 = st.t[:2].clone()
    taken = losses.HANDOVER["taken"]
    res = net.sample_elbo(x, y, draws="hip", num_batches=N)
    assert len(res) == 5
    loss, lp, lq, nll, out = res
    assert int(st.t[1]) == int(rng0[1]) + 1 and out.shape == (B, dims[-1])
    loss.backward()
    assert losses.HANDOVER["taken"] == taken + 1
    got = _grads(net)
    assert set(got) == {n for n, _ in net.named_parameters()} and all(torch.isfinite(g).all() for g in got.values())
    # the same step written out by hand from the parts, at the same Philox snapshot
    net.zero_grad(set_to_none=True)
    ls = net._layers()
    h, lp2, lq2 = x, None, None
    for k, l in enumerate(ls):
        h, a, b = l.sample_forward(h, activation="relu" if k < len(ls) - 1 else None, rng=rng0)
        lp2, lq2 = (a, b) if lp2 is None else (lp2 + a, lq2 + b)
    probs = L._SigmoidHeadFn.apply(h)
    assert torch.equal(probs.detach(), ops.binary_head(h.detach()))
    assert torch.equal(probs.detach(), out.detach())
    nll2 = losses.elbo_bce_loss(probs, y)
    loss2 = nll2 + (lq2 - lp2) / N
    for a, b in ((loss, loss2), (lp, lp2), (lq, lq2), (nll, nll2)):
        assert torch.equal(a.detach(), b.detach())
    loss2.backward()
    assert losses.HANDOVER["taken"] == taken + 2
    want = _grads(net)
    for n in want:
        assert torch.equal(got[n], want[n]), n
    # forward(): the head of the last layer's logits, probabilities of the layer's shape
    with torch.no_grad():
        net.eval()
        p = net(x, *[None] * len(ls), sample=False)
        assert p.shape == (B, dims[-1]) and bool(((p >= 0) & (p <= 1)).all())
    assert [tuple(a.shape) for a in net.inclusion_probabilities()] == [(o, i) for i, o in zip(dims[:-1], dims[1:])]


# ------------------------------------------------------------------------------------------- 2. hip draws against torch draws
@pytest.mark.parametrize("dims,B", [((20, 1), 400), ((20, 8, 1), 100)])
def test_hip_draws_vs_torch_path_on_the_same_draws(bnn, dev, dims, B):
    """tests/test_base_hip_draws_gpu.py::test_network_hip_draws_vs_torch_path_on_the_same_draws with the sigmoid head and a float
    target; that test's bars (values 2e-5, gradients 5e-4)."""
    net = _make(bnn, dims, dev, seed=0).train()
    x, y = _data(dims, B, dev, seed=5)
    st = bnn.ops.RngState.get(dev)
    rng0 = st.t[:2].clone()
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    loss_h, lp_h, lq_h, nll_h, out_h = net.sample_elbo(x, y, draws="hip", stats=stats)
    loss_h.backward()
    assert stats.tolist()[1:] == [B, 0, 0] and 0 <= stats.tolist()[0] <= B
    names = ("weight_mu", "weight_rho", "bias_mu", "bias_rho", "pa", "pb")
    layers = net._layers()
    gh = [{n: getattr(l, n).grad.clone() for n in names} for l in layers]
    assert all(torch.isfinite(l.lambdal.grad).all() for l in layers)
    ops = bnn.ops
    for l in layers:
        O, I, Lid = l.out_features, l.in_features, l._layer_id
        l.noise = {"eps_w": ops.philox_normal(rng0, ops.STREAM_EPS_W * 64 + Lid, O, I),
                   "eps_b": ops.philox_normal(rng0, ops.STREAM_EPS_B * 64 + Lid, 0, O),
                   "tau_w": l.tau_w.clone(), "tau_b": l.tau_b.clone()}
        gm = l.gammas.clone()
        l.gamma.rsample = (lambda gm=gm: gm)
    net.zero_grad()
    loss_t, lp_t, lq_t, nll_t, out_t = net.sample_elbo(x, y.long() if dims[-1] == 1 else y)    # an integer 0 / 1 target: .float()
    loss_t.backward()
    for h, t, what in ((loss_h, loss_t, "loss"), (lp_h, lp_t, "lp"), (lq_h, lq_t, "lq"), (nll_h, nll_t, "nll"), (out_h, out_t, "out")):
        e = rel_err(h.detach(), t.detach())
        print("%s B=%d %s: rel err %.3e" % (dims, B, what, e))
        assert e < 2e-5, what
    for li, l in enumerate(layers):
        for n in names:
            e = rel_err(gh[li][n], getattr(l, n).grad)
            print("%s B=%d layer %d d %s: rel err %.3e" % (dims, B, li, n, e))
            assert e < 5e-4, (li, n)
        assert torch.isfinite(l.lambdal.grad).all()
    # a three-layer network with the default head, built in the same process, returns the four values it returned before
    plain = _make(bnn, (20, 6, 5, 3), dev, head="log_softmax").train()
    yi = torch.randint(0, 3, (B,), device=dev)
    assert len(plain.sample_elbo(x, yi, draws="hip")) == 4 and len(plain.sample_elbo(x, yi)) == 4


# ------------------------------------------------------------------------------------------------------------------ 3. ensembles
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dims,B", CASES)
def test_ensemble_members_are_sample_predict_bitwise(bnn, dev, precision, monkeypatch, dims, B, prec):
    ev, ops = bnn.evaluate, bnn.ops
    net = _make(bnn, dims, dev).eval()
    x, _ = _data(dims, B, dev, seed=3)
    precision(prec)
    S, O = 5, dims[-1]
    st = ops.RngState.get(dev)

    def run(fn):
        bnn.manual_seed(9)
        off0 = st.t[:2].clone()
        out = fn()
        assert int(st.t[1]) == int(off0[1]) + S
        return out.clone(), off0

    def member_rng(off0, m):
        r = off0.clone()
        r[1] += m
        return r

    for gates in ("sample", "mpm"):
        outs, off0 = run(lambda: ev.base_ensemble(net, x, S, gates=gates)["outputs"])
        assert outs.shape == (S, B, O) and bool(((outs >= 0) & (outs <= 1)).all())
        for m in range(S):
            assert torch.equal(outs[m], net.sample_predict(x, gates=gates, rng=member_rng(off0, m))), (gates, m)
        fwd, _ = run(lambda: ev.ensemble_forward(net, x, S, gates=gates))
        chunked, _ = run(lambda: ev.ensemble_forward(net, x, S, gates=gates, max_members=2))
        assert torch.equal(fwd, outs) and torch.equal(chunked, outs)
        if O == 1:
            lp, _ = run(lambda: ev.ensemble_forward(net, x, S, gates=gates, log_probs=True))
            lpc, _ = run(lambda: ev.base_ensemble(net, x, S, gates=gates, log_probs=True, max_members=3)["outputs"])
            assert lp.shape == (S, B, 2) and torch.equal(lp, lpc)
            for m in range(S):
                assert torch.equal(lp[m], net.sample_predict(x, gates=gates, rng=member_rng(off0, m), log_probs=True)), (gates, m)
            # both columns against the probabilities of the same members: exp(lp[1]) = p, exp(lp[0]) = 1 - p (fp32 rounding of p)
            assert float((lp[..., 1].double().exp() - outs[..., 0].double()).abs().max()) <= 2e-6
            assert float((lp[..., 0].double().exp() - (1 - outs[..., 0].double())).abs().max()) <= 2e-6
            assert float((lp.double().exp().sum(-1) - 1).abs().max()) <= 1e-6
        else:
            with pytest.raises(ValueError, match="one output unit"):
                ev.ensemble_forward(net, x, S, log_probs=True)
    one, _ = run(lambda: torch.stack([net.sample_predict(x) for _ in range(S)]))       # the live state: one offset per call
    ref, _ = run(lambda: ev.ensemble_forward(net, x, S, batched=False))
    assert torch.equal(one, ref)
    # the loop form (a network with a layer wider than lbbnn_gate_members takes) gives the same members
    batched, _ = run(lambda: ev.base_ensemble(net, x, S)["outputs"])
    monkeypatch.setattr(ops, "GATE_MEMBERS_MAX_LD", 16)
    loop, _ = run(lambda: ev.base_ensemble(net, x, S)["outputs"])
    assert torch.equal(loop, batched)
    if O == 1:
        lpl, _ = run(lambda: ev.base_ensemble(net, x, S, log_probs=True, max_members=2)["outputs"])
        monkeypatch.undo()
        lpb, _ = run(lambda: ev.base_ensemble(net, x, S, log_probs=True)["outputs"])
        assert torch.equal(lpl, lpb)


def test_default_head_still_refuses_log_probs(bnn, dev):
    ev = bnn.evaluate
    net = _make(bnn, (20, 3), dev, head="log_softmax").eval()
    x = torch.rand(4, 20, device=dev)
    with pytest.raises(ValueError):
        ev.ensemble_forward(net, x, 2, log_probs=True)
    with pytest.raises(ValueError):
        ev.base_ensemble(net, x, 2, log_probs=True)
    with pytest.raises(ValueError):
        net.sample_predict(x, log_probs=True)
    out = ev.ensemble_forward(net, x, 2)
    assert out.shape == (2, 4, 3) and float((out.double().exp().sum(-1) - 1).abs().max()) < 1e-5


# --------------------------------------------------------------------------------------------------------------- 4. accumulators
def _same_result(a, b, path=""):
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            _same_result(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b, equal_nan=True), path
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def test_metrics_take_the_one_unit_head_as_two_classes(bnn, dev):
    ev = bnn.evaluate
    S, B = 6, 50
    net = _make(bnn, (20, 1), dev).eval()
    g = torch.Generator().manual_seed(2)
    data = [(torch.randn(B, 20, generator=g).to(dev), (torch.rand(B, generator=g) > 0.5).float().to(dev)) for _ in range(2)]
    acc, unc = ev.EvalAccumulator(2, S, dev), ev.UncertaintyAccumulator(2, S, dev)
    bnn.manual_seed(13)
    res = ev.evaluate_batches(net, data, S, acc=acc, uncertainty=unc)
    # the same (S, B, 2) log-probabilities handed to fresh accumulators directly
    acc2, unc2 = ev.EvalAccumulator(2, S, dev), ev.UncertaintyAccumulator(2, S, dev)
    bnn.manual_seed(13)
    blocks = []
    for x, y in data:
        o = ev.base_ensemble(net, x, S, log_probs=True)["outputs"]
        mean = ev._base_mean_forward(net, x, True)
        assert o.shape == (S, B, 2) and mean.shape == (B, 2)
        # the posterior-mean block is lbbnn_binary_head's 2-class form of the mode-2 logits (weight = alpha * mu) of the layer
        # called by itself, and its probabilities are what the network's own posterior-mean forward returns
        net.l1.alpha = torch.sigmoid(net.l1.lambdal.detach())
        logits = net.l1(x, None, sample=False, medimean=False)
        assert logits.shape == (B, 1)
        assert torch.equal(mean, bnn.ops.binary_head(logits, log_probs=True, want_probs=False))
        assert torch.equal(net(x, None, sample=False), bnn.ops.binary_head(logits))
        assert torch.equal(mean.argmax(1), (logits.reshape(-1) > 0).long())
        acc2.update(o, y.long(), mean)
        unc2.update(o, y.long())
        blocks.append(o.clone())
    want = acc2.result()
    want.update((k, v) for k, v in unc2.result().items() if k not in want)
    _same_result(res, want)
    assert res["rows"] == 2 * B == res["rows_with_target"] and res["bad_targets"] == 0 and res["confusion"].shape == (2, 2)
    # ensemble_eval speaks the same two classes
    bnn.manual_seed(13)
    r = ev.ensemble_eval(net, data[0][0], data[0][1].reshape(B, 1), S)
    assert torch.equal(r["outputs"], blocks[0]) and r["pred_ensemble"].shape == (B,) and r["density"].shape == (S,)
    acc3 = ev.EvalAccumulator(2, S, dev)
    acc3.update(r["outputs"], data[0][1].long(), ev._base_mean_forward(net, data[0][0], True))
    one = acc3.result()
    assert r["correct_ensemble"] == one["correct_ensemble"] and r["correct_posterior_mean"] == one["correct_posterior_mean"]
    # a two-unit head has no class axis
    wide = _make(bnn, (7, 5, 2), dev).eval()
    xw, yw = torch.rand(8, 7, device=dev), torch.zeros(8, device=dev)
    assert ev.ensemble_forward(wide, xw, 3).shape == (3, 8, 2)
    with pytest.raises(ValueError, match="multi-label"):
        ev.evaluate_batches(wide, [(xw, yw)], 3)
    with pytest.raises(ValueError, match="multi-label"):
        ev.ensemble_eval(wide, xw, yw, 3)


# ---------------------------------------------------------------------------------------------------------------- 5. graph replay
def test_graphed_study_step_with_sgd_equals_eager_subprocess():
    """make_graphed_train_step on the study network (20 -> 1, B = 400) with bnn_amd.optim.SGD's eleven groups and the BCE ELBO
    with stats: three replays leave the parameters, the losses and the counts of three eager steps from the same state, bit for
    bit; then the six prior groups' rates go to 0 through the table and stay bitwise under two more replays of the same graph.
    Own process (capture wants a clean autograd state), under a time limit."""
    code = r"""
import sys, copy, torch
sys.path.insert(0, %r)
import bnn_amd
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.base.BayesianNetwork((20, 1), head="sigmoid", weight_mu_init=(-0.01, 0.01), lambdal_init=(-0.5, 0.5)).to(dev).train()
init = copy.deepcopy(net.state_dict())
l = net.l1
slow, fast = ("bias_mu", "bias_rho", "weight_mu", "weight_rho"), ("pa", "pb", "weight_a", "weight_b", "bias_a", "bias_b", "lambdal")
opt = bnn_amd.optim.SGD([dict(params=[getattr(l, n)], lr=1e-4) for n in slow] + [dict(params=[getattr(l, n)], lr=1e-3) for n in fast], lr=0.01)
g = torch.Generator().manual_seed(1)
x = torch.randn(400, 20, generator=g).to(dev); y = (torch.rand(400, generator=g) > 0.5).float().to(dev)
st = torch.zeros(4, dtype=torch.int32, device=dev)
lf = lambda n, a, b: n.sample_elbo(a, b, draws="hip", num_batches=5, stats=st)[0]
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)

def reset():
    net.load_state_dict(init)
    for gr in opt.param_groups:
        gr["step_dev"].zero_()
    st.zero_()
    bnn_amd.manual_seed(7)

reset()
gl = [float(step(x, y)) for _ in range(3)]
gp = {k: v.detach().clone() for k, v in net.named_parameters()}
gs = st.tolist()
for i in range(4, 10):
    opt.param_groups[i]["lr"] = 0.0
for _ in range(2):
    step(x, y)
torch.cuda.synchronize()
for i in range(4, 10):
    p = opt.param_groups[i]["params"][0]
    name = [k for k, v in net.named_parameters() if v is p][0]
    assert torch.equal(p.detach(), gp[name]), name
assert not torch.equal(l.weight_mu.detach(), gp["l1.weight_mu"]) and not torch.equal(l.lambdal.detach(), gp["l1.lambdal"])
for i in range(4, 10):
    opt.param_groups[i]["lr"] = 1e-3
reset()
el = []
for _ in range(3):
    opt.zero_grad(set_to_none=True)
    loss = lf(net, x, y)
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
print("BASEHEAD_GRAPH_OK", gl, gs)
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "BASEHEAD_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])
