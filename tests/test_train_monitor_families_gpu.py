"""GPU tier of the training monitor for the BCE loss, the baseline family and variational dropout:
lbbnn_elbo_bce_loss_monitor behind elbo_bce_loss(monitor=...), the guarded optimizer steps behind it, the same step inside
one captured graph, base.sample_elbo(monitor=...) and vd.loss_fn(monitor=...).  Bitwise where the issue is "the same
arithmetic" (loss, stats, gradients, updates); the counts exactly and the fp64 sums to the worst-case rounding of their
additions against the numpy restatements tests/train_monitor_bce_ref.py and tests/train_monitor_ref.py.  The cases that
capture a HIP graph run once each, in a process of their own, under a time limit."""
import math
import os
import subprocess
import sys

import pytest
import torch

import train_monitor_bce_ref as bref
import train_monitor_ref as cref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BATCHES = 5.0
EPS64 = 2.0 ** -53                 # |got - ref| <= n_terms * EPS64 * sum|terms|: the worst case of ANY order of n_terms additions
FUSED = 4 * 2.0 ** -24             # fused against unfused loss: one rounding against three (nll, division, add), each 2^-24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _same(a, b):
    """The same bits (NaN payloads included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _kernel_terms(p, y):
    """The (B, O) fp32 terms as the loss kernel itself forms them: lbbnn_elbo_bce_loss on each element alone (B = O = 1, no kl:
    *loss is (float)(double)term, the term).  The device's logf is not numpy's, and not torch.log's either -- on an MI355X it
    differs from torch.log in the last bit for a third of the probabilities, while log1pf agrees -- so the terms a float64
    reference adds up have to come from the entry point whose bits the monitored loss promises.  Bad targets give 0."""
    import ctypes
    from bnn_amd import _lib
    pc, yc = p.detach().contiguous(), y.detach().contiguous()
    t = torch.zeros(pc.numel(), dtype=torch.float32, device=p.device)
    f, stream = _lib.lib().lbbnn_elbo_bce_loss, torch.cuda.current_stream(p.device).cuda_stream
    zero = ctypes.c_float(0.0)
    for i in range(pc.numel()):
        assert f(pc.data_ptr() + 4 * i, 1, yc.data_ptr() + 4 * i, 1, 1, 1, None, zero, t.data_ptr() + 4 * i, None, 0, stream) == 0
    return t.cpu().numpy().reshape(tuple(p.shape))


def _feq(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
# a lone thread; a few; one short of, and one past, the 1024-thread stride; several units; all 16; a column slice (ldp = 8)
SHAPES = [(1, 1, None), (5, 1, None), (1023, 1, None), (1025, 1, None), (70, 3, None), (64, 16, None), (70, 3, 8)]


def _three_steps(B, O, dev):
    """[(logits, target, kl)]: a clean step; one with a NaN probability (the first element) and a target of 1.5 (the last
    element; for one element the same one); one with kl = inf."""
    g = torch.Generator().manual_seed(1000 * B + O)
    out = []
    for i, kl in enumerate((12.5, 3.25, float("inf"))):
        x = torch.randn(B, O, generator=g) * 2
        y = (torch.rand(B, O, generator=g) > 0.5).float()
        if i == 1:
            x.view(-1)[0] = float("nan")
            y.view(-1)[-1] = 1.5
        out.append((x.to(dev), y.to(dev), kl))
    return out


@pytest.mark.parametrize("B,O,ld", SHAPES)
def test_kernel_loss_stats_gradients_and_totals(bnn, dev, B, O, ld):
    from bnn_amd import layers, losses
    mons = [bnn.TrainMonitor(O, dev), bnn.TrainMonitor(O, dev)]
    st_plain = torch.zeros(4, dtype=torch.int32, device=dev)
    st_mon = torch.zeros(4, dtype=torch.int32, device=dev)
    steps, guards, last = [], [], None
    for x, y, klv in _three_steps(B, O, dev):
        got = []
        for mon in (None, mons[0]):
            kl = torch.tensor(klv, device=dev, requires_grad=True)
            if ld is None:                                     # probabilities out of the sigmoid head: the hand-over route
                leaf = x.clone().requires_grad_(True)
                probs = layers._SigmoidHeadFn.apply(leaf)
            else:                                              # a leaf of probabilities, the loss reads a column slice of it
                leaf = torch.full((B, ld), 0.5, device=dev)
                leaf[:, :O] = torch.sigmoid(x)
                leaf.requires_grad_(True)
                probs = leaf[:, :O]
            probs.retain_grad()
            taken = losses.HANDOVER["taken"]
            loss = bnn.elbo_bce_loss(probs, y, kl, N_BATCHES, stats=st_plain if mon is None else st_mon, monitor=mon)
            loss.backward()
            assert losses.HANDOVER["taken"] - taken == (1 if ld is None else 0)
            got.append((loss.detach().clone(), probs.grad.clone(), leaf.grad.clone(), kl.grad.clone(), probs.detach().clone()))
        for k, what in enumerate(("loss", "g_probs", "g_logits / g_leaf", "g_kl")):
            assert _same(got[0][k], got[1][k]), (what, klv)
        assert torch.equal(st_plain, st_mon)
        guards.append(int(mons[0]._guard))
        with torch.no_grad():                                  # the same call into a second monitor: two runs from zero
            bnn.elbo_bce_loss(probs.detach(), y, kl.detach(), N_BATCHES, monitor=mons[1])
        p = got[1][4]
        steps.append(bref.step(p.cpu().numpy(), y.cpu().numpy(), klv, 1.0 / N_BATCHES, terms=_kernel_terms(p, y)))
        last = float(got[1][0])
    # what the reference says of the three steps: the NaN probability costs 100 and leaves the loss finite unless n == 1
    # drops it with its bad target; kl = inf does not
    assert steps[0]["finite"] and not steps[2]["finite"]
    assert guards == [0 if s["finite"] else 1 for s in steps], (guards, [s["finite"] for s in steps])
    assert guards == [0, 0, 1]
    want = cref.totals(steps)
    got = mons[0].result(strict=False)
    print("B=%d O=%d ld=%s counts %s" % (B, O, ld, {k: got[k] for k in cref.COUNT_NAMES}))
    for k in cref.COUNT_NAMES:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["rows"] == 3 * B * O and got["bad_targets"] == 1 and got["nonfinite_rows"] == 1 and got["nonfinite_steps"] == 1
    assert st_mon.tolist() == [got["correct"], got["rows"], got["bad_targets"], got["nonfinite_rows"]]
    n_add = sum(s["n_terms"] + 2 for s in steps if s["finite"])            # every addition behind a total, the kl terms too
    for k in cref.SUM_NAMES:
        bound = n_add * EPS64 * want[k + "_abs"]
        print("%s got %.17g ref %.17g |diff| %.3g bound %.3g" % (k, got[k], want[k], abs(got[k] - want[k]), bound))
        assert abs(got[k] - want[k]) <= bound, k
    s2 = steps[2]
    assert abs(got["last_nll"] - s2["nll"]) <= s2["n_terms"] * EPS64 * s2["abs_terms"]
    assert _feq(got["last_loss"], s2["loss"]) and _feq(got["last_loss"], last) and got["last_loss"] == float("inf")
    assert torch.equal(mons[0]._totals, mons[1]._totals) and torch.equal(mons[0]._guard, mons[1]._guard)


def test_last_values_follow_every_step(bnn, dev):
    """last_nll / last_loss after a FINITE step equal the reference's to the fp64 bound (the kernel test ends on kl = inf)."""
    B, O = 70, 3
    mon = bnn.TrainMonitor(O, dev)
    for x, y, klv in _three_steps(B, O, dev)[:2]:
        p = torch.sigmoid(x)
        loss = bnn.elbo_bce_loss(p, y, torch.tensor(klv, device=dev), N_BATCHES, monitor=mon)
        s = bref.step(p.cpu().numpy(), y.cpu().numpy(), klv, 1.0 / N_BATCHES, terms=_kernel_terms(p, y))
        r = mon.result(strict=False)
        bound = (s["n_terms"] + 1) * EPS64 * (s["abs_terms"] + abs(s["kl_term"]))
        print("last_nll %.17g ref %.17g, last_loss %.17g ref %.17g, bound %.3g" % (r["last_nll"], s["nll"], r["last_loss"], s["loss"], bound))
        assert abs(r["last_nll"] - s["nll"]) <= s["n_terms"] * EPS64 * s["abs_terms"]
        assert r["last_loss"] == float(loss) and abs(r["last_loss"] - s["loss"]) <= bound


# ------------------------------------------------------------------------------------------------------------------- 2. the guard
def _opt_state(opt, ps):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [v.clone() for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
    return out + [opt._tables()["steps"].clone()]


def _all_same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["Adam", "SGD"])
def test_a_step_with_a_nan_kl_is_skipped_on_the_device(bnn, dev, name):
    torch.manual_seed(0)
    net = bnn.lrt.BayesianNetwork((8, 1), head="sigmoid").to(dev).train()
    ps = list(net.parameters())
    opt = getattr(bnn.optim, name)(ps, lr=1e-2, **(dict(momentum=0.9) if name == "SGD" else {}))
    mon = bnn.TrainMonitor(1, dev)
    opt.set_guard(mon)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 8, generator=g).to(dev)
    y = (torch.rand(5, 1, generator=g) > 0.5).float().to(dev)
    bnn.manual_seed(3)

    def step(poison):
        opt.zero_grad(set_to_none=True)
        out = net(x, sample=True)
        kl = net.kl()
        loss = bnn.elbo_bce_loss(out, y, kl * float("nan") if poison else kl, N_BATCHES, monitor=mon)
        loss.backward()
        opt.step()
        return float(loss.detach())

    assert math.isfinite(step(False))
    s1 = _opt_state(opt, ps)
    assert math.isnan(step(True))
    assert _all_same(_opt_state(opt, ps), s1)                  # no parameter, moment or step counter moved
    r = mon.result()
    assert (r["steps"], r["nonfinite_steps"], r["skipped_steps"], int(mon._guard)) == (2, 1, 1, 1)
    assert math.isfinite(step(False))
    s3 = _opt_state(opt, ps)
    moved = [not torch.equal(a, b) for a, b in zip(s1[:len(ps)], s3[:len(ps)])]         # the next clean step updates
    assert any(moved) and all(m for m, p in zip(moved, ps) if p.grad is not None and bool((p.grad != 0).any()))
    assert float(s3[-1][0]) == float(s1[-1][0]) + 1
    r = mon.result()
    assert (r["steps"], r["nonfinite_steps"], r["skipped_steps"], int(mon._guard)) == (3, 1, 1, 0)
    assert all(bool(torch.isfinite(t).all()) for t in s3)


# -------------------------------------------------------------------------------------------------------------------- 3. the graph
def _run_child(code, token):
    code = code.replace("@ROOT@", repr(ROOT)).replace("@TESTS@", repr(os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and token in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])


def test_monitored_bce_step_under_a_graph_subprocess():
    """lrt (8, 1) with a sigmoid head, B = 5, optim.Adam behind the monitor's guard, elbo_bce_loss(monitor=mon) in one captured
    step: after mon.reset(), four replays leave bitwise the totals of four eager steps from the same parameters and Philox
    state."""
    _run_child(r"""
import sys, copy, torch
sys.path.insert(0, @ROOT@)
import bnn_amd
from bnn_amd import layers
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.lrt.BayesianNetwork((8, 1), head="sigmoid").to(dev).train()
init = copy.deepcopy(net.state_dict())
mon = bnn_amd.TrainMonitor(1, dev)
opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-2)
opt.set_guard(mon)
g = torch.Generator().manual_seed(1)
xs = [torch.randn(5, 8, generator=g).to(dev) for _ in range(4)]
ys = [(torch.rand(5, 1, generator=g) > 0.5).float().to(dev) for _ in range(4)]
lf = lambda n, a, b: bnn_amd.elbo_bce_loss(n(a, sample=True), b, n.kl(), 5, monitor=mon)
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, xs[0], ys[0])
assert mon.result()["steps"] == 3                      # the factory's eager warm-up steps are real steps

def reset():
    net.load_state_dict(init)
    for s in opt.state.values():
        s["exp_avg"].zero_(); s["exp_avg_sq"].zero_()
    for gr in opt.param_groups:
        gr["step_dev"].zero_()
    bnn_amd.manual_seed(7)
    mon.reset()

reset()
gl = [float(step(xs[i], ys[i])) for i in range(4)]
graphed = mon._totals.clone()
pg = [p.detach().clone() for p in net.parameters()]
r = mon.result()
assert r["steps"] == 4 and r["rows"] == 20 and r["nonfinite_steps"] == 0 and r["skipped_steps"] == 0 and r["last_loss"] == gl[3]
reset()
el = []
for i in range(4):
    opt.zero_grad(set_to_none=True)
    loss = lf(net, xs[i], ys[i])
    with layers.vector_backward_overlap():
        loss.backward()
    opt.step()
    el.append(float(loss.detach()))
del loss
torch.cuda.synchronize()
assert gl == el, (gl, el)
assert all(torch.equal(a, b.detach()) for a, b in zip(pg, net.parameters()))
assert torch.equal(graphed, mon._totals), (graphed.tolist(), mon._totals.tolist())
print("BCEGRAPH_OK", gl, r["accuracy"])
""", "BCEGRAPH_OK")


# ----------------------------------------------------------------------------------------------------------------- 4. the baseline
BASE_NETS = {"softmax": ((12, 16, 3), "log_softmax", 70), "sigmoid": ((8, 1), "sigmoid", 5)}


@pytest.mark.parametrize("kind", sorted(BASE_NETS))
def test_baseline_sample_elbo_with_a_monitor(bnn, dev, kind, monkeypatch):
    from bnn_amd import base, losses
    dims, head, B = BASE_NETS[kind]
    sig = head == "sigmoid"
    torch.manual_seed(0)
    net = base.BayesianNetwork(dims, head=head).to(dev).train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, dims[0], generator=g).to(dev)
    y = ((torch.rand(B, 1, generator=g) > 0.5).float() if sig else torch.randint(0, dims[-1], (B,), generator=g)).to(dev)
    seen = []
    name = "elbo_bce_loss" if sig else "elbo_loss"
    real = getattr(losses, name)

    def spy(out, target, kl=None, num_batches=1.0, **kw):
        seen.append((out.detach().clone(), target.detach().clone(), None if kl is None else kl.detach().clone(), num_batches,
                     kw.get("monitor")))
        return real(out, target, kl, num_batches, **kw)

    monkeypatch.setattr(losses, name, spy)
    mon = bnn.TrainMonitor(dims[-1], dev)
    runs = []
    for monitor in (None, mon):
        bnn.manual_seed(21)
        net.zero_grad(set_to_none=True)
        res = net.sample_elbo(x, y, draws="hip", num_batches=N_BATCHES, monitor=monitor)
        assert len(res) == (5 if sig else 4)
        res[0].backward()
        runs.append(([t.detach().clone() for t in res], {k: p.grad.clone() for k, p in net.named_parameters()}))
        del res
    (plain, gp), (fused, gf) = runs
    # one loss launch per step; the monitored one carries the whole ELBO
    assert len(seen) == 2 and seen[0][2] is None and seen[0][4] is None and seen[1][4] is mon and seen[1][3] == N_BATCHES
    assert _same(plain[1], fused[1]) and _same(plain[2], fused[2])                       # log_prior, log_q
    assert _same(seen[0][0], seen[1][0])                                                 # the loss received the same head output
    assert _same(seen[1][2].reshape(()), (fused[2] - fused[1]).reshape(()))
    kl_term = float(plain[2] - plain[1]) / N_BATCHES
    bound = FUSED * (abs(float(plain[3])) + abs(kl_term))
    print("%s loss fused %.9g unfused %.9g |diff| %.3g bound %.3g" % (kind, float(fused[0]), float(plain[0]),
                                                                         abs(float(fused[0]) - float(plain[0])), bound))
    assert abs(float(fused[0]) - float(plain[0])) <= bound
    assert abs(float(fused[3]) - float(plain[3])) <= 2 * bound                           # the printed nll: loss - kl_term
    if sig:
        assert _same(plain[4], fused[4])
    worst = 0.0
    assert gp.keys() == gf.keys() and len(gp) > 0
    for k in gp:
        d, lim = (gf[k] - gp[k]).abs(), FUSED * gp[k].abs()
        worst = max(worst, float((d / lim.clamp_min(1e-45)).max()))
        assert bool((d <= lim).all()), (k, float(d.max()))
        assert bool(torch.isfinite(gf[k]).all()), k
    print("%s gradients: worst |diff| / bound %.3g" % (kind, worst))
    r = mon.result()
    assert r["last_loss"] == float(fused[0])
    out, tgt, kl, _, _ = seen[1]
    if sig:
        s = bref.step(out.cpu().numpy(), tgt.cpu().numpy().reshape(out.shape), float(kl), 1.0 / N_BATCHES,
                      terms=_kernel_terms(out, tgt.reshape(out.shape)))
    else:
        s = cref.step(out.cpu().numpy(), tgt.cpu().numpy(), float(kl), 1.0 / N_BATCHES)
    want = cref.totals([s])
    assert (r["steps"], r["rows"], r["correct"]) == (1, B * (dims[-1] if sig else 1), want["correct"])
    for k in cref.COUNT_NAMES:
        assert r[k] == want[k], (k, r[k], want[k])
    # draws="torch" takes the same fused tail (its draws are torch.distributions': only the structure is compared)
    net.zero_grad(set_to_none=True)
    res = net.sample_elbo(x, y, num_batches=N_BATCHES, monitor=mon)
    assert len(seen) == 3 and seen[2][4] is mon and mon.result()["steps"] == 2
    assert mon.result()["last_loss"] == float(res[0].detach())


def test_baseline_graphed_step_with_an_invalid_prior_parameter_subprocess():
    """base (12, 16, 3), B = 70, optim.SGD behind the monitor's guard, sample_elbo(draws="hip", monitor=mon) in one captured
    step.  Two clean replays train.  Then pa = -1 on the first layer (an invalid Beta parameter that torch.distributions'
    argument checks would have refused): lgamma(-1) is inf, so the layer's log_prior is not finite.  Whatever the loss comes out
    as, finite <=> the step was applied: a non-finite loss is counted once as non-finite and once as skipped and changes no
    parameter."""
    _run_child(r"""
import sys, math, torch
sys.path.insert(0, @ROOT@)
import bnn_amd
from bnn_amd import base
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = base.BayesianNetwork((12, 16, 3)).to(dev).train()
mon = bnn_amd.TrainMonitor(3, dev)
opt = bnn_amd.optim.SGD(net.parameters(), lr=1e-3)
opt.set_guard(mon)
g = torch.Generator().manual_seed(1)
x = torch.randn(70, 12, generator=g).to(dev); y = torch.randint(0, 3, (70,), generator=g).to(dev)
lf = lambda n, a, b: n.sample_elbo(a, b, draws="hip", num_batches=5, monitor=mon)[0]
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)
mon.reset()
bnn_amd.manual_seed(7)
params = lambda: [p.detach().clone() for p in net.parameters()]
same = lambda a, b: all(torch.equal(u, v) for u, v in zip(a, b))
p0 = params()
l0 = [float(step(x, y)) for _ in range(2)]
r = mon.result()
assert all(math.isfinite(v) for v in l0) and not same(p0, params())
assert (r["steps"], r["rows"], r["nonfinite_steps"], r["skipped_steps"]) == (2, 140, 0, 0) and r["last_loss"] == l0[1]
with torch.no_grad():
    net.l1.pa.fill_(-1.0)
p2 = params()
lb = float(step(x, y))
r = mon.result()
print("loss with pa = -1:", lb, {k: r[k] for k in ("steps", "nonfinite_steps", "skipped_steps")})
assert r["steps"] == 3 and (r["last_loss"] == lb or (lb != lb and r["last_loss"] != r["last_loss"]))
assert math.isfinite(r["last_loss"]) == (r["skipped_steps"] == 0)
if math.isfinite(lb):
    assert r["nonfinite_steps"] == 0 and not same(p2, params()) and int(mon._guard) == 0
else:
    assert r["nonfinite_steps"] == 1 and r["skipped_steps"] == 1 and same(p2, params()) and int(mon._guard) == 1
print("BASEGRAPH_OK", l0, lb)
""", "BASEGRAPH_OK")


# ----------------------------------------------------------------------------------------------------------------------- 5. VD
def test_vd_loss_fn_with_a_monitor(bnn, dev):
    from bnn_amd import vd
    torch.manual_seed(0)
    model = vd.BNN((8, 6, 3)).to(dev)
    g = torch.Generator().manual_seed(4)
    x = torch.rand(5, 8, generator=g).to(dev)
    t = torch.randint(0, 3, (5,), generator=g).to(dev)
    mon = bnn.TrainMonitor(3, dev)
    pred = model(x)
    kl = vd.kl(model)
    assert kl.dim() == 0 and kl.dtype == torch.float32 and kl.device == pred.device
    model.eval()
    plain = vd.loss_fn(pred, t, model, num_batches=N_BATCHES)
    model.eval()
    fused = vd.loss_fn(pred, t, model, num_batches=N_BATCHES, monitor=mon)
    assert model.training                                                        # the side effect of :91 is kept
    s = cref.step(pred.detach().cpu().numpy(), t.cpu().numpy(), float(kl), 1.0 / N_BATCHES)
    bound = FUSED * (abs(s["nll"]) + abs(s["kl_term"]))
    print("vd loss fused %.9g unfused %.9g bound %.3g" % (float(fused), float(plain), bound))
    assert abs(float(fused) - float(plain)) <= bound
    r, want = mon.result(), cref.totals([s])
    for k in cref.COUNT_NAMES:
        assert r[k] == want[k], (k, r[k], want[k])
    for k in cref.SUM_NAMES:
        assert abs(r[k] - want[k]) <= 7 * EPS64 * want[k + "_abs"], k
    # (the reference's fp32 loss is rounded from a float64 sum in numpy's order: the two may round one fp32 step apart)
    assert r["last_loss"] == float(fused) and abs(r["last_loss"] - s["loss"]) <= 2.0 ** -24 * abs(s["loss"])
    fused.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
