"""GPU tier of the identity head and the fused Gaussian ELBO loss: the three kernels of csrc/gaussian_head.hip against the float64
restatement tests/gaussian_ref.py, the monitor and the guard behind them, the same step inside one captured graph, and the
identity head through every layer that has a sigmoid head -- held bit for bit against the sigmoid twin, whose probabilities are
lbbnn_binary_head of the very logits the identity head returns.

BARS (float64 of the same expression on the same float32 inputs; ulp = 2^-24 = 6e-8 relative).  A term 0.5 ((L + lv) + q) with
q = (d d) iv can cancel, so its errors are stated against S = |L| + |lv| + q (tests/gaussian_ref.py: magnitude = S / 2):
  * d = y - m 0.5 ulp, d d 1.5, iv = expf(-lv) <= 2 (the argument is exact), q <= 4 ulp of q; L + lv: the rounding of L and of
    the sum, <= 1 ulp of |L| + |lv|; the outer sum 0.5 ulp: under 5.5 ulp of S = 3.3e-7 S.  Bar per term 1e-6 * S / 2 (a factor
    3 for the device's expf); the loss, summed in fp64 and rounded once to fp32 (6e-8 |loss|): 1e-6 * (sum S / 2 + |kl term|);
  * g_mean = (g (m - y)) iv: 0.5 + 0.5 + 2 + 0.5 = 3.5 ulp, bar 1e-6 relative (+ 1e-30);
  * g_lv = (g 0.5) (1 - q): q's 4 ulp and the difference's 0.5, against |g| 0.5 (1 + q): bar 1e-6 of that (summed over the
    batch for a shared log_var, whose fp64 column sum is rounded once more);
  * g_kl = g * kl_scale is one fp32 product: exact.
Everything that is plumbing (the monitor's shared pass, the captured step, the head inside the network) is held bit for bit;
fp64 totals against the fp64 sum of the kernel's own fp32 terms within gaussian_ref.DBL * sum |term|."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gaussian_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BATCHES = 5.0
G_ROOT = 1.75                         # d(total) / d(loss): the loss is scaled before backward so that g is not 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _same(a, b):
    """Bit for bit (a NaN equal to a NaN of the same bits)."""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ 1. the loss kernels
# one element; a few units; all 16 units (T = 1024 threads); T = 1020 threads, more than one round; past the 1024-thread stride
LOSS_SHAPES = ((1, 1), (5, 3), (64, 16), (257, 5), (1030, 1))


def _case(B, O, per_element, seed):
    """CPU float32 (mean, target, log_var): targets about 1.3 standard deviations from the mean; with more than 8 elements a NaN,
    a +inf and a -inf target."""
    g = torch.Generator().manual_seed(seed)
    m = 2.0 * torch.randn(B, O, generator=g)
    lv = 0.7 * torch.randn((B, O) if per_element else (O,), generator=g)
    y = m + 1.3 * torch.randn(B, O, generator=g) * torch.exp(0.5 * lv)
    if B * O > 8:
        flat = y.view(-1)
        flat[3], flat[B * O // 2], flat[B * O - 2] = float("nan"), float("inf"), float("-inf")
    return m, y, lv


def _leaves(m, lv, sliced, dev):
    """Device leaves and the (mean, log_var) the loss reads: contiguous tensors, or column slices of ONE wider NaN-padded leaf
    (mean | 2 NaN columns | log_var | 1 NaN column; a shared log_var stays a leaf of its own)."""
    B, O = m.shape
    if not sliced:
        a, b = m.clone().to(dev).requires_grad_(True), lv.clone().to(dev).requires_grad_(True)
        return [a, b], a, b
    per_element = lv.dim() == 2
    w = torch.full((B, 2 * O + 3), float("nan"))
    w[:, :O] = m
    if per_element:
        w[:, O + 2:2 * O + 2] = lv
    w = w.to(dev).requires_grad_(True)
    b = w[:, O + 2:2 * O + 2] if per_element else lv.clone().to(dev).requires_grad_(True)
    return [w] if per_element else [w, b], w[:, :O], b


def _kernel_terms(mean, y, lv):
    """The (B, O) fp32 terms as the loss kernel itself forms them: lbbnn_elbo_gaussian_loss on each element alone (B = O = 1, no kl:
    *loss is (float)(double)term, the term).  Bad targets give 0."""
    from bnn_amd import _lib
    B, O = mean.shape
    t = torch.zeros(B * O, dtype=torch.float32, device=mean.device)
    f, stream = _lib.lib().lbbnn_elbo_gaussian_loss, torch.cuda.current_stream(mean.device).cuda_stream
    zero = ctypes.c_float(0.0)
    for b in range(B):
        for o in range(O):
            pl = lv.data_ptr() + 4 * ((b * lv.stride(0) + o * lv.stride(1)) if lv.dim() == 2 else o)
            rc = f(mean.data_ptr() + 4 * (b * mean.stride(0) + o * mean.stride(1)), 1, y.data_ptr() + 4 * (b * O + o), 1, pl, 0, 1, 1,
                   None, zero, t.data_ptr() + 4 * (b * O + o), None, None, stream)
            assert rc == 0
    return t.cpu().numpy().astype(np.float64).reshape(B, O)


@pytest.mark.parametrize("per_element", (False, True), ids=("shared", "element"))
@pytest.mark.parametrize("sliced", (False, True), ids=("dense", "slice"))
@pytest.mark.parametrize("B,O", LOSS_SHAPES)
def test_loss_gradients_stats_and_totals(bnn, dev, B, O, sliced, per_element):
    m, y, lv = _case(B, O, per_element, 100 * B + O)
    yd = y.to(dev)
    klv, scale = 12.5, 1.0 / N_BATCHES
    mons = [bnn.TrainMonitor(O, dev), bnn.TrainMonitor(O, dev)]
    st = [torch.zeros(4, dtype=torch.float64, device=dev) for _ in range(2)]
    got = []
    for k, mon in enumerate((None, mons[0])):
        leaves, mean, log_var = _leaves(m, lv, sliced, dev)
        kl = torch.tensor(klv, device=dev, requires_grad=True)
        loss = bnn.elbo_gaussian_loss(mean, yd, log_var, kl, N_BATCHES, stats=st[k], monitor=mon)
        (loss * G_ROOT).backward()
        got.append([loss.detach().clone(), kl.grad.clone()] + [l.grad.clone() for l in leaves])
    # ---- monitored against plain: the same bits
    assert len(got[0]) == len(got[1]) and all(_same(a, b) for a, b in zip(got[0], got[1]))
    assert torch.equal(st[0], st[1])
    # ---- against float64
    n_bad = 3 if B * O > 8 else 0
    mag = ref.magnitude(m, y, lv)
    want = ref.loss(m, y, lv, klv, scale)
    bar = 1e-6 * (float(mag.sum()) + abs(klv * scale))
    err = abs(float(got[0][0]) - want)
    print("gaussian loss B=%d O=%d: loss %.9g ref %.17g |diff| / bar %.3g" % (B, O, float(got[0][0]), want, err / bar))
    assert err <= bar
    g = float(np.float32(G_ROOT))
    gm64, glv64, _ = ref.grads(g, m, y, lv, scale)
    assert float(got[0][1]) == float(np.float32(G_ROOT) * np.float32(scale))                      # g_kl: one fp32 product
    leaf0 = got[0][2].cpu().numpy().astype(np.float64)
    g_mean = leaf0[:, :O]
    e_mean = float((np.abs(g_mean - gm64) / (1e-6 * np.abs(gm64) + 1e-30)).max())
    if per_element:
        g_lv = leaf0[:, O + 2:2 * O + 2] if sliced else got[0][3].cpu().numpy().astype(np.float64)
    else:
        g_lv = got[0][3].cpu().numpy().astype(np.float64)
    e_lv = float((np.abs(g_lv - glv64) / (1e-6 * ref.grad_lv_magnitude(g, m, y, lv) + 1e-30)).max())
    print("gaussian loss B=%d O=%d: worst |g_mean - ref| / bar %.3g, |g_lv - ref| / bar %.3g" % (B, O, e_mean, e_lv))
    assert e_mean <= 1.0 and e_lv <= 1.0
    if sliced:                                                     # the padding of the wide leaf: read by nothing, gradient 0
        pad = np.ones(leaf0.shape[1], bool)
        pad[:O] = False
        if per_element:
            pad[O + 2:2 * O + 2] = False
        assert not leaf0[:, pad].any()
    bad = ~np.isfinite(y.numpy())
    assert int(bad.sum()) == n_bad and not g_mean[bad].any() and (not per_element or not g_lv[bad].any())
    # ---- stats and totals: exact counts, fp64 sums of the kernel's own fp32 values
    leaves, mean, log_var = _leaves(m, lv, sliced, dev)
    with torch.no_grad():
        terms = _kernel_terms(mean, yd, log_var)
        e_term = float((np.abs(terms - ref.terms(m, y, lv)) / (1e-6 * mag + 1e-30)).max())
        print("gaussian loss B=%d O=%d: worst |term - ref| / bar %.3g" % (B, O, e_term))
        assert e_term <= 1.0
        bnn.elbo_gaussian_loss(mean, yd, log_var, torch.tensor(klv, device=dev), N_BATCHES, monitor=mons[1])
        bnn.elbo_gaussian_loss(mean, yd, log_var, torch.tensor(klv, device=dev), N_BATCHES, monitor=mons[1])
        bnn.elbo_gaussian_loss(mean, yd, log_var, torch.tensor(klv, device=dev), N_BATCHES, monitor=mons[0])
    assert torch.equal(mons[0]._totals, mons[1]._totals) and torch.equal(mons[0]._guard, mons[1]._guard)     # two identical passes
    d32 = np.where(bad, np.float32(0), (y.numpy() - m.numpy()).astype(np.float32))
    se, ae = (d32 * d32).astype(np.float32).astype(np.float64), np.abs(d32).astype(np.float64)
    s = st[1].cpu().numpy()
    assert abs(s[0] - se.sum()) <= ref.DBL * se.sum() and abs(s[1] - ae.sum()) <= ref.DBL * ae.sum()
    assert s[2] == B * O - n_bad and s[3] == n_bad
    r = mons[0].result(strict=False)
    c = ref.counts(m, y, lv)
    kl_term = float(np.float32(klv)) * float(np.float32(scale))
    assert (r["steps"], r["rows"], r["bad_targets"], r["nonfinite_rows"], r["nonfinite_steps"], r["nll_rows"]) == \
        (2, 2 * c["rows"], 2 * n_bad, 0, 0, 2 * (c["rows"] - n_bad))
    assert r["correct"] == 2 * c["correct"], (r["correct"], c["correct"])
    nll, a_nll = float(terms.sum()), float(np.abs(terms).sum())
    print("gaussian loss B=%d O=%d: nll_sum %.17g ref %.17g coverage %.3f" % (B, O, r["nll_sum"], 2 * nll, r["accuracy"]))
    assert abs(r["nll_sum"] - 2 * nll) <= ref.DBL * 2 * a_nll and abs(r["last_nll"] - nll) <= ref.DBL * a_nll
    assert abs(r["kl_term_sum"] - 2 * kl_term) <= ref.DBL * 2 * kl_term
    assert abs(r["loss_sum"] - 2 * (nll + kl_term)) <= ref.DBL * 2 * (a_nll + kl_term)
    assert r["last_loss"] == float(got[1][0]) and int(mons[0]._guard) == 0
    if n_bad:
        with pytest.raises(IndexError):
            mons[0].result()


def test_an_infinite_mean_raises_the_guard_and_the_optimizer_skips(bnn, dev):
    """One +inf element of the mean: the loss is not finite, the guard word is 1, the step is counted and the guarded Adam step
    changes no parameter, moment or step counter; the next clean step updates."""
    torch.manual_seed(0)
    net = bnn.lrt.BayesianNetwork((8, 1), head="identity").to(dev).train()
    log_var = torch.nn.Parameter(torch.zeros(1, device=dev))
    ps = list(net.parameters()) + [log_var]
    opt = bnn.optim.Adam([{"params": list(net.parameters())}, {"params": [log_var], "lr": 5e-2}], lr=1e-2)
    mon = bnn.TrainMonitor(1, dev)
    opt.set_guard(mon)
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(5, 8, generator=g).to(dev), torch.randn(5, 1, generator=g).to(dev)
    bump = torch.zeros(5, 1, device=dev)
    bump[2, 0] = float("inf")
    bnn.manual_seed(3)

    def state():
        out = [p.detach().clone() for p in ps]
        for p in ps:
            out += [v.clone() for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
        return out + [opt._tables()["steps"].clone()]

    def step(poison):
        opt.zero_grad(set_to_none=True)
        out = net(x, sample=True)
        loss = bnn.elbo_gaussian_loss(out + bump if poison else out, y, log_var, net.kl(), N_BATCHES, monitor=mon)
        loss.backward()
        opt.step()
        return float(loss.detach())

    same = lambda a, b: len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    assert math.isfinite(step(False))
    s1 = state()
    assert not math.isfinite(step(True))
    assert same(state(), s1)
    r = mon.result()
    assert (r["steps"], r["nonfinite_steps"], r["nonfinite_rows"], r["skipped_steps"], int(mon._guard)) == (2, 1, 1, 1, 1)
    assert r["nll_rows"] == 5                                       # the finite step's elements only
    assert math.isfinite(step(False))
    s3 = state()
    assert not torch.equal(s1[len(ps) - 1], s3[len(ps) - 1]) and not torch.equal(s1[0], s3[0])       # log_var and a weight moved
    r = mon.result()
    assert (r["steps"], r["nonfinite_steps"], r["skipped_steps"], int(mon._guard)) == (3, 1, 1, 0)
    assert all(bool(torch.isfinite(t).all()) for t in s3)


def test_nonfinite_log_var_and_empty_batch(bnn, dev):
    m, y = torch.zeros(4, 2, device=dev), torch.ones(4, 2, device=dev)
    mon = bnn.TrainMonitor(2, dev)
    lv = torch.tensor([0.0, float("nan")], device=dev)
    assert math.isnan(float(bnn.elbo_gaussian_loss(m, y, lv, monitor=mon)))
    r = mon.result()
    assert (r["nonfinite_rows"], r["nonfinite_steps"], int(mon._guard)) == (4, 1, 1)
    kl = torch.tensor(2.5, device=dev)
    empty = bnn.elbo_gaussian_loss(m[:0], y[:0], lv, kl, 5.0)                   # an empty batch: the kl term alone
    assert float(empty) == 0.5
    with pytest.raises(ValueError, match="16"):
        bnn.elbo_gaussian_loss(torch.zeros(2, 17, device=dev), torch.zeros(2, 17, device=dev), torch.zeros(17, device=dev))


# ------------------------------------------------------------------------------------------------------------------- 2. the graph
def _run_child(code, token):
    code = code.replace("@ROOT@", repr(ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and token in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])


def test_monitored_gaussian_step_under_a_graph_subprocess():
    """lrt (8, 1) with an identity head, B = 5, a learnable log_var in its own Adam group behind the monitor's guard,
    elbo_gaussian_loss(stats=, monitor=) in one captured step: after a reset, four replays leave bitwise the losses, parameters,
    stats and totals of four eager steps from the same parameters and Philox state."""
    _run_child(r"""
import sys, copy, torch
sys.path.insert(0, @ROOT@)
import bnn_amd
from bnn_amd import layers
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.lrt.BayesianNetwork((8, 1), head="identity").to(dev).train()
log_var = torch.nn.Parameter(torch.zeros(1, device=dev))
init = copy.deepcopy(net.state_dict())
mon = bnn_amd.TrainMonitor(1, dev)
stats = torch.zeros(4, dtype=torch.float64, device=dev)
opt = bnn_amd.optim.Adam([{"params": list(net.parameters())}, {"params": [log_var], "lr": 5e-2}], lr=1e-2)
opt.set_guard(mon)
g = torch.Generator().manual_seed(1)
xs = [torch.randn(5, 8, generator=g).to(dev) for _ in range(4)]
ys = [torch.randn(5, 1, generator=g).to(dev) for _ in range(4)]
lf = lambda n, a, b: bnn_amd.elbo_gaussian_loss(n(a, sample=True), b, log_var, n.kl(), 5, stats=stats, monitor=mon)
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, xs[0], ys[0])
assert mon.result()["steps"] == 3                      # the factory's eager warm-up steps are real steps

def reset():
    net.load_state_dict(init)
    with torch.no_grad():
        log_var.zero_()
    for s in opt.state.values():
        s["exp_avg"].zero_(); s["exp_avg_sq"].zero_()
    for gr in opt.param_groups:
        gr["step_dev"].zero_()
    bnn_amd.manual_seed(7)
    mon.reset()
    stats.zero_()

reset()
gl = [float(step(xs[i], ys[i])) for i in range(4)]
graphed, gstats = mon._totals.clone(), stats.clone()
pg = [p.detach().clone() for p in list(net.parameters()) + [log_var]]
r = mon.result()
assert r["steps"] == 4 and r["rows"] == 20 and r["nonfinite_steps"] == 0 and r["skipped_steps"] == 0 and r["last_loss"] == gl[3]
assert float(log_var) != 0.0 and float(gstats[2]) == 20.0
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
assert all(torch.equal(a, b.detach()) for a, b in zip(pg, list(net.parameters()) + [log_var]))
assert torch.equal(graphed, mon._totals), (graphed.tolist(), mon._totals.tolist())
assert torch.equal(gstats, stats)
print("GAUSSGRAPH_OK", gl, r["accuracy"], float(log_var))
""", "GAUSSGRAPH_OK")


# -------------------------------------------------------------------------------------------------------------------- 3. the head
def _twins(bnn, kind, dev):
    """(identity network, sigmoid twin): the same seeded parameters."""
    out = []
    for head in ("identity", "sigmoid"):
        torch.manual_seed(11)
        if kind == "lrt1":
            net = bnn.lrt.BayesianNetwork((20, 1), head=head)
        elif kind == "lrt3":
            net = bnn.lrt.BayesianNetwork((12, 8, 3), head=head)
        elif kind == "mnf3":
            net = bnn.mnf.BayesianNetwork((12, 8, 3), 2, z_flow_type="Planar", r_flow_type="Planar", head=head)
        else:
            net = bnn.mnf.BayesianNetwork((12, 8, 3), 2, head=head)                # RNVP z flows
        out.append(net.to(dev))
    a, b = out[0].state_dict(), out[1].state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    return out


def _head_of_raw(bnn, raw):
    """lbbnn_binary_head of raw outputs of any shape (.., O): the sigmoid head's own elementwise launch."""
    flat = raw.detach().reshape(-1, raw.shape[-1]).contiguous()
    return bnn.ops.binary_head(flat).reshape(raw.shape)


def _both(bnn, nets, dev, fn, seed=5):
    """fn(net) on the identity network and on its sigmoid twin from the same Philox offset: (raw, probs, offsets equal)."""
    res, rng = [], []
    for net in nets:
        bnn.manual_seed(seed)
        res.append(fn(net))
        rng.append(bnn.ops.RngState.get(dev).t.clone())
    return res[0], res[1], torch.equal(rng[0], rng[1])


@pytest.mark.parametrize("kind", ("lrt1", "lrt3", "mnf3"))
def test_identity_head_is_the_sigmoid_head_minus_its_launch(bnn, dev, kind):
    ev = bnn.evaluate
    nets = _twins(bnn, kind, dev)
    I, O = nets[0].dims[0], nets[0].dims[-1]
    x = torch.randn(7, I, generator=torch.Generator().manual_seed(2)).to(dev)
    S = 3

    def check(fn, what, shape):
        raw, probs, same_rng = _both(bnn, nets, dev, fn)
        assert tuple(raw.shape) == shape and tuple(probs.shape) == shape, (what, raw.shape, probs.shape)
        assert _same(_head_of_raw(bnn, raw), probs), what
        assert same_rng, what                                          # the head draws nothing: the same Philox offsets

    for net in nets:
        net.train()
    check(lambda n: n(x, sample=True), "autograd forward", (7, O))
    with torch.no_grad():
        check(lambda n: n(x, sample=True).clone(), "no-grad forward (train)", (7, O))
        for net in nets:
            net.eval()
        check(lambda n: n(x, sample=True).clone(), "no-grad forward (eval, sample)", (7, O))
        check(lambda n: n(x, sample=False).clone(), "no-grad forward (posterior mean)", (7, O))
        plans = [bnn.graphs.LaunchPlan(n, x, sample=True) for n in nets]
        assert len(plans[0]) == len(plans[1]) - 1                      # the same C calls but the head's launch
        raw, probs, same_rng = _both(bnn, plans, dev, lambda p: p()[0].clone())
        assert _same(_head_of_raw(bnn, raw), probs) and same_rng
        check(lambda n: ev.ensemble_forward(n, x, S, batched=False), "ensemble loop", (S, 7, O))
        check(lambda n: ev.ensemble_forward(n, x, S, batched=True), "ensemble batched", (S, 7, O))
        for gates, kw in (("alpha", {}), ("mpm", {}), ("mpm", dict(compact=True))):
            fzs = [ev.freeze(n, gates, **kw) for n in nets]
            assert fzs[0].head == "identity" and fzs[1].head == "sigmoid"
            for what, fn in (("ensemble", lambda f: f.ensemble(x, S)), ("members", lambda f: f.ensemble(x, S, max_members=2)),
                             ("ensemble_forward", lambda f: ev.ensemble_forward(f, x, S))):
                raw, probs, same_rng = _both(bnn, fzs, dev, fn)
                assert tuple(raw.shape) == (S, 7, O) and _same(_head_of_raw(bnn, raw), probs) and same_rng, (gates, kw, what)
            raw, probs, same_rng = _both(bnn, fzs, dev, lambda f: f(x, sample=False).clone())
            assert tuple(raw.shape) == (7, O) and _same(_head_of_raw(bnn, raw), probs) and same_rng, (gates, kw)
            if not kw:
                for f in fzs:
                    f.refresh()
                raw, probs, same_rng = _both(bnn, fzs, dev, lambda f: f.ensemble(x, S))
                assert _same(_head_of_raw(bnn, raw), probs) and same_rng, (gates, "refresh")


def test_identity_head_on_a_dense_frozen_rnvp_network(bnn, dev):
    ev = bnn.evaluate
    nets = _twins(bnn, "rnvp", dev)
    x = torch.randn(7, 12, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        fzs = [ev.freeze(n, "alpha", dense=True) for n in nets]
        raw, probs, same_rng = _both(bnn, fzs, dev, lambda f: f.ensemble(x, 3))
        assert tuple(raw.shape) == (3, 7, 3) and _same(_head_of_raw(bnn, raw), probs) and same_rng
        raw, probs, same_rng = _both(bnn, nets, dev, lambda n: ev.ensemble_forward(n, x, 3, batched=True))
        assert _same(_head_of_raw(bnn, raw), probs) and same_rng


@pytest.mark.parametrize("kind", ("lrt1", "lrt3", "mnf3"))
def test_parameter_gradients_equal_the_torch_spelling_of_the_loss(bnn, dev, kind):
    """The same forward (same Philox offset), the fused loss against its torch spelling: every parameter gradient, the gradient of
    log_var and the loss.  A gradient is J^T g_mean (+ the KL's part, the same in both); g_mean differs by the loss test's 1e-6
    per element and the two float32 backward passes round alike, so the bar is 1e-6 * (B * O) * max |gradient| per tensor -- the
    worst case of B * O perturbed summands with |J g| <= max |gradient|."""
    net = _twins(bnn, kind, dev)[0].train()
    I, O = net.dims[0], net.dims[-1]
    B = 5
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(B, I, generator=g).to(dev), torch.randn(B, O, generator=g).to(dev)
    y[1, 0] = float("nan")
    res = []
    for fused in (True, False):
        log_var = (0.3 * torch.arange(O, dtype=torch.float32, device=dev) - 0.2).requires_grad_(True)
        net.zero_grad(set_to_none=True)
        bnn.manual_seed(9)
        out = net(x, sample=True)
        kl = net.kl()
        if fused:
            loss = bnn.elbo_gaussian_loss(out, y, log_var, kl, N_BATCHES)
        else:
            ok = torch.isfinite(y)
            d = torch.where(ok, y, out.detach()) - out
            term = 0.5 * ((ref.LOG_2PI + log_var) + (d * d) * torch.exp(-log_var))
            loss = torch.where(ok, term, torch.zeros_like(term)).sum() + kl / N_BATCHES
        loss.backward()
        res.append((float(loss.detach()), [p.grad.clone() for p in net.parameters()] + [log_var.grad.clone()]))
        del loss, out, kl
    assert abs(res[0][0] - res[1][0]) <= 2e-6 * (abs(res[1][0]) + 10.0 * B * O)
    worst = 0.0
    for a, b in zip(res[0][1], res[1][1]):
        bar = 1e-6 * B * O * float(b.abs().max()) + 1e-30
        worst = max(worst, float((a - b).abs().max()) / bar)
    print("%s: worst |grad - torch spelling| / bar %.3g over %d tensors" % (kind, worst, len(res[0][1])))
    assert worst <= 1.0
