"""GPU tier of the multi-group Adam: bnn_amd.optim.Adam on lbbnn_adam_step_groups / lbbnn_grad_sumsq -- every parameter group in
one launch, learning rates read from a device table (so they change under a captured graph), gradient masks, global-norm
clipping, AdamW.  Parity bar unless a case says bitwise: the project's Adam bar, max-norm relative error below 2e-6 against
torch.optim.Adam / AdamW on the same gradients (conftest.rel_err).  Cases that capture a HIP graph run once, in a process of
their own, under a time limit."""
import copy
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-6
SHAPES = [(1,), (7,), (33, 17), (4097,), (130, 1200), (5,)]          # the awkward shapes of test_fused_adam_matches_torch_adam
RATES = [1e-4, 1e-3, 1e-5, 0.1]                                      # the reference's four rates (LBBNN-GP-MF.py:520-554)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _run(code, tag, timeout=600):
    env = dict(os.environ)
    env.pop("LBBNN_DP_FORCE_COLLECTIVE", None)
    r = subprocess.run([sys.executable, "-c", code.replace("@ROOT@", repr(ROOT))], capture_output=True, text=True, timeout=timeout,
                       env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and tag in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


def _params(dev, shapes, seed):
    g = torch.Generator().manual_seed(seed)
    base = [torch.randn(s, generator=g).to(dev) for s in shapes]
    return [torch.nn.Parameter(t.clone()) for t in base], [torch.nn.Parameter(t.clone()) for t in base]


def _set_grads(pa, pb, gs):
    for p, q, g in zip(pa, pb, gs):
        p.grad, q.grad = g.clone(), g.clone()


# ------------------------------------------------------------------------------------------------------- 1. unchanged default
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_default_optimizer_is_bitwise_lbbnn_adam_step(bnn, dev, wd):
    """One group, 5 steps, the six awkward shapes: parameters, exp_avg and exp_avg_sq of bnn_amd.optim.Adam (now on
    lbbnn_adam_step_groups) are bitwise what lbbnn_adam_step gives when driven directly on clones."""
    from bnn_amd import _lib
    torch.manual_seed(0)
    pa, _ = _params(dev, SHAPES, 1)
    ref_p = [p.detach().clone() for p in pa]
    ref_m = [torch.zeros_like(p) for p in ref_p]
    ref_v = [torch.zeros_like(p) for p in ref_p]
    ref_step = torch.zeros(1, device=dev)
    lr, betas, eps = 1e-2, (0.9, 0.99), 1e-8
    opt = bnn.optim.Adam(pa, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for it in range(5):
        gs = [torch.randn(s, device=dev) * (0.1 + it) for s in SHAPES]
        for p, g in zip(pa, gs):
            p.grad = g.clone()
        opt.step()
        lst = _lib.AdamList()
        lst.n = len(ref_p)
        for k in range(len(ref_p)):
            lst.p[k], lst.g[k], lst.m[k], lst.v[k] = ref_p[k].data_ptr(), gs[k].data_ptr(), ref_m[k].data_ptr(), ref_v[k].data_ptr()
            lst.numel[k] = ref_p[k].numel()
        rc = lib.lbbnn_adam_step(ctypes.byref(lst), lr, betas[0], betas[1], eps, wd, ref_step.data_ptr(), 1, stream)
        assert rc == 0
        torch.cuda.synchronize()
    for p, rp, rm, rv in zip(pa, ref_p, ref_m, ref_v):
        assert torch.equal(p.detach(), rp)
        assert torch.equal(opt.state[p]["exp_avg"], rm) and torch.equal(opt.state[p]["exp_avg_sq"], rv)
    assert float(opt.param_groups[0]["step_dev"]) == 5.0 == float(ref_step)


# ------------------------------------------------------------------------------------------------------------- 2. many groups
def _many_groups(params):
    """33 single-tensor groups with the reference's four rates and mixed betas / eps / weight decay, plus one group of four."""
    groups = []
    for i in range(33):
        groups.append(dict(params=[params[i]], lr=RATES[i % 4], betas=((0.9, 0.999), (0.8, 0.99), (0.95, 0.9))[i % 3],
                           eps=(1e-8, 1e-6)[i % 2], weight_decay=(0.0, 0.01, 0.1)[(i // 2) % 3]))
    groups.append(dict(params=list(params[33:]), lr=3e-3, betas=(0.85, 0.98), eps=1e-7, weight_decay=0.02))
    return groups


MANY_SHAPES = [SHAPES[i % 6] if i % 11 else (70, 300) for i in range(37)]


def test_many_groups_match_torch_adam(bnn, dev):
    torch.manual_seed(1)
    pa, pb = _params(dev, MANY_SHAPES, 2)
    oa, ob = bnn.optim.Adam(_many_groups(pa), lr=1e-4), torch.optim.Adam(_many_groups(pb), lr=1e-4)
    for it in range(5):
        _set_grads(pa, pb, [torch.randn(s, device=dev) * (0.1 + it) for s in MANY_SHAPES])
        oa.step(); ob.step()
    worst = max(rel_err(p.detach(), q.detach()) for p, q in zip(pa, pb))
    print("many groups: worst rel err %.3e" % worst)
    assert worst < BAR
    assert len(oa.param_groups) == 34 and all(float(g["step_dev"]) == 5.0 for g in oa.param_groups)
    # one counter array: the groups' counters are views of it, in order
    base = oa.param_groups[0]["step_dev"].data_ptr()
    assert all(g["step_dev"].data_ptr() == base + 4 * i for i, g in enumerate(oa.param_groups))


# ------------------------------------------------------------------------------------------------------------ 3. launch budget
def _recorded_step(opt):
    from bnn_amd import _lib
    _lib.RECORD = rec = []
    try:
        opt.step()
    finally:
        _lib.RECORD = None
    torch.cuda.synchronize()
    return [name for name, _, _ in rec]


def test_launch_budget_one_call_per_list(bnn, dev):
    """One step() of the 33 + 1 group optimizer (37 tensors: one list) is ONE lbbnn_adam_step_groups call -- one launch, the
    counters advance inside it (include/lbbnn.h) -- and no lbbnn_adam_step; with clipping one lbbnn_grad_sumsq call more (two
    launches: partials, fixed-order reduction), 3 launches per list in all.  130 tensors are ceil(130 / 64) = 3 lists.  (A step of
    the 34 groups was 34 lbbnn_adam_step calls, 68 launches, before.)"""
    from bnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lbbnn.h")).read()
    assert "Launches: exactly 1." in hdr and "Launches: 1, or 2 with finalize_count > 0." in hdr
    torch.manual_seed(2)
    for clip in (None, 1.0):
        pa, _ = _params(dev, MANY_SHAPES, 3)
        opt = bnn.optim.Adam(_many_groups(pa), lr=1e-4, max_grad_norm=clip)
        for p in pa:
            p.grad = torch.randn_like(p)
        opt.step()                                                   # state and tables exist
        names = _recorded_step(opt)
        assert names == ([] if clip is None else ["lbbnn_grad_sumsq"]) + ["lbbnn_adam_step_groups"], names
        assert all(float(g["step_dev"]) == 2.0 for g in opt.param_groups)
    many = [torch.nn.Parameter(torch.randn(3 + (i % 5), device=dev)) for i in range(130)]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in many]
    groups = lambda ps: [dict(params=ps[:100], lr=1e-2), dict(params=ps[100:], lr=1e-3)]
    opt, opt_ref = bnn.optim.Adam(groups(many), max_grad_norm=0.5), torch.optim.Adam(groups(ref))
    assert _lib.ADAM_GROUPS_MAX_TENSORS == 64
    for it in range(3):
        _set_grads(many, ref, [torch.randn_like(p) for p in many])
        torch.nn.utils.clip_grad_norm_(ref, 0.5)
        names = _recorded_step(opt)
        opt_ref.step()
        assert names == ["lbbnn_grad_sumsq"] * 3 + ["lbbnn_adam_step_groups"] * 3, names
    assert max(rel_err(p.detach(), q.detach()) for p, q in zip(many, ref)) < BAR
    assert [float(g["step_dev"]) for g in opt.param_groups] == [3.0, 3.0]


def test_step_without_gradients_only_advances_the_counters(bnn, dev):
    """No parameter has a gradient: the step is one advance-only launch (one workgroup, no tensor) -- parameters and moments stay,
    every group with parameters counts the step, as the per-group loop did."""
    from bnn_amd import _lib
    pa, _ = _params(dev, SHAPES[:4], 12)
    opt = bnn.optim.Adam([dict(params=pa[:2]), dict(params=pa[2:], lr=1e-2)], lr=1e-3)
    for p in pa:
        p.grad = torch.randn_like(p)
    opt.step()
    before = [p.detach().clone() for p in pa]
    m_before = [opt.state[p]["exp_avg"].clone() for p in pa]
    opt.zero_grad(set_to_none=True)
    names = _recorded_step(opt)
    assert names == ["lbbnn_adam_step_groups"]
    assert all(torch.equal(p.detach(), b) for p, b in zip(pa, before))
    assert all(torch.equal(opt.state[p]["exp_avg"], m) for p, m in zip(pa, m_before))
    assert [float(g["step_dev"]) for g in opt.param_groups] == [2.0, 2.0]
    pa[3].grad = torch.ones_like(pa[3])                              # one tensor of the second group only: both groups count
    opt.step()
    assert [float(g["step_dev"]) for g in opt.param_groups] == [3.0, 3.0]
    assert torch.equal(pa[0].detach(), before[0]) and not torch.equal(pa[3].detach(), before[3])


# -------------------------------------------------------------------------------------------------------- 4. rates under replay
def test_rates_change_under_replay_subprocess():
    """opt.step() alone captured with graphs.capture over static .grad buffers; 8 replays with fresh gradients, a StepLR schedule
    and one manual edit of one group's lr and weight_decay, push_hyperparameters() before each replay: the trajectory is
    torch.optim.Adam's with the same schedule, below 2e-6.  (Before the device table the captured rate never changed.)"""
    _run(r"""
import sys, torch
sys.path.insert(0, @ROOT@)
sys.path.insert(0, @ROOT@ + "/tests")
import bnn_amd
from conftest import rel_err
dev = torch.device("cuda:0")
torch.manual_seed(0)
shapes = [(1,), (7,), (33, 17), (4097,), (130, 1200), (5,)]
base = [torch.randn(s, device=dev) for s in shapes]
pa = [torch.nn.Parameter(t.clone()) for t in base]
pb = [torch.nn.Parameter(t.clone()) for t in base]
groups = lambda ps: [dict(params=ps[:2], lr=1e-2), dict(params=ps[2:4], lr=1e-3, weight_decay=0.0), dict(params=ps[4:], lr=0.1, betas=(0.8, 0.99))]
oa, ob = bnn_amd.optim.Adam(groups(pa), lr=1e-3), torch.optim.Adam(groups(pb), lr=1e-3)
sa = torch.optim.lr_scheduler.StepLR(oa, step_size=2, gamma=0.5)
sb = torch.optim.lr_scheduler.StepLR(ob, step_size=2, gamma=0.5)
static = [torch.zeros_like(p) for p in pa]
for p, g in zip(pa, static):
    p.grad = g
def grads(it):
    g = torch.Generator().manual_seed(100 + it)
    return [torch.randn(s, generator=g).to(dev) * (0.5 + it) for s in shapes]
def feed(it):
    for s, q, g in zip(static, pb, grads(it)):
        s.copy_(g); q.grad = g.clone()
feed(0); oa.step(); ob.step(); sa.step(); sb.step()           # eager: allocates the state outside the capture
graph = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with bnn_amd.graphs.capture(graph):
    oa.step()
pushes = 0
for it in range(1, 9):
    if it == 4:                                               # one manual edit on top of the schedule
        for o in (oa, ob):
            o.param_groups[1]["lr"] = 3e-3; o.param_groups[1]["weight_decay"] = 0.01
    feed(it)
    pushes += int(oa.push_hyperparameters())
    graph.replay()
    ob.step(); sa.step(); sb.step()
torch.cuda.synchronize()
lrs = [g["lr"] for g in oa.param_groups]
assert lrs == [g["lr"] for g in ob.param_groups] and lrs[0] < 1e-2 / 8, lrs
worst = max(rel_err(p.detach(), q.detach()) for p, q in zip(pa, pb))
print("rates under replay: worst rel err %.3e, %d pushes in 8 replays, final rates %s" % (worst, pushes, lrs))
assert worst < 2e-6, worst
assert 4 <= pushes < 8, pushes                                # copies only when a value changed
assert all(float(g["step_dev"]) == 9.0 for g in oa.param_groups)
print("REPLAY_RATES_OK")
""", "REPLAY_RATES_OK")


# ------------------------------------------------------------------------------------------------- 5. freeze through the real step
def test_freeze_groups_through_graphed_train_step_subprocess():
    """make_graphed_train_step on the baseline net (draws="hip", 784-64-48-10, B = 32), one group per tensor.  After 2 replays the
    pa / pb / weight_a / weight_b / bias_a / bias_b groups get lr = 0: after 3 more replays those tensors are bitwise unchanged
    and finite, weight_mu moved on, and the frozen groups' exp_avg kept moving (the update still ran, with rate 0)."""
    _run(r"""
import sys, torch
sys.path.insert(0, @ROOT@)
import bnn_amd
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.base.BayesianNetwork((784, 64, 48, 10)).to(dev).train()
named = list(net.named_parameters())
opt = bnn_amd.optim.Adam([dict(params=[p], lr=1e-3) for _, p in named], lr=1e-3)
g = torch.Generator().manual_seed(1)
x = torch.rand(32, 1, 28, 28, generator=g).to(dev); y = torch.randint(0, 10, (32,), generator=g).to(dev)
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lambda n, a, b: n.sample_elbo(a, b, draws="hip")[0], x, y)
for _ in range(2):
    step(x, y)
frozen_names = ("pa", "pb", "weight_a", "weight_b", "bias_a", "bias_b")
frozen = [i for i, (n, _) in enumerate(named) if n.split(".")[-1] in frozen_names]
assert len(frozen) == 18, [n for n, _ in named]
for i in frozen:
    opt.param_groups[i]["lr"] = 0.0
torch.cuda.synchronize()
snap = {n: p.detach().clone() for n, p in named}
m_snap = {i: opt.state[named[i][1]]["exp_avg"].clone() for i in frozen}
for _ in range(3):
    loss = step(x, y)
torch.cuda.synchronize()
for i in frozen:
    n, p = named[i]
    assert torch.equal(p.detach(), snap[n]) and torch.isfinite(p).all(), n
    assert not torch.equal(opt.state[p]["exp_avg"], m_snap[i]), n
moved = [n for n, p in named if n.endswith("weight_mu") and not torch.equal(p.detach(), snap[n])]
assert len(moved) == 3, moved
assert all(float(gr["step_dev"]) == 3 + 5 for gr in opt.param_groups)          # 3 warm-up steps, 5 replays
assert torch.isfinite(loss)
print("FREEZE_OK")
""", "FREEZE_OK")


# ---------------------------------------------------------------------------------------------------------------------- 6. mask
def test_masked_elements_keep_zero_moments(bnn, dev):
    """A masked-out element with weight_decay = 0 never sees a gradient: exp_avg, exp_avg_sq stay 0 and the parameter stays."""
    torch.manual_seed(4)
    p = torch.nn.Parameter(torch.randn(130, 77, device=dev))
    q = torch.nn.Parameter(p.detach().clone())
    mask = (torch.rand(130, 77, device=dev) < 0.5).float()
    r = torch.nn.Parameter(p.detach().clone())
    oa, ob, oc = bnn.optim.Adam([p], lr=1e-2), torch.optim.Adam([q], lr=1e-2), bnn.optim.Adam([r], lr=1e-2)
    oa.set_grad_mask(p, mask)
    start = p.detach().clone()
    for it in range(3):
        g = torch.randn_like(p)
        p.grad, q.grad, r.grad = g.clone(), g * mask, g * mask
        oa.step(); ob.step(); oc.step()
    off = mask == 0
    assert off.any() and (~off).any()
    assert (oa.state[p]["exp_avg"][off] == 0).all() and (oa.state[p]["exp_avg_sq"][off] == 0).all()
    assert torch.equal(p.detach()[off], start[off]) and not torch.equal(p.detach()[~off], start[~off])
    assert torch.equal(p.detach(), r.detach())                       # bitwise this optimizer on gradients masked beforehand
    assert rel_err(p.detach(), q.detach()) < BAR                     # and torch.optim.Adam on them within the bar
    oa.set_grad_mask(p, None)                                        # removed: the whole gradient again
    p.grad = torch.ones_like(p)
    oa.step()
    assert (oa.state[p]["exp_avg"][off] != 0).all()


def test_grad_mask_equals_hook_form_subprocess():
    """COND_OPT two ways on two copies of the baseline net (784-64-48-10, B = 32, draws="hip", same Philox seed), 4 steps:
    set_grad_mask(weight_mu, lambda: l.gammas) against the example's register_hook(gr * l.gammas), each eager and captured.
    Phase "relaxed" (gamma.exact = False, the training phase before the reference's epoch-20 switch: gates are relaxed-Bernoulli
    values in (0, 1)): below 2e-6.  Phase "exact" (gamma.exact = True: hard gates in {0, 1}): bitwise."""
    _run(r"""
import sys, copy, torch
sys.path.insert(0, @ROOT@)
sys.path.insert(0, @ROOT@ + "/tests")
import bnn_amd
from conftest import rel_err
dev = torch.device("cuda:0")
torch.manual_seed(0)
proto = bnn_amd.base.BayesianNetwork((784, 64, 48, 10)).to(dev).train()
init = copy.deepcopy(proto.state_dict())
g = torch.Generator().manual_seed(1)
x = torch.rand(32, 1, 28, 28, generator=g).to(dev); y = torch.randint(0, 10, (32,), generator=g).to(dev)
lf = lambda n, a, b: n.sample_elbo(a, b, draws="hip")[0]

def run(form, mode, exact):
    net = bnn_amd.base.BayesianNetwork((784, 64, 48, 10)).to(dev).train()
    net.load_state_dict(init)
    ls = (net.l1, net.l2, net.l3)
    for l in ls:
        l.gamma.exact = exact
    opt = bnn_amd.optim.Adam([dict(params=[p], lr=1e-3) for p in net.parameters()], lr=1e-3)
    for l in ls:
        if form == "mask":
            opt.set_grad_mask(l.weight_mu, lambda l=l: l.gammas)
        else:
            l.weight_mu.register_hook(lambda gr, l=l: gr * l.gammas)
    if mode == "graph":
        step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)
        net.load_state_dict(init)                                    # the warm-up steps moved the parameters: start over
        for st in opt.state.values():
            st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
        for gr in opt.param_groups:
            gr["step_dev"].zero_()
    bnn_amd.manual_seed(11)
    for it in range(4):
        if mode == "graph":
            step(x, y)
        else:
            opt.zero_grad(set_to_none=True)
            loss = lf(net, x, y)
            loss.backward()
            opt.step()
            del loss
    torch.cuda.synchronize()
    gates = [l.gammas.detach().clone() for l in ls]
    out = {k: v.detach().clone() for k, v in net.named_parameters()}
    bnn_amd.graphs.release_module_graph_refs(net)
    return out, gates

for exact in (False, True):
    phase = "exact" if exact else "relaxed"
    res = {}
    for mode in ("graph", "eager"):       # graphs first: an eager autograd graph alive on the default stream breaks a later capture
        for form in ("mask", "hook"):
            res[(mode, form)], gates = run(form, mode, exact)
            soft = sum(int(((gt != 0) & (gt != 1)).sum()) for gt in gates)
            print("phase %s, %s %s: %d gates strictly between 0 and 1" % (phase, mode, form, soft))
            assert soft == 0 or not exact, (phase, mode, form, soft)
            assert all(0 < float(gt.mean()) < 1 for gt in gates)
    ref = res[("eager", "hook")]
    for key, val in res.items():
        worst = max(rel_err(val[k], ref[k]) for k in ref)
        same = all(torch.equal(val[k], ref[k]) for k in ref)
        print("phase %s: %s %s against eager hook: worst rel err %.3e, bitwise %s" % (phase, key[0], key[1], worst, same))
        assert worst < 2e-6, (phase, key, worst)
        if exact:
            assert same, (phase, key)
    moved = [k for k in ref if k.endswith("weight_mu") and not torch.equal(ref[k], init[k])]
    assert len(moved) == 3
print("MASK_OK")
""", "MASK_OK", timeout=900)


# ------------------------------------------------------------------------------------------------------------------ 7. clipping
CLIP_SHAPES = SHAPES + [(300, 1000)]                                 # 116 partials of 4096 elements: two rows of the column sums
CLIP_SCALES = [3e-4, 1e-3, 1e-2, 1.0, 2e-3, 0.3]                     # norms around max_grad_norm = 1 on both sides


def _clip_run(bnn, dev, seed, mask=None):
    pa, pb = _params(dev, CLIP_SHAPES, seed)
    oa = bnn.optim.Adam(pa, lr=1e-2, weight_decay=0.01, max_grad_norm=1.0)
    ob = torch.optim.Adam(pb, lr=1e-2, weight_decay=0.01)
    if mask is not None:
        oa.set_grad_mask(pa[4], mask)
    gen = torch.Generator().manual_seed(seed + 1)
    norms, refs, exact = [], [], []
    for it in range(6):
        gs = [torch.randn(s, generator=gen).to(dev) * CLIP_SCALES[it] for s in CLIP_SHAPES]
        _set_grads(pa, pb, gs)
        if mask is not None:
            pb[4].grad.mul_(mask)
        exact.append(float(torch.sqrt(sum(q.grad.double().pow(2).sum() for q in pb))))
        refs.append(float(torch.nn.utils.clip_grad_norm_(pb, 1.0)))
        oa.step(); ob.step()
        norms.append(oa.grad_norm.clone())
        assert torch.equal(pa[0].grad, gs[0])                        # .grad is not rescaled (unlike clip_grad_norm_)
    torch.cuda.synchronize()
    return pa, pb, norms, refs, exact


def test_clipping_matches_clip_grad_norm_then_adam(bnn, dev):
    pa, pb, norms, refs, exact = _clip_run(bnn, dev, 5)
    # the reference's own norms decide whether the case shows anything: clipped on >= 2 steps, untouched on >= 2
    assert sum(r > 1.0 for r in refs) >= 2 and sum(r < 1.0 for r in refs) >= 2, refs
    worst = max(rel_err(p.detach(), q.detach()) for p, q in zip(pa, pb))
    nerr = [abs(float(n) - e) / e for n, e in zip(norms, exact)]
    print("clipping: reference norms %s, worst parameter rel err %.3e, grad_norm rel err against fp64 %s"
          % (["%.4g" % r for r in refs], worst, ["%.2e" % e for e in nerr]))
    assert worst < BAR
    assert max(nerr) < BAR
    # the same state and gradients again: bitwise the same norms and parameters (fixed-order sums, no atomics)
    pa2, _, norms2, _, _ = _clip_run(bnn, dev, 5)
    assert all(torch.equal(a, b) for a, b in zip(norms, norms2))
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(pa, pa2))


def test_clipping_norm_is_that_of_the_masked_gradients(bnn, dev):
    mask = (torch.rand(130, 1200, generator=torch.Generator().manual_seed(9)) < 0.3).float().to(dev)
    pa, pb, norms, refs, exact = _clip_run(bnn, dev, 6, mask=mask)
    _, _, _, _, unmasked = _clip_run(bnn, dev, 6)
    assert sum(r > 1.0 for r in refs) >= 2 and sum(r < 1.0 for r in refs) >= 2, refs
    assert all(abs(e - u) / u > 0.05 for e, u in zip(exact, unmasked))          # the mask changes the norm visibly
    assert max(abs(float(n) - e) / e for n, e in zip(norms, exact)) < BAR
    assert max(rel_err(p.detach(), q.detach()) for p, q in zip(pa, pb)) < BAR


def test_clipping_propagates_nan_like_clip_grad_norm(bnn, dev):
    p = torch.nn.Parameter(torch.ones(10, device=dev))
    opt = bnn.optim.Adam([p], lr=1e-2, max_grad_norm=1.0)
    p.grad = torch.full((10,), float("nan"), device=dev)
    opt.step()
    assert torch.isnan(opt.grad_norm).all() and torch.isnan(p).all()


# --------------------------------------------------------------------------------------------------------------------- 8. AdamW
def test_decoupled_weight_decay_matches_torch_adamw(bnn, dev):
    torch.manual_seed(7)
    pa, pb = _params(dev, SHAPES, 8)
    groups = lambda ps: [dict(params=ps[:3], lr=1e-2, weight_decay=0.05), dict(params=ps[3:], lr=3e-3, weight_decay=0.2)]
    oa = bnn.optim.Adam(groups(pa), betas=(0.9, 0.99), decoupled_weight_decay=True)
    ob = torch.optim.AdamW(groups(pb), betas=(0.9, 0.99))
    plain = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oc = bnn.optim.Adam(groups(plain), betas=(0.9, 0.99))
    for it in range(5):
        gs = [torch.randn(s, device=dev) * (0.1 + it) for s in SHAPES]
        _set_grads(pa, pb, gs)
        for p, g in zip(plain, gs):
            p.grad = g.clone()
        oa.step(); ob.step(); oc.step()
    worst = max(rel_err(p.detach(), q.detach()) for p, q in zip(pa, pb))
    print("AdamW: worst rel err %.3e" % worst)
    assert worst < BAR
    assert max(rel_err(p.detach(), q.detach()) for p, q in zip(plain, pb)) > 1e-4      # coupled decay is another trajectory


# ---------------------------------------------------------------------------------------------------------------- 9. checkpoint
def test_checkpoint_with_groups_at_different_step_counts(bnn, dev):
    """add_param_group after 2 steps (the tables regrow, the first group's counter carries over), 2 more steps, state_dict() ->
    fresh bnn_amd.optim.Adam and fresh torch.optim.Adam -> 2 more steps: all trajectories agree with a torch.optim.Adam that
    never stopped; the state_dict carries torch's per-parameter ``step`` (4 and 2) and no device counter."""
    torch.manual_seed(9)
    shapes = [(37, 5), (11,), (4097,), (3,)]
    pa, pb = _params(dev, shapes, 10)
    gs = [[torch.randn(s, device=dev) for s in shapes] for _ in range(6)]

    def run(opt, params, k0, k1, n):
        for k in range(k0, k1):
            for p, g in zip(params[:n], gs[k][:n]):
                p.grad = g.clone()
            opt.step()
    ours, ref = bnn.optim.Adam(pa[:2], lr=1e-2), torch.optim.Adam(pb[:2], lr=1e-2)
    run(ours, pa, 0, 2, 2); run(ref, pb, 0, 2, 2)
    extra = dict(lr=3e-3, betas=(0.8, 0.99), weight_decay=0.01)
    ours.add_param_group(dict(params=pa[2:], **extra)); ref.add_param_group(dict(params=pb[2:], **extra))
    run(ours, pa, 2, 4, 4); run(ref, pb, 2, 4, 4)
    assert [float(g["step_dev"]) for g in ours.param_groups] == [4.0, 2.0]
    sd = ours.state_dict()
    assert [float(sd["state"][i]["step"]) for i in range(4)] == [4.0, 4.0, 2.0, 2.0]
    assert all("step_dev" not in g for g in sd["param_groups"])
    two = lambda ps: [dict(params=ps[:2]), dict(params=ps[2:])]
    ours2 = bnn.optim.Adam(two(pa), lr=1.0); ours2.load_state_dict(copy.deepcopy(sd))
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ref2 = torch.optim.Adam(two(pc), lr=1.0); ref2.load_state_dict(copy.deepcopy(sd))
    assert [float(g["step_dev"]) for g in ours2.param_groups] == [4.0, 2.0]
    assert [g["lr"] for g in ours2.param_groups] == [1e-2, 3e-3]
    run(ours2, pa, 4, 6, 4); run(ref, pb, 4, 6, 4); run(ref2, pc, 4, 6, 4)
    for a, b, c in zip(pa, pb, pc):
        assert rel_err(a.detach(), b.detach()) < BAR and rel_err(c.detach(), b.detach()) < BAR
    assert [float(g["step_dev"]) for g in ours2.param_groups] == [6.0, 4.0]
    # and back: torch's state_dict loads into ours
    ours3 = bnn.optim.Adam(two(pa), lr=1.0); ours3.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert [float(g["step_dev"]) for g in ours3.param_groups] == [6.0, 4.0]


# ------------------------------------------------------------------------------------------------------------ 10. data parallel
def test_data_parallel_graphed_step_follows_rate_change_subprocess():
    """DataParallelELBO.make_graphed_step at world size 1 (no collective forced): a rate change between replays takes effect --
    the parameters differ from a run without the change and equal the eager bucket step with the change, below 2e-6."""
    _run(r"""
import sys, copy, torch
sys.path.insert(0, @ROOT@)
sys.path.insert(0, @ROOT@ + "/tests")
import bnn_amd
from bnn_amd import layers
from bnn_amd.parallel import DataParallelELBO
from conftest import rel_err
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.mnf.BayesianNetwork((784, 128, 64, 10), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
init = copy.deepcopy(net.state_dict())
x = torch.rand(256, 1, 28, 28, device=dev); y = torch.randint(0, 10, (256,), device=dev)
res = {}
for mode in ("graph-change", "graph-plain", "eager-change"):      # graphs first (an eager autograd graph breaks a later capture)
    net.load_state_dict(init)
    opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-3)
    dp = DataParallelELBO(net)
    if mode.startswith("graph"):
        step = dp.make_graphed_step(opt, x, y, 100, warmup=2)
        net.load_state_dict(init)
        for st in opt.state.values():
            st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
        for g in opt.param_groups:
            g["step_dev"].zero_()
    for it in range(4):
        if it == 2 and mode.endswith("change"):
            opt.param_groups[0]["lr"] = 1e-4
        bnn_amd.manual_seed(50 + it)
        if mode.startswith("eager"):
            opt.zero_grad(set_to_none=True)
            loss = dp.loss(net(x, sample=True), y, 100)
            with layers.vector_backward_overlap():
                loss.backward()
            dp.all_reduce_grads(unpack=False)
            opt.step(grads=dp.reduced_grads())
            del loss
        else:
            step(x, y)
    torch.cuda.synchronize()
    res[mode] = {k: v.detach().clone() for k, v in net.named_parameters()}
    bnn_amd.graphs.release_module_graph_refs(net)
a, b, c = res["graph-change"], res["graph-plain"], res["eager-change"]
differ = sum(not torch.equal(a[k], b[k]) for k in a)
worst = max(rel_err(a[k], c[k]) for k in a)
print("dp: %d of %d tensors differ from the run without the change; worst rel err against eager with it %.3e" % (differ, len(a), worst))
assert differ > 0 and all(not torch.equal(a[k], b[k]) for k in a if k.endswith("weight_mu")), differ
assert worst < 2e-6, worst
print("DP_RATE_OK")
""", "DP_RATE_OK")
