"""GPU tier of the multi-group SGD: bnn_amd.optim.SGD on lbbnn_sgd_step_groups / lbbnn_grad_sumsq -- every parameter group in one
launch, rates / momentum / dampening / weight decay read from a device table (so they change under a captured graph), gradient
masks, global-norm clipping.  Parity bar unless a case says bitwise: the project's optimizer bar (the BAR of
test_adam_groups_gpu.py), max-norm relative error below 2e-6 against torch.optim.SGD on the same gradients (conftest.rel_err).
The case that captures a HIP graph runs once, in a process of its own, under a time limit."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-6
# the chunk boundary (4096 elements per workgroup) from both sides, an unaligned tail, more than one workgroup per tensor
SHAPES = [(1,), (7,), (33, 17), (4095,), (4096,), (4097,), (130, 1200)]
SHAPES12 = SHAPES + [(5,), (4097,), (33, 17), (7,), (4096,)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _params(dev, shapes, seed):
    g = torch.Generator().manual_seed(seed)
    base = [torch.randn(s, generator=g).to(dev) for s in shapes]
    return [torch.nn.Parameter(t.clone()) for t in base], [torch.nn.Parameter(t.clone()) for t in base]


def _set_grads(pa, pb, gs):
    for p, q, g in zip(pa, pb, gs):
        p.grad, q.grad = g.clone(), g.clone()


def _twelve_groups(params):
    """12 single-tensor groups: four rates, momentum in {0, 0.9}, dampening in {0, 0.1}, weight decay in {0, 0.01}, Nesterov
    where torch allows it (momentum > 0, dampening = 0)."""
    groups = []
    for i, p in enumerate(params):
        mom = (0.0, 0.9)[i % 2]
        damp = (0.0, 0.1)[(i // 2) % 2]
        groups.append(dict(params=[p], lr=(0.1, 0.01, 1e-3, 0.3)[i % 4], momentum=mom, dampening=damp,
                           weight_decay=(0.0, 0.01)[(i // 4) % 2], nesterov=bool(mom > 0 and damp == 0 and i % 3 == 0)))
    return groups


def _recorded_step(opt):
    from bnn_amd import _lib
    _lib.RECORD = rec = []
    try:
        opt.step()
    finally:
        _lib.RECORD = None
    torch.cuda.synchronize()
    return [name for name, _, _ in rec]


# ------------------------------------------------------------------------------------------------------------ parity with torch
def test_twelve_groups_match_torch_sgd(bnn, dev):
    torch.manual_seed(1)
    pa, pb = _params(dev, SHAPES12, 2)
    ga = _twelve_groups(pa)
    assert {(g["momentum"], g["dampening"], g["weight_decay"]) for g in ga} >= {(0.0, 0.0, 0.0), (0.9, 0.1, 0.01), (0.9, 0.0, 0.0)}
    assert any(g["nesterov"] for g in ga) and not all(g["nesterov"] for g in ga if g["momentum"] > 0 and g["dampening"] == 0)
    oa, ob = bnn.optim.SGD(ga, lr=1e-2), torch.optim.SGD(_twelve_groups(pb), lr=1e-2)
    for it in range(5):
        _set_grads(pa, pb, [torch.randn(s, device=dev) * (0.1 + it) for s in SHAPES12])
        oa.step(); ob.step()
    worst = max(rel_err(p.detach(), q.detach()) for p, q in zip(pa, pb))
    bufs = [(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"]) for p, q, g in zip(pa, pb, ga) if g["momentum"]]
    worst_b = max(rel_err(a, b) for a, b in bufs)
    print("12 groups: worst rel err parameters %.3e, momentum buffers %.3e" % (worst, worst_b))
    assert worst < BAR and worst_b < BAR and len(bufs) == 6
    # buffers only where the group has a momentum
    assert all(("momentum_buffer" in oa.state[p]) == bool(g["momentum"]) for p, g in zip(pa, ga))
    assert len(oa.param_groups) == 12 and all(float(g["step_dev"]) == 5.0 for g in oa.param_groups)
    base = oa.param_groups[0]["step_dev"].data_ptr()                   # one counter array, the groups' counters its views
    assert all(g["step_dev"].data_ptr() == base + 4 * i for i, g in enumerate(oa.param_groups))


def test_sixty_five_tensors_go_out_as_two_lists(bnn, dev):
    """65 tensors in two groups (one with momentum): two lbbnn_sgd_step_groups calls per step, with clipping exactly the two
    lbbnn_grad_sumsq calls more; the trajectory is clip_grad_norm_ + torch.optim.SGD's."""
    from bnn_amd import _lib
    assert _lib.ADAM_GROUPS_MAX_TENSORS == 64
    shapes = [SHAPES[i % 6] for i in range(65)]
    groups = lambda ps: [dict(params=ps[:40], lr=0.05, momentum=0.9), dict(params=ps[40:], lr=0.01, weight_decay=0.01)]
    for clip in (None, 0.5):
        pa, pb = _params(dev, shapes, 3)
        oa, ob = bnn.optim.SGD(groups(pa), lr=0.1, max_grad_norm=clip), torch.optim.SGD(groups(pb), lr=0.1)
        gen = torch.Generator().manual_seed(4)
        for it in range(3):
            _set_grads(pa, pb, [torch.randn(s, generator=gen).to(dev) * (0.02, 0.001, 0.05)[it] for s in shapes])
            if clip is not None:
                ref_norm = float(torch.nn.utils.clip_grad_norm_(pb, clip))
            names = _recorded_step(oa)
            ob.step()
            assert names == ([] if clip is None else ["lbbnn_grad_sumsq"] * 2) + ["lbbnn_sgd_step_groups"] * 2, names
            if clip is not None:
                assert abs(float(oa.grad_norm) - ref_norm) / ref_norm < BAR
        worst = max(rel_err(p.detach(), q.detach()) for p, q in zip(pa, pb))
        print("65 tensors, clip %s: worst rel err %.3e" % (clip, worst))
        assert worst < BAR
        assert [float(g["step_dev"]) for g in oa.param_groups] == [3.0, 3.0]


def test_launch_budget_one_call_per_list(bnn, dev):
    hdr = open(os.path.join(ROOT, "include", "lbbnn.h")).read()
    assert hdr.count("Launches: exactly 1.") == 2
    for clip in (None, 1.0):
        pa, _ = _params(dev, SHAPES12, 5)
        opt = bnn.optim.SGD(_twelve_groups(pa), lr=1e-2, max_grad_norm=clip)
        for p in pa:
            p.grad = torch.randn_like(p)
        opt.step()
        names = _recorded_step(opt)
        assert names == ([] if clip is None else ["lbbnn_grad_sumsq"]) + ["lbbnn_sgd_step_groups"], names
        assert all(float(g["step_dev"]) == 2.0 for g in opt.param_groups)


# --------------------------------------------------------------------------------------------------------------------- zero rate
def test_zero_rate_group_stays_bitwise_and_empty_steps_only_count(bnn, dev):
    pa, _ = _params(dev, SHAPES, 6)
    groups = [dict(params=pa[:3], lr=0.0, momentum=0.9, weight_decay=0.01), dict(params=pa[3:5], lr=0.1, momentum=0.9),
              dict(params=[], lr=0.1), dict(params=pa[5:], lr=0.0)]
    opt = bnn.optim.SGD(groups, lr=0.1)
    before = [p.detach().clone() for p in pa]
    for it in range(3):
        for p in pa:
            p.grad = torch.randn_like(p) * 10
        opt.step()
    frozen = pa[:3] + pa[5:]
    assert all(torch.equal(p.detach(), b) for p, b in zip(frozen, before[:3] + before[5:]))     # lr = 0: not one bit moves
    assert all(not torch.equal(p.detach(), b) for p, b in zip(pa[3:5], before[3:5]))
    assert all(opt.state[p]["momentum_buffer"].abs().max() > 0 for p in pa[:3])                  # the update ran, with rate 0
    assert [float(g["step_dev"]) for g in opt.param_groups] == [3.0, 3.0, 0.0, 3.0]              # the empty group does not count
    # a step without gradients: one advance-only launch, nothing moves
    snap = [p.detach().clone() for p in pa]
    bufs = [opt.state[p]["momentum_buffer"].clone() for p in pa[:5]]
    opt.zero_grad(set_to_none=True)
    assert _recorded_step(opt) == ["lbbnn_sgd_step_groups"]
    assert all(torch.equal(p.detach(), b) for p, b in zip(pa, snap))
    assert all(torch.equal(opt.state[p]["momentum_buffer"], b) for p, b in zip(pa[:5], bufs))
    assert [float(g["step_dev"]) for g in opt.param_groups] == [4.0, 4.0, 0.0, 4.0]


# ------------------------------------------------------------------------------------------------------------ masks and clipping
def test_mask_equals_hook_form_bitwise(bnn, dev):
    """set_grad_mask against multiplying .grad by the mask and then stepping: the same bits (parameters and buffers); and
    torch.optim.SGD on the masked gradients within the bar."""
    torch.manual_seed(7)
    shapes = [(130, 77), (4097,), (7,)]
    pa, pb = _params(dev, shapes, 8)
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    kw = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=0.01)
    oa, ob, oc = bnn.optim.SGD(pa, **kw), bnn.optim.SGD(pb, **kw), torch.optim.SGD(pc, **kw)
    masks = [(torch.rand(s, device=dev) < 0.5).float() for s in shapes[:2]] + [torch.rand(shapes[2], device=dev)]
    for p, m in zip(pa, masks):
        oa.set_grad_mask(p, m)
    for it in range(4):
        gs = [torch.randn(s, device=dev) for s in shapes]
        for p, q, r, g, m in zip(pa, pb, pc, gs, masks):
            p.grad, q.grad, r.grad = g.clone(), g * m, g * m
        oa.step(); ob.step(); oc.step()
    for p, q, r in zip(pa, pb, pc):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"])
        assert rel_err(p.detach(), r.detach()) < BAR


CLIP_SHAPES = SHAPES + [(300, 1000)]
CLIP_SCALES = [3e-4, 1e-3, 1e-2, 1.0, 2e-3, 0.3]                     # norms around max_grad_norm = 1 on both sides


def test_clipping_matches_clip_grad_norm_then_sgd(bnn, dev):
    pa, pb = _params(dev, CLIP_SHAPES, 9)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=0.01)
    oa, ob = bnn.optim.SGD(pa, max_grad_norm=1.0, **kw), torch.optim.SGD(pb, **kw)
    gen = torch.Generator().manual_seed(10)
    refs = []
    for it in range(6):
        gs = [torch.randn(s, generator=gen).to(dev) * CLIP_SCALES[it] for s in CLIP_SHAPES]
        _set_grads(pa, pb, gs)
        refs.append(float(torch.nn.utils.clip_grad_norm_(pb, 1.0)))
        oa.step(); ob.step()
        assert abs(float(oa.grad_norm) - refs[-1]) / refs[-1] < BAR
        assert torch.equal(pa[0].grad, gs[0])                        # .grad is not rescaled
    assert sum(r > 1.0 for r in refs) >= 2 and sum(r < 1.0 for r in refs) >= 2, refs
    worst = max(rel_err(p.detach(), q.detach()) for p, q in zip(pa, pb))
    print("clipping: reference norms %s, worst rel err %.3e" % (["%.4g" % r for r in refs], worst))
    assert worst < BAR


def test_clipping_propagates_nan_like_adam(bnn, dev):
    p = torch.nn.Parameter(torch.ones(10, device=dev))
    opt = bnn.optim.SGD([p], lr=1e-2, max_grad_norm=1.0)
    p.grad = torch.full((10,), float("nan"), device=dev)
    opt.step()
    assert torch.isnan(opt.grad_norm).all() and torch.isnan(p).all()


# ------------------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_round_trip_and_torch_interchange(bnn, dev):
    """Two groups at different counts (the second added after 2 steps, one with momentum and one without): state_dict() -> a fresh
    bnn_amd.optim.SGD and a fresh torch.optim.SGD -> 2 more steps: both agree with a torch.optim.SGD that never stopped."""
    torch.manual_seed(11)
    shapes = [(37, 5), (11,), (4097,), (3,)]
    pa, pb = _params(dev, shapes, 12)
    gs = [[torch.randn(s, device=dev) for s in shapes] for _ in range(6)]

    def run(opt, params, k0, k1, n):
        for k in range(k0, k1):
            for p, g in zip(params[:n], gs[k][:n]):
                p.grad = g.clone()
            opt.step()
    kw = dict(lr=0.05, momentum=0.9, dampening=0.1)
    ours, ref = bnn.optim.SGD(pa[:2], **kw), torch.optim.SGD(pb[:2], **kw)
    run(ours, pa, 0, 2, 2); run(ref, pb, 0, 2, 2)
    extra = dict(lr=0.01, momentum=0.0, weight_decay=0.01)
    ours.add_param_group(dict(params=pa[2:], **extra)); ref.add_param_group(dict(params=pb[2:], **extra))
    run(ours, pa, 2, 4, 4); run(ref, pb, 2, 4, 4)
    assert [float(g["step_dev"]) for g in ours.param_groups] == [4.0, 2.0]
    sd = ours.state_dict()
    assert all("step_dev" not in g for g in sd["param_groups"])
    assert sorted(sd["state"]) == [0, 1] and all(set(sd["state"][i]) == {"momentum_buffer"} for i in (0, 1))
    two = lambda ps: [dict(params=ps[:2]), dict(params=ps[2:])]
    ours2 = bnn.optim.SGD(two(pa), lr=1.0); ours2.load_state_dict(copy.deepcopy(sd))
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ref2 = torch.optim.SGD(two(pc), lr=1.0); ref2.load_state_dict(copy.deepcopy(sd))
    assert [float(g["step_dev"]) for g in ours2.param_groups] == [1.0, 0.0]       # a buffer came with the first group only
    assert [g["lr"] for g in ours2.param_groups] == [0.05, 0.01]
    run(ours2, pa, 4, 6, 4); run(ref, pb, 4, 6, 4); run(ref2, pc, 4, 6, 4)
    for a, b, c in zip(pa, pb, pc):
        assert rel_err(a.detach(), b.detach()) < BAR and rel_err(c.detach(), b.detach()) < BAR
    # and back: torch's state_dict loads into ours
    ours3 = bnn.optim.SGD(two(pa), lr=1.0); ours3.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert [float(g["step_dev"]) for g in ours3.param_groups] == [1.0, 0.0]
    # a fresh optimizer's state_dict has no buffers (its counters are 0): torch initialises them itself
    fresh = bnn.optim.SGD(two(pa), **kw)
    assert fresh.state_dict()["state"] == {}


def test_pushing_a_momentum_to_a_group_without_buffers_raises(bnn, dev):
    pa, _ = _params(dev, [(7,), (33, 17)], 13)
    opt = bnn.optim.SGD([dict(params=pa[:1], momentum=0.9), dict(params=pa[1:])], lr=0.1)
    for p in pa:
        p.grad = torch.randn_like(p)
    opt.step()
    assert "momentum_buffer" in opt.state[pa[0]] and "momentum_buffer" not in opt.state[pa[1]]
    opt.param_groups[0]["momentum"] = 0.5                                # a group with buffers may change its momentum
    assert opt.push_hyperparameters()
    opt.param_groups[1]["momentum"] = 0.9
    table = opt._tables()["hyper"].clone()
    with pytest.raises(RuntimeError):
        opt.push_hyperparameters()
    assert torch.equal(opt._tables()["hyper"], table)                    # a host check: nothing was copied
    with pytest.raises(RuntimeError):
        opt.step()
    opt.param_groups[1]["momentum"] = 0.0
    opt.step()


# ------------------------------------------------------------------------------------------------------------------ graph replay
def test_captured_step_equals_eager_and_follows_a_zero_rate_subprocess():
    """opt.step() captured over static .grad buffers: 4 replays equal 4 eager steps bit for bit; then one group's lr is set to 0
    between replays: that group is frozen bitwise, the others move, and the graph is the one captured before."""
    code = r"""
import sys, torch
sys.path.insert(0, @ROOT@)
import bnn_amd
dev = torch.device("cuda:0")
torch.manual_seed(0)
shapes = [(1,), (7,), (33, 17), (4095,), (4096,), (4097,), (130, 1200)]
base = [torch.randn(s, device=dev) for s in shapes]
pa = [torch.nn.Parameter(t.clone()) for t in base]
pb = [torch.nn.Parameter(t.clone()) for t in base]
groups = lambda ps: [dict(params=ps[:2], lr=0.1), dict(params=ps[2:4], lr=0.01, momentum=0.9, nesterov=True),
                     dict(params=ps[4:], lr=0.05, momentum=0.9, dampening=0.1, weight_decay=0.01)]
oa, ob = bnn_amd.optim.SGD(groups(pa), lr=0.1), bnn_amd.optim.SGD(groups(pb), lr=0.1)
static = [torch.zeros_like(p) for p in pa]
for p, g in zip(pa, static):
    p.grad = g
def feed(it):
    gen = torch.Generator().manual_seed(100 + it)
    for s, q, sh in zip(static, pb, shapes):
        g = torch.randn(sh, generator=gen).to(dev) * (0.5 + it)
        s.copy_(g); q.grad = g.clone()
feed(0); oa.step(); ob.step()                                  # eager: allocates the buffers outside the capture
graph = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with bnn_amd.graphs.capture(graph):
    oa.step()
for it in range(1, 5):
    feed(it); assert not oa.push_hyperparameters(); graph.replay(); ob.step()
torch.cuda.synchronize()
for p, q in zip(pa, pb):
    assert torch.equal(p.detach(), q.detach())
for p, q in zip(pa[2:], pb[2:]):
    assert torch.equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"])
assert [float(g["step_dev"]) for g in oa.param_groups] == [5.0] * 3
for o in (oa, ob):
    o.param_groups[1]["lr"] = 0.0
snap = [p.detach().clone() for p in pa]
for it in range(5, 8):
    feed(it); pushed = oa.push_hyperparameters(); assert pushed == (it == 5); graph.replay(); ob.step()
torch.cuda.synchronize()
assert all(torch.equal(p.detach(), s) for p, s in zip(pa[2:4], snap[2:4]))
assert all(not torch.equal(p.detach(), s) for p, s in zip(pa[:2] + pa[4:], snap[:2] + snap[4:]))
for p, q in zip(pa, pb):
    assert torch.equal(p.detach(), q.detach())
assert [float(g["step_dev"]) for g in oa.param_groups] == [8.0] * 3
print("SGD_REPLAY_OK")
"""
    r = subprocess.run([sys.executable, "-c", code.replace("@ROOT@", repr(ROOT))], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "SGD_REPLAY_OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


def test_data_parallel_graphed_step_with_sgd_subprocess():
    """DataParallelELBO.make_graphed_step at world size 1 with bnn_amd.optim.SGD (two groups, one with momentum): a rate change
    between replays takes effect -- the parameters differ from a run without the change and equal the eager bucket step with
    the change, below 2e-6 (the bar of the same case for Adam in tests/test_adam_groups_gpu.py) -- and a group whose rate goes to
    0 stays bitwise."""
    code = r"""
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
first = [p for n, p in net.named_parameters() if n.startswith("l1.")]
rest = [p for n, p in net.named_parameters() if not n.startswith("l1.")]
res, snap = {}, {}
for mode in ("graph-change", "graph-plain", "eager-change"):      # graphs first (an eager autograd graph breaks a later capture)
    net.load_state_dict(init)
    opt = bnn_amd.optim.SGD([dict(params=first, lr=1e-4, momentum=0.9), dict(params=rest, lr=1e-4)], lr=1e-4)
    dp = DataParallelELBO(net)
    if mode.startswith("graph"):
        step = dp.make_graphed_step(opt, x, y, 100, warmup=2)
        net.load_state_dict(init)
        for st in opt.state.values():
            st["momentum_buffer"].zero_()
        for g in opt.param_groups:
            g["step_dev"].zero_()
    for it in range(4):
        if it == 2 and mode.endswith("change"):
            opt.param_groups[0]["lr"] = 1e-5
            opt.param_groups[1]["lr"] = 0.0
            torch.cuda.synchronize()
            snap[mode] = [p.detach().clone() for p in rest]
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
    if mode.endswith("change"):
        assert all(torch.equal(p.detach(), s) for p, s in zip(rest, snap[mode])), mode       # rate 0: not one bit moves
    assert [float(g["step_dev"]) for g in opt.param_groups] == [4.0, 4.0]
    bnn_amd.graphs.release_module_graph_refs(net)
a, b, c = res["graph-change"], res["graph-plain"], res["eager-change"]
differ = sum(not torch.equal(a[k], b[k]) for k in a)
worst = max(rel_err(a[k], c[k]) for k in a)
print("dp sgd: %d of %d tensors differ from the run without the change; worst rel err against eager with it %.3e" % (differ, len(a), worst))
assert differ > 0 and all(not torch.equal(a[k], init[k]) for k in a if k.endswith("weight_mu")), differ
assert worst < 2e-6, worst
print("DP_SGD_OK")
"""
    env = dict(os.environ)
    env.pop("LBBNN_DP_FORCE_COLLECTIVE", None)
    r = subprocess.run([sys.executable, "-c", code.replace("@ROOT@", repr(ROOT))], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DP_SGD_OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
