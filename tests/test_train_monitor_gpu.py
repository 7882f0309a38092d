"""GPU tier of the training monitor: lbbnn_elbo_loss_monitor behind elbo_loss(monitor=...), the guarded list
steps behind optimizer.set_guard(monitor), and both inside one captured training step.  Bitwise where the issue is "the same
arithmetic" (loss, gradients, updates); the counts exactly and the fp64 sums to the worst-case rounding of their additions
against the numpy restatement tests/train_monitor_ref.py.  The case that captures a HIP graph runs once, in a process of its
own, under a time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_monitor_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BATCHES = 15.0
# |got - ref| <= SUM_BOUND * sum|terms|: n * 2^-53 for the at most 7500 fp64 additions of a total here is 8.4e-13
SUM_BOUND = 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _rows(B, C, wide, seed, dev):
    """(buffer, log-probabilities): rows of C log-probabilities, dense or cut out of a wider buffer (ldp = C + 3)."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(B, C + (3 if wide else 0), generator=g)
    buf[:, :C] = torch.log_softmax(buf[:, :C] * 3, dim=1)
    buf = buf.to(dev)
    return buf, buf[:, :C]


def _targets(B, C, seed, dev):
    return torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed)).to(dev)


# ------------------------------------------------------------------------------------------- 1. the same bits as the plain loss
@pytest.mark.parametrize("C", [1, 2, 10, 64])
@pytest.mark.parametrize("B", [1, 7, 1023, 1024, 1025, 2500])
def test_monitored_loss_and_gradients_are_bitwise_the_plain_ones_leaf(bnn, dev, B, C):
    """A plain leaf tensor (the lbbnn_elbo_loss_backward_logits / _backward route without a head to hand over to): one pass,
    several passes and a ragged last pass of the 1024-thread loop; dense rows and rows of a wider buffer; kl given and None."""
    mon = bnn.TrainMonitor(C, dev)
    t = _targets(B, C, 100 + B, dev)
    steps = []
    for wide in (False, True):
        for with_kl in (False, True):
            got = []
            for monitor in (None, mon):
                buf, _ = _rows(B, C, wide, B * 7 + C, dev)
                buf.requires_grad_(True)
                kl = torch.tensor(123.456, device=dev, requires_grad=True) if with_kl else None
                loss = bnn.elbo_loss(buf[:, :C], t, kl, N_BATCHES, monitor=monitor)
                loss.backward()
                got.append((loss.detach().clone(), buf.grad.clone(), None if kl is None else kl.grad.clone()))
            assert torch.equal(got[0][0], got[1][0]), (wide, with_kl, float(got[0][0]), float(got[1][0]))
            assert torch.equal(got[0][1], got[1][1]), (wide, with_kl)
            if with_kl:
                assert torch.equal(got[0][2], got[1][2])
            steps.append(ref.step(buf.detach()[:, :C].cpu().numpy(), t.cpu().numpy(), float(kl.detach()) if with_kl else None,
                                  1.0 / N_BATCHES))
    # ... and the four monitored calls left the reference's totals at this shape
    r, want = mon.result(), ref.totals(steps)
    assert r["steps"] == 4 and r["rows"] == 4 * B and r["nonfinite_steps"] == 0
    for k in ref.COUNT_NAMES:
        assert r[k] == want[k], (k, r[k], want[k])
    for k in ref.SUM_NAMES:
        assert abs(r[k] - want[k]) <= SUM_BOUND * want[k + "_abs"], (k, r[k], want[k])
    assert r["last_loss"] == float(got[1][0])


@pytest.mark.parametrize("B", [7, 1025])
def test_monitored_loss_and_gradients_are_bitwise_the_plain_ones_fused_head(bnn, dev, B):
    """Log-probabilities out of a network's fused log_softmax head: the loss backward hands the logits' gradient to the head.
    Same parameters, same Philox state: the loss and every parameter gradient are the same bits with and without a monitor."""
    torch.manual_seed(0)
    net = bnn.lrt.BayesianNetwork((20, 16, 10)).to(dev).train()
    x = torch.rand(B, 20, generator=torch.Generator().manual_seed(1)).to(dev)
    t = _targets(B, 10, 2, dev)
    mon = bnn.TrainMonitor(10, dev)
    got = []
    for monitor in (None, mon):
        bnn.manual_seed(11)
        net.zero_grad(set_to_none=True)
        loss = bnn.elbo_loss(net(x, sample=True), t, net.kl(), N_BATCHES, monitor=monitor)
        loss.backward()
        got.append((loss.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()}))
        del loss
    assert torch.equal(got[0][0], got[1][0])
    assert got[0][1].keys() == got[1][1].keys() and len(got[0][1]) > 0
    for k in got[0][1]:
        assert torch.equal(got[0][1][k], got[1][1][k]), k
    r = mon.result()
    assert r["steps"] == 1 and r["rows"] == B and r["last_loss"] == float(got[1][0])


# ------------------------------------------------------------------------------------------------------- 2. / 3. totals, guard
C2 = 5


def _three_batches(dev):
    """[(log-probabilities, target, kl)]: 2500 rows out of a wider buffer with bad targets (-1, C, 2^40), a NaN row, a -inf row
    and a tie at the maximum, all three away from their rows' targets; 1025 dense rows whose row 3 has a NaN AT its target (the
    loss is not finite); 7 dense rows without kl."""
    _, a = _rows(2500, C2, True, 1, dev)
    ta = _targets(2500, C2, 2, dev)
    ta[5], ta[1023], ta[1024], ta[2499] = -1, C2, 2 ** 40, -7
    ta[10], ta[11], ta[12] = 0, 0, 4
    a[10, 3] = float("nan")                                   # a NaN is the arg-max: row 10 predicts 3, its target is 0
    a[11, 2] = float("-inf")
    a[12, 1] = a[12, 4] = 0.0                                 # tie at the maximum (log-probabilities are <= 0): index 1 wins, target 4
    a[1023, 0] = float("nan")                                 # a non-finite row with a bad target
    _, b = _rows(1025, C2, False, 3, dev)
    tb = _targets(1025, C2, 4, dev)
    tb[3] = 2
    b[3, 2] = float("nan")
    _, c = _rows(7, C2, False, 5, dev)
    tc = _targets(7, C2, 6, dev)
    kl = lambda v: torch.tensor(v, device=dev)
    return [(a, ta, kl(321.5)), (b, tb, kl(77.25)), (c, tc, None)]


@pytest.fixture(scope="module")
def three(bnn, dev):
    """The three batches, the reference's steps for them (computed once, shared, never changed) and the losses of the plain call."""
    batches = _three_batches(dev)
    steps = [ref.step(lp.cpu().numpy(), t.cpu().numpy(), None if kl is None else float(kl), 1.0 / N_BATCHES)
             for lp, t, kl in batches]
    plain = [bnn.elbo_loss(lp, t, kl, N_BATCHES) for lp, t, kl in batches]
    return batches, steps, plain


def test_totals_equal_the_reference(bnn, dev, three):
    batches, steps, plain = three
    assert [s["finite"] for s in steps] == [True, False, True]
    mons = [bnn.TrainMonitor(C2, dev), bnn.TrainMonitor(C2, dev)]
    for mon in mons:
        for (lp, t, kl), p in zip(batches, plain):
            loss = bnn.elbo_loss(lp, t, kl, N_BATCHES, monitor=mon)
            assert torch.equal(loss, p) or (torch.isnan(loss) and torch.isnan(p))
    want = ref.totals(steps)
    assert want["bad_targets"] == 4 and want["nonfinite_rows"] == 4 and want["nonfinite_steps"] == 1
    with pytest.raises(IndexError):
        mons[0].result()
    got = mons[0].result(strict=False)
    print("totals", {k: got[k] for k in ref.COUNT_NAMES})
    for k in ref.COUNT_NAMES:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ref.SUM_NAMES:
        print("%s got %.17g ref %.17g |diff| %.3g bound %.3g" % (k, got[k], want[k], abs(got[k] - want[k]), SUM_BOUND * want[k + "_abs"]))
        assert abs(got[k] - want[k]) <= SUM_BOUND * want[k + "_abs"], k
    # the last call's values: its nll to the rounding of its 7 additions, its loss the fp32 number the call returned
    assert abs(got["last_nll"] - steps[2]["nll"]) <= SUM_BOUND * steps[2]["abs_terms"]
    assert got["last_loss"] == float(plain[2]) and abs(got["last_loss"] - steps[2]["loss"]) <= 1.2e-7 * abs(steps[2]["loss"])
    for k in ("nll_mean", "loss_mean", "accuracy"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    # the same calls, the same bits
    assert torch.equal(mons[0]._totals, mons[1]._totals) and torch.equal(mons[0]._guard, mons[1]._guard)
    mons[0].reset()
    assert all(v == 0 for v in mons[0]._read()) and int(mons[0]._guard) == 0


def test_guard_word_follows_the_last_step(bnn, dev, three):
    batches, _, _ = three
    mon = bnn.TrainMonitor(C2, dev)
    seen = []
    for i in (0, 1, 2, 1, 1, 0):
        lp, t, kl = batches[i]
        bnn.elbo_loss(lp, t, kl, N_BATCHES, monitor=mon)
        seen.append(int(mon._guard))
    assert seen == [0, 1, 0, 1, 1, 0]                         # per step, not sticky
    r = mon.result(strict=False)
    assert r["steps"] == 6 and r["nonfinite_steps"] == 3 and r["skipped_steps"] == 0


# ---------------------------------------------------------------------------------------------------------- 4. / 5. guarded step
SIZES = [1, 3, 4095, 4096, 4097, 10000]
CASES = {"adam": ("Adam", dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.01)),
         "adamw": ("Adam", dict(lr=1e-2, weight_decay=0.1, decoupled_weight_decay=True)),
         "adam_mask": ("Adam", dict(lr=1e-2)),
         "adam_clip": ("Adam", dict(lr=1e-2, max_grad_norm=1.0)),
         "sgd": ("SGD", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01))}


def _twin(bnn, dev, case, layout, guard):
    """(optimizer, parameters): the same values and groups for every call.  "sizes": the sizes at which the list kernels take
    another path (one element, a ragged float4, one chunk less / exactly / plus one element, several chunks) plus a view that
    starts 4 bytes off a 16-byte boundary (the non-vector path), in three groups one of which is empty; "seventy": 70 tensors,
    more than one list holds."""
    g = torch.Generator().manual_seed(3)
    if layout == "sizes":
        ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(dev)) for n in SIZES]
        ps.append(torch.nn.Parameter(torch.randn(1004, generator=g).to(dev)[1:1002]))
        assert ps[-1].data_ptr() % 16 == 4 and ps[-1].is_contiguous()
        groups = [dict(params=ps[:3]), dict(params=[], lr=0.5), dict(params=ps[3:], lr=3e-3)]
    else:
        ps = [torch.nn.Parameter(torch.randn(5 + (i % 9) * 31, generator=g).to(dev)) for i in range(70)]
        groups = [dict(params=ps[:40]), dict(params=ps[40:], lr=3e-3)]
    name, kw = CASES[case]
    opt = getattr(bnn.optim, name)(groups, **kw)
    if case == "adam_mask":
        for p in ps[::2]:
            opt.set_grad_mask(p, (torch.rand(p.shape, generator=g) > 0.5).float().to(dev))
    opt.set_guard(guard)
    return opt, ps


def _grads(ps, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g).to(dev) for p in ps]


def _step(opt, ps, grads):
    for p, gr in zip(ps, grads):
        p.grad = gr.clone()
    opt.step()


def _state(opt, ps):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [v.clone() for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
    return out + [opt._tables()["steps"].clone()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("layout", ["sizes", "seventy"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_guarded_step(bnn, dev, case, layout):
    mon = bnn.TrainMonitor(10, dev)
    og, pg = _twin(bnn, dev, case, layout, mon)
    ou, pu = _twin(bnn, dev, case, layout, None)
    many = layout == "seventy"
    # guard 0: three steps, bitwise the unguarded twin's (parameters, moments, step counters)
    for it in range(3):
        gs = _grads(pg, 10 + it, dev)
        _step(og, pg, gs)
        _step(ou, pu, gs)
    assert _same(_state(og, pg), _state(ou, pu))
    want_steps = [3.0, 0.0, 3.0] if not many else [3.0, 3.0]
    assert og._tables()["steps"].tolist() == want_steps
    assert mon.result()["skipped_steps"] == 0
    # guard 1: nothing moves, every step() is counted once (a step of two lists too), the ticket is back at zero
    before = _state(og, pg)
    mon._guard.fill_(1)
    for it in range(2):
        _step(og, pg, _grads(pg, 20 + it, dev))
        assert _same(_state(og, pg), before)
        assert mon.result()["skipped_steps"] == it + 1
        assert og._tables()["ticket"].tolist() == [0, 0, 0, 0]
    # finite, bad, finite: the unguarded twin that saw only the two finite steps
    for it, flag in enumerate((0, 1, 0)):
        gs = _grads(pg, 30 + it, dev)
        mon._guard.fill_(flag)
        _step(og, pg, gs)
        if not flag:
            _step(ou, pu, gs)
    assert _same(_state(og, pg), _state(ou, pu))
    assert og._tables()["steps"].tolist() == ou._tables()["steps"].tolist() == ([5.0, 0.0, 5.0] if not many else [5.0, 5.0])
    assert mon.result()["skipped_steps"] == 3
    assert og._tables()["ticket"].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 6. the scale as a gradient check
@pytest.mark.parametrize("name", ["Adam", "SGD"])
def test_infinite_max_grad_norm_is_a_pure_gradient_check(bnn, dev, name):
    mon = bnn.TrainMonitor(10, dev)
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(n, generator=g).to(dev) for n in (3, 4097, 10000)]
    kw = dict(lr=1e-2, momentum=0.9) if name == "SGD" else dict(lr=1e-2)
    pa = [torch.nn.Parameter(t.clone()) for t in base]
    pb = [torch.nn.Parameter(t.clone()) for t in base]
    oa = getattr(bnn.optim, name)(pa, max_grad_norm=float("inf"), **kw)
    oa.set_guard(mon)
    ob = getattr(bnn.optim, name)(pb, **kw)
    gs = _grads(pa, 6, dev)
    _step(oa, pa, gs)
    _step(ob, pb, gs)
    assert float(oa._tables()["scale"]) == 1.0                # nothing is clipped
    assert _same(_state(oa, pa), _state(ob, pb))              # bitwise the unclipped, unguarded update
    for poison in (float("nan"), float("inf")):
        before, skipped = _state(oa, pa), mon.result()["skipped_steps"]
        bad = [x.clone() for x in _grads(pa, 7, dev)]
        bad[1][4000] = poison
        _step(oa, pa, bad)                                    # the loss flag is 0: the scale alone stops the step
        assert int(mon._guard) == 0 and not np.isfinite(float(oa._tables()["scale"]))
        assert _same(_state(oa, pa), before)
        assert mon.result()["skipped_steps"] == skipped + 1
    gs = _grads(pa, 8, dev)
    _step(oa, pa, gs)
    _step(ob, pb, gs)
    assert _same(_state(oa, pa), _state(ob, pb))


# -------------------------------------------------------------------------------------------------------------- 7. under a graph
def test_monitored_guarded_step_under_a_graph_subprocess():
    """lrt (20, 16, 3), B = 8, optim.Adam behind the monitor's guard, the loss with monitor=mon, all in one captured step.
    Three finite replays train and leave the totals of the reference fed the log-probabilities of the same three steps run
    eagerly from the same parameters and Philox offsets; a replay on a poisoned input changes no parameter, moment or counter
    and is counted once as non-finite and once as skipped; the next finite replay trains again.
    The poison is +inf in one input column, not a NaN: the ReLU of the hidden layer's GEMM epilogue is a hardware max, which
    returns 0 for a NaN, so a NaN in the INPUT never reaches the loss of this network (the step is then an ordinary finite one);
    an infinite input gives every hidden unit +inf, 0 or NaN -> 0, and one +inf activation makes the whole row of
    log-probabilities NaN."""
    code = r"""
import sys, copy, torch
sys.path.insert(0, @ROOT@)
sys.path.insert(0, @TESTS@)
import bnn_amd
from bnn_amd import layers
import train_monitor_ref as ref
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = bnn_amd.lrt.BayesianNetwork((20, 16, 3)).to(dev).train()
init = copy.deepcopy(net.state_dict())
mon = bnn_amd.TrainMonitor(3, dev)
opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-2)
opt.set_guard(mon)
g = torch.Generator().manual_seed(1)
xs = [torch.rand(8, 20, generator=g).to(dev) for _ in range(4)]
ys = [torch.randint(0, 3, (8,), generator=g).to(dev) for _ in range(4)]
lf = lambda n, a, b: bnn_amd.elbo_loss(n(a, sample=True), b, n.kl(), 15, monitor=mon)
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, xs[0], ys[0])
assert mon.result()["steps"] == 3                      # the factory's eager warm-up steps are real steps
mon.reset()

def reset():
    net.load_state_dict(init)
    for s in opt.state.values():
        s["exp_avg"].zero_(); s["exp_avg_sq"].zero_()
    for gr in opt.param_groups:
        gr["step_dev"].zero_()
    bnn_amd.manual_seed(7)

def state():
    out = [p.detach().clone() for p in net.parameters()]
    for p in net.parameters():
        out += [opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()]
    return out + [gr["step_dev"].clone() for gr in opt.param_groups]

same = lambda a, b: all(torch.equal(u, v) for u, v in zip(a, b))
reset()
s0 = state()
gl = [float(step(xs[i], ys[i])) for i in range(3)]
got = mon.result()
s3 = state()
assert not same(s0, s3) and float(opt.param_groups[0]["step_dev"]) == 3.0
assert got["steps"] == 3 and got["nonfinite_steps"] == 0 and got["skipped_steps"] == 0 and int(mon._guard) == 0
xn = xs[3].clone(); xn[:, 5] = float("inf")
ln = float(step(xn, ys[3]))
assert ln != ln, ln
assert same(state(), s3)
r = mon.result()
assert r["steps"] == 4 and r["nonfinite_steps"] == 1 and r["skipped_steps"] == 1 and int(mon._guard) == 1, r
lf4 = float(step(xs[3], ys[3]))
s5 = state()
assert lf4 == lf4 and not same(s5, s3) and float(opt.param_groups[0]["step_dev"]) == 4.0
r = mon.result()
assert r["steps"] == 5 and r["nonfinite_steps"] == 1 and r["skipped_steps"] == 1 and int(mon._guard) == 0, r
assert all(u.isfinite().all() for u in s5)
# the first three steps again, eagerly, without monitor or guard: the log-probabilities the reference is fed
opt.set_guard(None)
reset()
steps, el = [], []
for i in range(3):
    opt.zero_grad(set_to_none=True)
    lp = net(xs[i], sample=True)
    kl = net.kl()
    loss = bnn_amd.elbo_loss(lp, ys[i], kl, 15)
    steps.append(ref.step(lp.detach().cpu().numpy(), ys[i].cpu().numpy(), float(kl.detach()), 1.0 / 15))
    with layers.vector_backward_overlap():
        loss.backward()
    opt.step()
    el.append(float(loss.detach()))
del loss, lp, kl
torch.cuda.synchronize()
assert gl == el, (gl, el)
assert same(state(), s3)
want = ref.totals(steps)
for k in ref.COUNT_NAMES:
    assert got[k] == want[k], (k, got[k], want[k])
for k in ref.SUM_NAMES:
    assert abs(got[k] - want[k]) <= 1e-12 * want[k + "_abs"], (k, got[k], want[k])
assert got["last_loss"] == gl[2] and abs(got["last_nll"] - steps[2]["nll"]) <= 1e-12 * steps[2]["abs_terms"]
print("MONITORGRAPH_OK", gl, got["accuracy"])
""".replace("@ROOT@", repr(ROOT)).replace("@TESTS@", repr(os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "MONITORGRAPH_OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])


# --------------------------------------------------------------------------------------------------------------- 8. target guard
def test_a_target_the_kernel_cannot_read_is_refused_on_the_host(bnn, dev):
    """A target on another device, or with fewer elements than rows, never reaches the library.  (Both calls carry monitor= on
    purpose: code without the keyword refuses them with a TypeError before any pointer is handed over.)"""
    B, C = 16, 10
    mon = bnn.TrainMonitor(C, dev)
    _, lp = _rows(B, C, False, 1, dev)
    t = _targets(B, C, 2, dev)
    with pytest.raises(ValueError, match="target is on cpu"):
        bnn.elbo_loss(lp, t.cpu(), monitor=mon)
    with pytest.raises(ValueError, match="15 element"):
        bnn.elbo_loss(lp, t[:B - 1], monitor=mon)
    assert mon.result()["steps"] == 0
