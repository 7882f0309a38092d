"""GPU tier of the MNF replicate study (bnn_amd.study.fit_mnf_replicates, lbbnn_mnf_study_fit): one step's gradients and several
steps against the float64 restatement tests/mnf_replicate_study_ref.py at two parameter settings (the seeded initialisation and
acting flows), independence and determinism bit for bit, per-replicate inputs, the rate groups, the guard, and agreement with
the existing path (a network trained by graphs.make_graphed_train_step + optim.Adam with three groups).

The bars.  The kernel adds in another order than the existing autograd path, so its bar is 4x the error of THAT path against
the same restatement at the same shapes (the factor of test_replicate_study_gpu.py), measured on an MI355X with
``existing_path_grad_errors`` / ``existing_path_several`` below (DESIGN.md 9.6 has the table):
  one step's gradients   existing path worst 5.18e-5 of a tensor's max over the 14 cases (z_flow.1.b at 20 -> 1, acting flows:
                         one number, the sum of two terms of opposite sign; the kernel measured 8.17e-5 there and at most
                         3.1e-6 in the 13 other cases, where the existing path has at most 3.0e-5).  4x is 2.07e-4, above the
                         contract's 1e-4: the bar is 1e-4, not widened
  several steps          existing path worst 3.99e-6 (parameters and moments, relative to the tensor's max) and 8.49e-8
                         (the epochs' mean and last loss) (the kernel measured 4.45e-6 and 8.49e-8)
"""
import copy
import functools

import numpy as np
import pytest
import torch

import mnf_replicate_study_ref as ref

pytestmark = pytest.mark.gpu

CONTRACT = 1e-4                        # the package's contract (test_parity_gpu.TOL): no bar is wider
GRAD_EXISTING = 5.18e-5                # measured: the autograd path against the restatement, worst tensor of the 14 cases
GRAD_BAR = min(4 * GRAD_EXISTING, CONTRACT)       # 4x would be 2.07e-4: the bar is the contract's 1e-4, not widened
STEPS_EXISTING = 3.99e-6               # measured: the graphed step for the same six steps, parameters and moments
STEPS_BAR = min(4 * STEPS_EXISTING, CONTRACT)
LOSS_EXISTING = 8.49e-8                # measured: the loss of those steps
LOSS_BAR = min(4 * LOSS_EXISTING, CONTRACT)

# (I, O, B, T): one element; a partial Philox group of 4 in every vector stream; the study's shape; odd sizes; both sides of a
# wave boundary (65 vector owners); both limits (I = 256 with four transforms, O = 16)
GRAD_SHAPES = [(1, 1, 1, 1), (3, 2, 5, 2), (20, 1, 400, 2), (33, 3, 7, 3), (65, 2, 5, 2), (256, 4, 64, 4), (64, 16, 65, 1)]
SETTINGS = ("seeded", "acting")
PRIORS_KW = dict(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
B1 = 0.9
MIN_GRAD_SHARE = 1e-4                  # no gradient element below this share of its tensor's max (the several-steps condition)


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_data(N, I, O, seed, R=None):
    """Standard-normal covariates and Bernoulli targets from a sparse logistic model, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    shape = (N, I) if R is None else (R, N, I)
    x = torch.randn(*shape, generator=g)
    w = torch.randn(I, O, generator=g) * (torch.rand(I, O, generator=g) < 0.4)
    y = (torch.rand(*shape[:-1], O, generator=g) < torch.sigmoid(x @ w)).float()
    return x, y


def rel(got, want):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).detach().cpu().double()
    return float((got.reshape(-1) - want.reshape(-1)).abs().max() / want.abs().max().clamp_min(1e-300))


def make_net(bnn, I, O, T, seed, offset, setting, device=None):
    """One replicate at a parameter setting: the seeded values, or those with acting flows for the step {seed, offset}."""
    import bnn_amd
    pri = bnn_amd.Priors(**PRIORS_KW)
    net = bnn_amd.study.make_mnf_replicates(1, (I, O), num_transforms=T, seeds=[seed], priors=pri)[0]
    if setting == "acting":
        ref.set_net_params(net, ref.acting(ref.net_params(net), seed, offset))
    return (net.to(device) if device is not None else net), pri


def net_tensors(bnn, net):
    return dict(bnn.study._named_tensors(net))


def state_rows(bnn, res, r, O, I, T):
    m = {k: v[r].cpu() for k, v in bnn.study.unpack_mnf(res.state.exp_avg, O, I, T, T).items()}
    v = {k: v[r].cpu() for k, v in bnn.study.unpack_mnf(res.state.exp_avg_sq, O, I, T, T).items()}
    return m, v


# ------------------------------------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def grad_reference(I, O, B, T, setting, seed=11, offset=5):
    net, pri = make_net(None, I, O, T, seed, offset, setting)
    x, y = make_data(B, I, O, 100 + I)
    return ref.fit(ref.net_params(net), x, y, 1, B, 0.01, seed=seed, offset=offset, priors=pri)["grads"][0]


SEVERAL = dict(I=20, O=1, T=2, B=16, N=2 * 16 + 5, epochs=2, lrs=[[0.01, 0.004, 0.0035], [0.004, 0.003, 0.002]], restarts=(1,),
               seed=9, offset=7, data_seed=1)
TWIN = dict(I=20, O=1, T=2, N=2000, B=400, seeds=[50, 51, 52], offset=3, r=1, data_seed=22)


def _conditioned(want):
    """The condition on the inputs, on the restatement, no element left out: every step is finite and Adam's normalised update
    is not decided by rounding."""
    if not all(want["finite"]):
        return False
    return all(float(g[n].abs().min()) >= MIN_GRAD_SHARE * float(g[n].abs().max()) for g in want["grads"] for n in g)


@functools.lru_cache(maxsize=None)
def several_reference(data_seed=None):
    c = SEVERAL
    net, pri = make_net(None, c["I"], c["O"], c["T"], c["seed"], c["offset"], "acting")
    x, y = make_data(c["N"], c["I"], c["O"], c["data_seed"] if data_seed is None else data_seed)
    want = ref.fit(ref.net_params(net), x, y, c["epochs"], c["B"], c["lrs"], restarts=c["restarts"], seed=c["seed"],
                   offset=c["offset"], priors=pri)
    return x, y, want


@functools.lru_cache(maxsize=None)
def twin_reference(data_seed=None):
    c = TWIN
    net, pri = make_net(None, c["I"], c["O"], c["T"], c["r"], c["offset"], "seeded")
    x, y = make_data(c["N"], c["I"], c["O"], c["data_seed"] if data_seed is None else data_seed)
    want = ref.fit(ref.net_params(net), x, y, 1, c["B"], 0.01, seed=c["seeds"][c["r"]], offset=c["offset"], priors=pri)
    return x, y, want


def pick_data_seed(reference, first=0, tries=200):
    """The first data seed at which the restatement shows the condition (CPU only; how SEVERAL / TWIN's data_seed were chosen.
    The gradients of the KL branch do not depend on the data: SEVERAL's ``seed`` -- the network's and the Philox state's -- is
    the first from 4 on at which one of the data seeds 0 .. 5 gives the condition)."""
    for s in range(first, first + tries):
        if _conditioned(reference(s)[2]):
            return s
    raise RuntimeError("no data seed with the condition")


# ------------------------------------------------------------------------------------------------ the existing path (yardstick)
def existing_path_grad_errors(bnn, dev, I, O, B, T, setting, seed=11, offset=5):
    """net(x, sample=True), elbo_bce_loss, backward() from Philox state {seed, offset}: per tensor, the error of .grad against
    the restatement's gradient relative to its max."""
    net, _ = make_net(bnn, I, O, T, seed, offset, setting, dev)
    net.train()
    x, y = make_data(B, I, O, 100 + I)
    want = grad_reference(I, O, B, T, setting, seed, offset)
    bnn.manual_seed(seed, offset)
    loss = bnn.elbo_bce_loss(net(x.to(dev), sample=True), y.to(dev), net.kl(), 1.0)
    loss.backward()
    return {n: rel(t.grad, want[n]) for n, t in net_tensors(bnn, net).items()}


def existing_path_fit(bnn, dev, net, x, y, epochs, batch, lrs, restarts, seed, offset):
    """Train ``net`` as the package could before the study kernel: one captured step per batch size
    (graphs.make_graphed_train_step), optim.Adam with the script's three groups behind the monitor's guard, the rates set per
    epoch, the optimizer state zeroed at a restart, Philox state {seed, offset} at the first step.  lrs: (epochs, 3).
    Returns (optimizer, [loss per step])."""
    N, O = x.shape[0], y.shape[1]
    nb = -(-N // batch)
    saved = [p.detach().clone() for p in net.parameters()]
    named = net_tensors(bnn, net)
    groups = [{"params": [t for n, t in named.items() if ref.group_of(n) == g], "lr": float(lrs[0][g])} for g in range(3)]
    opt = bnn.optim.Adam(groups, lr=float(lrs[0][0]))
    mon = bnn.TrainMonitor(O, dev)
    opt.set_guard(mon)

    def elbo(net, data, target):
        return bnn.elbo_bce_loss(net(data, sample=True), target, net.kl(), N / batch, monitor=mon)

    sizes = sorted({min(batch, N - k * batch) for k in range(nb)})
    steps = {bs: bnn.graphs.make_graphed_train_step(net, opt, elbo, x[:bs], y[:bs]) for bs in sizes}

    def reset_opt():
        for p in net.parameters():
            opt.state[p]["exp_avg"].zero_()
            opt.state[p]["exp_avg_sq"].zero_()
        for g in opt.param_groups:
            g["step_dev"].zero_()

    with torch.no_grad():                                            # the factory's warm-up steps trained the net: undo them
        for p, s in zip(net.parameters(), saved):
            p.copy_(s)
    reset_opt()
    mon.reset()
    bnn.manual_seed(seed, offset)
    losses = []
    for ep in range(epochs):
        if ep in restarts:
            reset_opt()
        for gi, g in enumerate(opt.param_groups):
            g["lr"] = float(lrs[ep][gi])
        for k in range(nb):
            rows = slice(k * batch, min((k + 1) * batch, N))
            losses.append(steps[rows.stop - rows.start](x[rows], y[rows]).clone())
    return opt, losses


def several_errors(named_params, m, v, want):
    errs = {}
    for n in want["params"]:
        errs["p." + n] = rel(named_params[n], want["params"][n])
        errs["m." + n] = rel(m[n], want["exp_avg"][n])
        errs["v." + n] = rel(v[n], want["exp_avg_sq"][n])
    return errs


def existing_path_several(bnn, dev):
    """The six steps of test_several_steps through the existing path: (tensor errors, loss errors)."""
    c = SEVERAL
    x, y, want = several_reference()
    net, _ = make_net(bnn, c["I"], c["O"], c["T"], c["seed"], c["offset"], "acting", dev)
    net.train()
    opt, losses = existing_path_fit(bnn, dev, net, x.to(dev), y.to(dev), c["epochs"], c["B"], c["lrs"], c["restarts"], c["seed"], c["offset"])
    named = net_tensors(bnn, net)
    errs = several_errors(named, {n: opt.state[t]["exp_avg"] for n, t in named.items()},
                          {n: opt.state[t]["exp_avg_sq"] for n, t in named.items()}, want)
    ls = [float(l.detach()) for l in losses]
    hist = want["history"]
    loss_errs = [abs(np.mean(ls[:3]) - hist[0, 0]) / abs(hist[0, 0]), abs(np.mean(ls[3:]) - hist[1, 0]) / abs(hist[1, 0]),
                 abs(ls[2] - hist[0, 3]) / abs(hist[0, 3]), abs(ls[5] - hist[1, 3]) / abs(hist[1, 3])]
    return errs, loss_errs


# ------------------------------------------------------------------------------------------------ one step, gradients
def kernel_grad_errors(bnn, dev, I, O, B, T, setting, seed=11, offset=5):
    net, _ = make_net(bnn, I, O, T, seed, offset, setting, dev)
    x, y = make_data(B, I, O, 100 + I)
    want = grad_reference(I, O, B, T, setting, seed, offset)
    res = bnn.study.fit_mnf_replicates([net], x.to(dev), y.to(dev), 1, B, lr=0.01, seeds=[seed], offset=offset, betas=(B1, 0.999))
    m, _ = state_rows(bnn, res, 0, O, I, T)
    assert float(res.state.step[0]) == 1.0 and int(res.skipped_steps[0]) == 0
    return {n: rel(m[n].double() / (1 - float(np.float32(B1))), want[n]) for n in want}


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("I,O,B,T", GRAD_SHAPES)
def test_one_step_gradients(bnn, dev, I, O, B, T, setting):
    """epochs = 1, one batch: exp_avg / (1 - beta1) is the gradient, of every tensor of the packed row."""
    errs = kernel_grad_errors(bnn, dev, I, O, B, T, setting)
    print("one-step gradient errors (I, O, B, T) = %s %s: worst %.2e (%s) %s"
          % ((I, O, B, T), setting, max(errs.values()), max(errs, key=errs.get), {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) < GRAD_BAR, errs


# ------------------------------------------------------------------------------------------------ several steps
def test_several_steps(bnn, dev):
    """20 -> 1, T = 2, acting flows, 2 epochs of 3 batches with a short last one, a restart at epoch 1, three different rate
    columns: parameters, moments, step counter, Philox offset and all six history columns."""
    c = SEVERAL
    x, y, want = several_reference()
    assert _conditioned(want) and len(want["grads"]) == 6
    net, _ = make_net(bnn, c["I"], c["O"], c["T"], c["seed"], c["offset"], "acting", dev)
    res = bnn.study.fit_mnf_replicates([net], x.to(dev), y.to(dev), c["epochs"], c["B"], lr=[r[0] for r in c["lrs"]],
                                       lr_z_flow=[r[1] for r in c["lrs"]], lr_r_flow=[r[2] for r in c["lrs"]],
                                       restarts=c["restarts"], seeds=[c["seed"]], offset=c["offset"])
    m, v = state_rows(bnn, res, 0, c["O"], c["I"], c["T"])
    assert list(res.params) == ref.names(c["T"], c["T"])
    errs = several_errors({n: res.params[n][0] for n in res.params}, m, v, want)
    hist = res.history[0].cpu().numpy()
    loss_errs = [abs(hist[e, k] - want["history"][e, k]) / abs(want["history"][e, k]) for e in range(2) for k in (0, 1, 3, 4)]
    print("several steps: worst tensor error %.2e (%s), worst loss error %.2e" % (max(errs.values()), max(errs, key=errs.get), max(loss_errs)))
    assert max(errs.values()) < STEPS_BAR, errs
    assert max(loss_errs) < LOSS_BAR, loss_errs
    assert np.array_equal(hist[:, 2], want["history"][:, 2]) and np.array_equal(hist[:, 5], [0.0, 0.0])
    assert float(res.state.step[0]) == want["step"] == 3                        # restarted at epoch 1
    assert res.state.rng[0].tolist() == [c["seed"], want["offset"]] and int(res.skipped_steps[0]) == 0
    for n, t in net_tensors(bnn, net).items():                                   # ... and the net holds the trained values
        assert torch.equal(t.detach().reshape(-1), res.params[n][0].reshape(-1)), n
    assert torch.equal(res.inclusion_probabilities[0], net.inclusion_probabilities()[0])


# ------------------------------------------------------------------------------------------------ independence, determinism
def _tiny(bnn, dev, R, I=5, O=2, N=11, T=2):
    pri = [bnn.Priors(**dict(PRIORS_KW, alpha_prior=0.2 + 0.5 * (r % 7) / 7)) for r in range(R)]
    nets = bnn.study.make_mnf_replicates(R, (I, O), num_transforms=T, priors=pri, device=dev)
    x, y = make_data(N, I, O, 5, R=R)
    g = torch.Generator().manual_seed(9)
    lr = (0.002 + 0.02 * torch.rand(3, R, 3, generator=g)).to(dev)              # [group](R, epochs)
    return nets, x.to(dev), y.to(dev), lr


def _fit(bnn, nets, x, y, lr, **kw):
    args = dict(epochs=3, batch_size=4, lr=lr[0].contiguous(), lr_z_flow=lr[1].contiguous(), lr_r_flow=lr[2].contiguous(),
                restarts=(2,), seeds=kw.pop("seeds", None) or [40 + r for r in range(len(nets))], offset=2)
    args.update(kw)
    return bnn.study.fit_mnf_replicates(nets, x, y, **args)


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    """Bit for bit: parameters, moments, counters, Philox states, history."""
    pairs = [(a.state.exp_avg, b.state.exp_avg), (a.state.exp_avg_sq, b.state.exp_avg_sq), (a.state.step, b.state.step),
             (a.state.rng, b.state.rng), (a.skipped_steps, b.skipped_steps), (a.history, b.history),
             (a.inclusion_probabilities, b.inclusion_probabilities)] + [(a.params[n], b.params[n]) for n in a.params]
    return all(torch.equal(p[rows_a].contiguous().view(torch.uint8), q[rows_b].contiguous().view(torch.uint8)) for p, q in pairs)


def _clone(nets):
    return [copy.deepcopy(n) for n in nets]


def test_replicate_of_a_call_equals_its_single_call_and_runs_repeat(bnn, dev):
    nets, x, y, lr = _tiny(bnn, dev, 3)
    a = _fit(bnn, _clone(nets), x, y, lr)
    b = _fit(bnn, _clone(nets), x, y, lr)
    assert _same(a, b)                                                           # two runs, the same bits
    for r in range(3):
        one = _fit(bnn, _clone(nets[r:r + 1]), x[r:r + 1], y[r:r + 1], lr[:, r:r + 1], seeds=[40 + r])
        assert _same(a, one, slice(r, r + 1), slice(0, 1)), r
    assert not torch.equal(a.params["z_flow.0.u"][0], a.params["z_flow.0.u"][1])
    assert torch.isfinite(a.history).all() and all(torch.isfinite(t).all() for t in a.params.values())


def test_more_workgroups_than_compute_units(bnn, dev):
    R = 300
    nets, x, y, lr = _tiny(bnn, dev, R, I=3, O=1, N=6)
    a = _fit(bnn, _clone(nets), x, y, lr)
    for r in (0, 77, 150, 255, 299):
        one = _fit(bnn, _clone(nets[r:r + 1]), x[r:r + 1], y[r:r + 1], lr[:, r:r + 1], seeds=[40 + r])
        assert _same(a, one, slice(r, r + 1), slice(0, 1)), r


def test_chunked_launches_and_continuing_from_state(bnn, dev):
    nets, x, y, lr = _tiny(bnn, dev, 3)
    whole = _fit(bnn, _clone(nets), x, y, lr)
    chunked = _fit(bnn, _clone(nets), x, y, lr, epochs_per_launch=1)
    assert _same(whole, chunked)
    cont = _clone(nets)
    first = _fit(bnn, cont, x, y, lr[:, :, :2], epochs=2, restarts=())
    second = _fit(bnn, cont, x, y, lr[:, :, 2:], epochs=1, restarts=(0,), state=first.state)
    pairs = [(whole.state.exp_avg, second.state.exp_avg), (whole.state.exp_avg_sq, second.state.exp_avg_sq),
             (whole.state.step, second.state.step), (whole.state.rng, second.state.rng),
             (whole.history[:, :2], first.history), (whole.history[:, 2:], second.history)]
    pairs += [(whole.params[n], second.params[n]) for n in whole.params]
    assert all(torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8)) for p, q in pairs)


def test_per_replicate_inputs_reach_their_replicate(bnn, dev):
    """(R, N, I) data, a priors table and three (R, epochs) rate tables: swap the inputs of replicates 0 and 2 and the results
    swap; each input changed for replicate 2 alone changes replicate 2 alone."""
    nets, x, y, lr = _tiny(bnn, dev, 3)
    a = _fit(bnn, _clone(nets), x, y, lr)
    perm = [2, 1, 0]
    swapped = [_clone(nets)[i] for i in perm]
    b = _fit(bnn, swapped, x[perm].contiguous(), y[perm].contiguous(), lr[:, perm], seeds=[40 + i for i in perm])
    for r in range(3):
        assert _same(a, b, slice(r, r + 1), slice(perm[r], perm[r] + 1)), r
    for change in ("x", "priors", "lr", "lr_z_flow", "lr_r_flow"):
        x2, lr2, nets2 = x.clone(), lr.clone(), _clone(nets)
        if change == "x":
            x2[2, 0, 0] += 0.5
        elif change.startswith("lr"):
            lr2[("lr", "lr_z_flow", "lr_r_flow").index(change), 2, 1] *= 1.5
        else:
            nets2[2].l1.priors = bnn.Priors(**dict(PRIORS_KW, sigma_prior=2.0))
        c = _fit(bnn, nets2, x2, y, lr2)
        assert _same(a, c, slice(0, 2), slice(0, 2)), change
        assert not torch.equal(a.params["weight_mu"][2], c.params["weight_mu"][2]), change


@pytest.mark.parametrize("frozen", ["z_flow", "r_flow"])
def test_rate_groups_reach_their_group(bnn, dev, frozen):
    """A zero rate for one flow: every tensor of that flow keeps its bits while the other flow and the named tensors move."""
    nets, x, y, lr = _tiny(bnn, dev, 2)
    before = [ref.net_params(n) for n in nets]
    kw = {"lr_" + frozen: 0.0}
    res = _fit(bnn, nets, x, y, lr, **kw)
    for r in range(2):
        for n in res.params:
            same = torch.equal(res.params[n][r].cpu().reshape(-1).view(torch.int32), before[r][n].reshape(-1).view(torch.int32))
            assert same == n.startswith(frozen), (r, n)


def test_ops_wrapper_argument_checks(bnn, dev):
    """ops.mnf_study_fit's own refusals on device tensors (n_epochs = 0: the valid call launches nothing): the row width, the
    (epochs, 3) / (R, epochs, 3) rate table, dtypes, contiguity, the data shapes."""
    from test_mnf_replicate_study_host import _ops_tensors
    ok = lambda **ch: dict(_ops_tensors(device=dev), **ch)
    t = _ops_tensors(device=dev)
    bnn.ops.mnf_study_fit(**t)                                                   # valid: a no-op
    bnn.ops.mnf_study_fit(**ok(lr=torch.zeros(2, 3, 3, device=dev), priors=torch.ones(2, 5, device=dev), x=torch.zeros(2, 6, 4, device=dev)))
    for bad in (dict(lr=torch.zeros(3, device=dev)), dict(lr=torch.zeros(2, 3, device=dev)), dict(lr=torch.zeros(3, 2, device=dev)),
                dict(priors=torch.ones(3, 5, device=dev)), dict(x=torch.zeros(6, 5, device=dev)), dict(y=torch.zeros(7, 1, device=dev))):
        with pytest.raises(ValueError):
            bnn.ops.mnf_study_fit(**ok(**bad))
    for bad in (dict(params=t["params"][:, :-1].contiguous()), dict(Tz=1), dict(exp_avg=t["exp_avg"].double()),
                dict(lr=t["lr"].double()), dict(rng=t["rng"].int()), dict(x=torch.zeros(4, 6, device=dev).t()),
                dict(history=torch.zeros(2, 3, 5, dtype=torch.float64, device=dev)), dict(restarts=torch.zeros(1, dtype=torch.int64, device=dev))):
        with pytest.raises(RuntimeError, match="must be a contiguous"):
            bnn.ops.mnf_study_fit(**ok(**bad))


# ------------------------------------------------------------------------------------------------ guard
def test_guard_skips_the_poisoned_batch_only(bnn, dev):
    c = SEVERAL
    x, y, _ = several_reference()
    mk = lambda: [make_net(bnn, c["I"], c["O"], c["T"], c["seed"], c["offset"], "acting", dev)[0] for _ in range(3)]
    xr = x.repeat(3, 1, 1)
    xr[1, c["B"] + 3, 4] = float("nan")                                         # replicate 1, a row of batch 1
    kw = dict(lr=[r[0] for r in c["lrs"]], lr_z_flow=[r[1] for r in c["lrs"]], lr_r_flow=[r[2] for r in c["lrs"]],
              restarts=c["restarts"], seeds=[c["seed"]] * 3, offset=c["offset"])
    clean = bnn.study.fit_mnf_replicates(mk(), x.to(dev), y.to(dev), c["epochs"], c["B"], **kw)
    nets = mk()
    res = bnn.study.fit_mnf_replicates(nets, xr.to(dev), y.to(dev), c["epochs"], c["B"], **kw)
    assert res.skipped_steps.tolist() == [0, 2, 0]
    assert res.history[1, :, 5].tolist() == [1.0, 1.0] and res.state.step.tolist() == [3.0, 2.0, 3.0]
    assert res.state.rng[:, 1].tolist() == [c["offset"] + 6] * 3                 # skipped steps advance the offset too
    for r in (0, 2):                                                             # the neighbours: bitwise the clean fit
        assert _same(res, clean, slice(r, r + 1), slice(r, r + 1)), r
    pri = bnn.Priors(**PRIORS_KW)
    P0 = ref.net_params(make_net(bnn, c["I"], c["O"], c["T"], c["seed"], c["offset"], "acting")[0])
    want = ref.fit(P0, x, y, c["epochs"], c["B"], c["lrs"], restarts=c["restarts"], seed=c["seed"], offset=c["offset"], priors=pri,
                   drop_steps=(1, 4))
    assert want["finite"] == [True, False, True, True, False, True]
    m, v = state_rows(bnn, res, 1, c["O"], c["I"], c["T"])
    errs = several_errors({n: res.params[n][1] for n in res.params}, m, v, want)
    assert max(errs.values()) < STEPS_BAR, errs
    assert all(torch.isfinite(t).all() for t in res.params.values())


# ------------------------------------------------------------------------------------------------ against the existing path
def test_agrees_with_a_twin_trained_by_the_graphed_step(bnn, dev):
    """20 -> 1, N = 2000, B = 400, T = 2, one epoch: nets[r] after the fit against a twin trained by make_graphed_train_step +
    optim.Adam (three groups) from the same seed and offset; freeze(nets[r], "mpm") then works on it."""
    c = TWIN
    I, O, T, N, B, r = c["I"], c["O"], c["T"], c["N"], c["B"], c["r"]
    x, y, want = twin_reference()
    assert _conditioned(want)
    pri = bnn.Priors(**PRIORS_KW)
    nets = bnn.study.make_mnf_replicates(3, (I, O), num_transforms=T, seeds=[0, 1, 2], priors=pri, device=dev)
    x, y = x.to(dev), y.to(dev)
    twin = bnn.study.make_mnf_replicates(1, (I, O), num_transforms=T, seeds=[r], priors=pri, device=dev)[0].train()
    opt, _ = existing_path_fit(bnn, dev, twin, x, y, 1, B, [[0.01, 0.01, 0.01]], (), seed=c["seeds"][r], offset=c["offset"])
    res = bnn.study.fit_mnf_replicates(nets, x, y, 1, B, lr=0.01, seeds=c["seeds"], offset=c["offset"])
    mine, theirs = net_tensors(bnn, nets[r]), net_tensors(bnn, twin)
    m, v = state_rows(bnn, res, r, O, I, T)
    diffs = {"p." + n: rel(mine[n], theirs[n]) for n in mine}
    diffs.update({"m." + n: rel(m[n], opt.state[theirs[n]]["exp_avg"]) for n in mine})
    diffs.update({"v." + n: rel(v[n], opt.state[theirs[n]]["exp_avg_sq"]) for n in mine})
    worst = max(diffs.values())
    print("twin: worst tensor difference %.2e (%s)" % (worst, max(diffs, key=diffs.get)))
    assert worst < STEPS_BAR, diffs
    # (five steps from weights of +-0.01 do not separate the classes yet: the accuracy is the restatement's, not a level)
    assert float(res.history[r, 0, 2]) == want["history"][0, 2] and int(res.skipped_steps[r]) == 0
    mpm = bnn.evaluate.freeze(nets[r], gates="mpm")
    out = bnn.evaluate.evaluate_batches(mpm, [(x, y)], samples=4)
    assert 0.0 <= out["accuracy_ensemble"] <= 1.0
