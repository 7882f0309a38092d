"""GPU tier of the replicate study (bnn_amd.study.fit_replicates, lbbnn_lrt_study_fit): one step's gradients and several steps
against the float64 restatement tests/replicate_study_ref.py, independence and determinism bit for bit, per-replicate inputs,
the guard, and agreement with the existing path (a network trained by graphs.make_graphed_train_step + optim.Adam).

The bars.  The kernel adds its rows in another order than the existing autograd path, so its bar is 4x the error of THAT path
against the same restatement at the same shapes, measured on an MI355X with ``existing_path_grad_errors`` /
``existing_path_fit`` below (DESIGN.md 9.5 has the table):
  one step's gradients   existing path worst 9.73e-7 of a tensor's max (the kernel measured 5.15e-7)
  several steps          existing path worst 1.00e-6 (parameters and moments, relative to the tensor's max) and 8.97e-8
                         (the epochs' mean and last loss) (the kernel measured 1.76e-6 and 8.97e-8)
"""
import numpy as np
import pytest
import torch

import replicate_study_ref as ref

pytestmark = pytest.mark.gpu

GRAD_EXISTING = 9.73e-7                # measured: the autograd path against the restatement, worst tensor of the five shapes
GRAD_BAR = 4 * GRAD_EXISTING
STEPS_EXISTING = 1.00e-6               # measured: the graphed step for the same six steps, parameters and moments
STEPS_BAR = 4 * STEPS_EXISTING
LOSS_EXISTING = 8.97e-8                # measured: the loss of those steps
LOSS_BAR = 4 * LOSS_EXISTING

GRAD_SHAPES = [(1, 1, 1), (20, 1, 400), (33, 3, 7), (256, 4, 64), (64, 16, 65)]        # (I, O, B)
PRIORS_KW = dict(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
B1 = 0.9


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


def cpu_params(net):
    return {n: getattr(net.l1, n).detach().cpu().clone() for n in ref.NAMES}


def rel(got, want):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def state_rows(bnn, res, r, O, I):
    """Replicate r's exp_avg / exp_avg_sq as named CPU tensors."""
    m = {k: v[r].cpu() for k, v in bnn.study.unpack(res.state.exp_avg, O, I).items()}
    v = {k: v[r].cpu() for k, v in bnn.study.unpack(res.state.exp_avg_sq, O, I).items()}
    return m, v


# ------------------------------------------------------------------------------------------------ the existing path (yardstick)
def existing_path_grad_errors(bnn, dev, I, O, B, seed=11, offset=5):
    """net(x, sample=True), elbo_bce_loss, backward() from Philox state {seed, offset}: per tensor, the error of .grad against
    the restatement's gradient relative to its max."""
    pri = bnn.Priors(**PRIORS_KW)
    net = bnn.study.make_replicates(1, (I, O), seeds=[seed], priors=pri, device=dev)[0].train()
    x, y = make_data(B, I, O, 100 + I)
    want = ref.fit(cpu_params(net), x, y, 1, B, [0.01], seed=seed, offset=offset, priors=pri)["grads"][0]
    bnn.manual_seed(seed, offset)
    loss = bnn.elbo_bce_loss(net(x.to(dev), sample=True), y.to(dev), net.kl(), 1.0)
    loss.backward()
    return {n: rel(getattr(net.l1, n).grad, want[n]) for n in ref.NAMES}


def existing_path_fit(bnn, dev, net, x, y, epochs, batch, lrs, restarts, seed, offset):
    """Train ``net`` as the package could before the study kernel: one captured step per batch size
    (graphs.make_graphed_train_step), optim.Adam behind the monitor's guard, the rates set per epoch, the optimizer state zeroed
    at a restart, Philox state {seed, offset} at the first step.  Returns (optimizer, [loss per step])."""
    N = x.shape[0]
    O = y.shape[1]
    nb = -(-N // batch)
    saved = [p.detach().clone() for p in net.parameters()]
    opt = bnn.optim.Adam(net.parameters(), lr=float(lrs[0]))
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
        for g in opt.param_groups:
            g["lr"] = float(lrs[ep])
        for k in range(nb):
            rows = slice(k * batch, min((k + 1) * batch, N))
            losses.append(steps[rows.stop - rows.start](x[rows], y[rows]).clone())
    return opt, losses


# ------------------------------------------------------------------------------------------------ one step, gradients
def kernel_grad_errors(bnn, dev, I, O, B, seed=11, offset=5):
    pri = bnn.Priors(**PRIORS_KW)
    nets = bnn.study.make_replicates(1, (I, O), seeds=[seed], priors=pri, device=dev)
    x, y = make_data(B, I, O, 100 + I)
    want = ref.fit(cpu_params(nets[0]), x, y, 1, B, [0.01], seed=seed, offset=offset, priors=pri)["grads"][0]
    res = bnn.study.fit_replicates(nets, x.to(dev), y.to(dev), 1, B, lr=0.01, seeds=[seed], offset=offset, betas=(B1, 0.999))
    m, _ = state_rows(bnn, res, 0, O, I)
    return {n: rel(m[n].double() / (1 - float(np.float32(B1))), want[n]) for n in ref.NAMES}


@pytest.mark.parametrize("I,O,B", GRAD_SHAPES)
def test_one_step_gradients(bnn, dev, I, O, B):
    """epochs = 1, one batch: exp_avg / (1 - beta1) is the gradient.  One row; the study's shape; odd sizes with partial waves
    and a partial Philox group of 4; both limits (I = 256: five element slots, O = 16); a batch one past a wave multiple."""
    errs = kernel_grad_errors(bnn, dev, I, O, B)
    print("one-step gradient errors (I, O, B) = %s: %s" % ((I, O, B), {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) < GRAD_BAR, errs


# ------------------------------------------------------------------------------------------------ several steps
SEVERAL = dict(I=20, O=1, B=16, N=2 * 16 + 5, epochs=2, lrs=[0.01, 0.004], restarts=(1,), seed=4, offset=7, data_seed=2)


def several_inputs(bnn, dev):
    c = SEVERAL
    pri = bnn.Priors(**PRIORS_KW)
    nets = bnn.study.make_replicates(1, (c["I"], c["O"]), seeds=[c["seed"]], priors=pri, device=dev)
    x, y = make_data(c["N"], c["I"], c["O"], c["data_seed"])
    want = ref.fit(cpu_params(nets[0]), x, y, c["epochs"], c["B"], c["lrs"], restarts=c["restarts"], seed=c["seed"],
                   offset=c["offset"], priors=pri)
    return nets, x, y, want


def several_errors(named_params, m, v, want):
    errs = {}
    for n in ref.NAMES:
        errs["p." + n] = rel(named_params[n], want["params"][n])
        errs["m." + n] = rel(m[n], want["exp_avg"][n])
        errs["v." + n] = rel(v[n], want["exp_avg_sq"][n])
    return errs


def test_several_steps(bnn, dev):
    """2 epochs of 3 batches with a short last one, a restart at epoch 1, a two-value rate table: parameters, moments, step
    counter and all six history columns."""
    c = SEVERAL
    nets, x, y, want = several_inputs(bnn, dev)
    # the condition on the inputs, on the restatement, no element left out: Adam's normalised update is not decided by rounding
    assert all(want["finite"]) and len(want["grads"]) == 6
    for g in want["grads"]:
        for n in ref.NAMES:
            assert float(g[n].abs().min()) >= 1e-4 * float(g[n].abs().max()), n
    res = bnn.study.fit_replicates(nets, x.to(dev), y.to(dev), c["epochs"], c["B"], lr=c["lrs"], restarts=c["restarts"],
                                   seeds=[c["seed"]], offset=c["offset"])
    m, v = state_rows(bnn, res, 0, c["O"], c["I"])
    errs = several_errors({n: res.params[n][0] for n in ref.NAMES}, m, v, want)
    hist = res.history[0].cpu().numpy()
    loss_errs = [abs(hist[e, k] - want["history"][e, k]) / abs(want["history"][e, k]) for e in range(2) for k in (0, 1, 3, 4)]
    print("several steps: worst tensor error %.2e (%s), worst loss error %.2e" % (max(errs.values()), max(errs, key=errs.get), max(loss_errs)))
    assert max(errs.values()) < STEPS_BAR, errs
    assert max(loss_errs) < LOSS_BAR, loss_errs
    assert np.array_equal(hist[:, 2], want["history"][:, 2]) and np.array_equal(hist[:, 5], [0.0, 0.0])
    assert float(res.state.step[0]) == want["step"] == 3                        # restarted at epoch 1
    assert res.state.rng[0].tolist() == [c["seed"], want["offset"]] and int(res.skipped_steps[0]) == 0
    for n in ref.NAMES:                                                          # ... and the nets hold the trained values
        assert torch.equal(getattr(nets[0].l1, n).detach(), res.params[n][0])
    assert torch.equal(res.inclusion_probabilities[0], nets[0].inclusion_probabilities()[0])


# ------------------------------------------------------------------------------------------------ independence, determinism
def _tiny(bnn, dev, R, I=5, O=2, N=11):
    pri = [bnn.Priors(**dict(PRIORS_KW, alpha_prior=0.2 + 0.5 * (r % 7) / 7)) for r in range(R)]
    nets = bnn.study.make_replicates(R, (I, O), priors=pri, device=dev)
    x, y = make_data(N, I, O, 5, R=R)
    g = torch.Generator().manual_seed(9)
    lr = (0.002 + 0.02 * torch.rand(R, 3, generator=g)).to(dev)
    return nets, x.to(dev), y.to(dev), lr


def _fit(bnn, nets, x, y, lr, **kw):
    args = dict(epochs=3, batch_size=4, lr=lr, restarts=(2,), seeds=kw.pop("seeds", None) or [40 + r for r in range(len(nets))], offset=2)
    args.update(kw)
    return bnn.study.fit_replicates(nets, x, y, **args)


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    """Bit for bit: parameters, moments, counters, Philox states, history."""
    pairs = [(a.state.exp_avg, b.state.exp_avg), (a.state.exp_avg_sq, b.state.exp_avg_sq), (a.state.step, b.state.step),
             (a.state.rng, b.state.rng), (a.skipped_steps, b.skipped_steps), (a.history, b.history),
             (a.inclusion_probabilities, b.inclusion_probabilities)] + [(a.params[n], b.params[n]) for n in ref.NAMES]
    return all(torch.equal(p[rows_a].view(torch.uint8), q[rows_b].view(torch.uint8)) for p, q in pairs)


def _clone_nets(bnn, nets):
    import copy
    return [copy.deepcopy(n) for n in nets]


def test_replicate_of_a_call_equals_its_single_call_and_runs_repeat(bnn, dev):
    nets, x, y, lr = _tiny(bnn, dev, 3)
    a = _fit(bnn, _clone_nets(bnn, nets), x, y, lr)
    b = _fit(bnn, _clone_nets(bnn, nets), x, y, lr)
    assert _same(a, b)                                                           # two runs, the same bits
    for r in range(3):
        one = _fit(bnn, _clone_nets(bnn, nets[r:r + 1]), x[r:r + 1], y[r:r + 1], lr[r:r + 1], seeds=[40 + r])
        assert _same(a, one, slice(r, r + 1), slice(0, 1)), r
    assert not torch.equal(a.params["lambdal"][0], a.params["lambdal"][1])


def test_more_workgroups_than_compute_units(bnn, dev):
    R = 300
    nets, x, y, lr = _tiny(bnn, dev, R, I=3, O=1, N=6)
    a = _fit(bnn, _clone_nets(bnn, nets), x, y, lr)
    for r in (0, 77, 150, 255, 299):
        one = _fit(bnn, _clone_nets(bnn, nets[r:r + 1]), x[r:r + 1], y[r:r + 1], lr[r:r + 1], seeds=[40 + r])
        assert _same(a, one, slice(r, r + 1), slice(0, 1)), r


def test_chunked_launches_and_continuing_from_state(bnn, dev):
    nets, x, y, lr = _tiny(bnn, dev, 3)
    whole = _fit(bnn, _clone_nets(bnn, nets), x, y, lr)
    chunked = _fit(bnn, _clone_nets(bnn, nets), x, y, lr, epochs_per_launch=1)
    assert _same(whole, chunked)
    cont = _clone_nets(bnn, nets)
    first = _fit(bnn, cont, x, y, lr[:, :2].contiguous(), epochs=2, restarts=())
    second = _fit(bnn, cont, x, y, lr[:, 2:].contiguous(), epochs=1, restarts=(0,), state=first.state)
    pairs = [(whole.state.exp_avg, second.state.exp_avg), (whole.state.exp_avg_sq, second.state.exp_avg_sq),
             (whole.state.step, second.state.step), (whole.state.rng, second.state.rng),
             (whole.history[:, :2], first.history), (whole.history[:, 2:], second.history)]
    pairs += [(whole.params[n], second.params[n]) for n in ref.NAMES]
    assert all(torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8)) for p, q in pairs)


def test_per_replicate_inputs_reach_their_replicate(bnn, dev):
    """(R, N, I) data, a priors table and an (R, epochs) rate table: swap the inputs of replicates 0 and 2 and the results swap."""
    nets, x, y, lr = _tiny(bnn, dev, 3)
    a = _fit(bnn, _clone_nets(bnn, nets), x, y, lr)
    perm = [2, 1, 0]
    swapped = [_clone_nets(bnn, nets)[i] for i in perm]
    b = _fit(bnn, swapped, x[perm].contiguous(), y[perm].contiguous(), lr[perm].contiguous(), seeds=[40 + i for i in perm])
    for r in range(3):
        assert _same(a, b, slice(r, r + 1), slice(perm[r], perm[r] + 1)), r
    # each of the three per-replicate inputs matters on its own: changing it for replicate 2 changes replicate 2 only
    for change in ("x", "priors", "lr"):
        x2, lr2, nets2 = x.clone(), lr.clone(), _clone_nets(bnn, nets)
        if change == "x":
            x2[2, 0, 0] += 0.5
        elif change == "lr":
            lr2[2, 1] *= 1.5
        else:
            nets2[2].l1.priors = bnn.Priors(**dict(PRIORS_KW, sigma_prior=2.0))
        c = _fit(bnn, nets2, x2, y, lr2)
        assert _same(a, c, slice(0, 2), slice(0, 2)), change
        assert not torch.equal(a.params["weight_mu"][2], c.params["weight_mu"][2]), change


# ------------------------------------------------------------------------------------------------ guard
def test_guard_skips_the_poisoned_batch_only(bnn, dev):
    c = SEVERAL
    pri = bnn.Priors(**PRIORS_KW)
    nets = bnn.study.make_replicates(3, (c["I"], c["O"]), seeds=[c["seed"]] * 3, priors=pri, device=dev)
    x, y = make_data(c["N"], c["I"], c["O"], c["data_seed"])
    xr = x.repeat(3, 1, 1)
    xr[1, c["B"] + 3, 4] = float("nan")                                         # replicate 1, a row of batch 1
    clean = bnn.study.fit_replicates(_clone_nets(bnn, nets), x.to(dev), y.to(dev), c["epochs"], c["B"], lr=c["lrs"],
                                     restarts=c["restarts"], seeds=[c["seed"]] * 3, offset=c["offset"])
    res = bnn.study.fit_replicates(nets, xr.to(dev), y.to(dev), c["epochs"], c["B"], lr=c["lrs"], restarts=c["restarts"],
                                   seeds=[c["seed"]] * 3, offset=c["offset"])
    assert res.skipped_steps.tolist() == [0, 2, 0]
    assert res.history[1, :, 5].tolist() == [1.0, 1.0] and res.state.step.tolist() == [3.0, 2.0, 3.0]
    assert res.state.rng[:, 1].tolist() == [c["offset"] + 6] * 3                 # skipped steps advance the offset too
    for r in (0, 2):                                                             # the neighbours: bitwise the clean fit
        assert _same(res, clean, slice(r, r + 1), slice(r, r + 1)), r
    want = ref.fit(cpu_params(bnn.study.make_replicates(1, (c["I"], c["O"]), seeds=[c["seed"]], priors=pri)[0]), x, y, c["epochs"],
                   c["B"], c["lrs"], restarts=c["restarts"], seed=c["seed"], offset=c["offset"], priors=pri, drop_steps=(1, 4))
    assert want["finite"] == [True, False, True, True, False, True]
    m, v = state_rows(bnn, res, 1, c["O"], c["I"])
    errs = several_errors({n: res.params[n][1] for n in ref.NAMES}, m, v, want)
    assert max(errs.values()) < STEPS_BAR, errs
    assert all(torch.isfinite(res.params[n]).all() for n in ref.NAMES)


# ------------------------------------------------------------------------------------------------ against the existing path
def test_agrees_with_a_twin_trained_by_the_graphed_step(bnn, dev):
    """20 -> 1, N = 2000, B = 400, one epoch: nets[r] after the fit against a twin trained by make_graphed_train_step +
    optim.Adam from the same seed and offset; freeze(nets[r], "mpm") then works on it."""
    I, O, N, B, R = 20, 1, 2000, 400, 3
    pri = bnn.Priors(**PRIORS_KW)
    nets = bnn.study.make_replicates(R, (I, O), seeds=[0, 1, 2], priors=pri, device=dev)
    x, y = make_data(N, I, O, 21)
    x, y = x.to(dev), y.to(dev)
    r = 1
    twin = bnn.study.make_replicates(1, (I, O), seeds=[r], priors=pri, device=dev)[0].train()
    opt, _ = existing_path_fit(bnn, dev, twin, x, y, 1, B, [0.01], (), seed=50 + r, offset=3)
    res = bnn.study.fit_replicates(nets, x, y, 1, B, lr=0.01, seeds=[50, 51, 52], offset=3)
    worst = max(rel(getattr(nets[r].l1, n), getattr(twin.l1, n)) for n in ref.NAMES)
    m, v = state_rows(bnn, res, r, O, I)
    worst = max([worst] + [rel(m[n], opt.state[getattr(twin.l1, n)]["exp_avg"]) for n in ref.NAMES]
                + [rel(v[n], opt.state[getattr(twin.l1, n)]["exp_avg_sq"]) for n in ref.NAMES])
    print("twin: worst tensor difference %.2e" % worst)
    assert worst < STEPS_BAR
    assert float(res.history[r, 0, 2]) > 0.5 and int(res.skipped_steps[r]) == 0
    mpm = bnn.evaluate.freeze(nets[r], gates="mpm")
    out = bnn.evaluate.evaluate_batches(mpm, [(x, y)], samples=4)
    assert 0.5 < out["accuracy_ensemble"] <= 1.0
