"""GPU tier of the regression metrics on the device (include/lbbnn.h: lbbnn_eval_regression; evaluate.ensemble_regression /
RegressionAccumulator / evaluate_batches; graphs.make_graphed_eval_step) against tests/gaussian_ref.py.

BARS (float64 of the same expression on the same float32 inputs; ulp = 2^-24 = 6e-8 relative):
  * pred_mean and epistemic_var: bit for bit against the numpy float32 restatement in the documented order;
  * aleatoric_var = expf(lv): <= 2 ulp, bar 1e-6 relative;  total_std = sqrtf(ev + av) from the bit-exact ev: av's 2 ulp, the
    sum's 0.5, halved by the root plus its own 0.5: bar 1e-6 relative;
  * sq_err = e e with e = y - pred_mean from the bit-exact mean: 1.5 ulp, bar 1e-6 relative (+ 1e-30);
  * log_density: a member's term t_s = -0.5 ((L + lv) + q_s) carries under 5.5 ulp of S_s = |L| + |lv| + q_s
    (tests/test_gaussian_head_gpu.py), the logsumexp passes the largest term's error on and adds a few ulp of |mx| + log S, all
    below S_max: bar 1e-6 * (max_s S_s + |log_density| + log S + 1), absolute;
  * pit: Phi's argument (r hs) / sqrt 2 carries 4 ulp relative, which moves Phi by at most 4 ulp * max |t| phi(t) < 6e-8; erfcf's
    own <= 4 ulp of Phi <= 1 and the member sum's S / 2 ulp: bar 1e-6 absolute for S <= 10.
The PIT histogram is held EXACTLY against the float64 reference: the inputs are chosen on the CPU beforehand so that every
scored element's float64 pit * pit_bins lies at least 1e-4 from an integer (20 times the bar above); the margin is asserted here
with the reference alone and no element is dropped.  fp64 totals against the fp64 sums of the kernel's own fp32 values within
gaussian_ref.DBL * sum |value|; integer totals exact; two passes bit-identical."""
import math

import numpy as np
import pytest
import torch

import gaussian_ref as ref

pytestmark = pytest.mark.gpu

PIT_BINS = 20
MARGIN = 1e-4
# one element; 4 full workgroups of 256 elements, all 16 units; 6 workgroups, the last with 5 elements; 3, the last with 188
SHAPES = ((1, 1, 1), (2, 64, 16), (3, 257, 5), (10, 700, 1))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _same(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _inputs(S, B, O, seed, lv=None, spoil=True):
    """CPU float32 (outputs (S, B, O), target (B, O), log_var (O,), mean_outputs (B, O)): members spread about a centre, targets
    within two standard deviations of it, redrawn until every float64 pit * PIT_BINS lies 2 * MARGIN from an integer; then, with
    more than 8 elements, a NaN and an inf target and one infinite member output."""
    g = torch.Generator().manual_seed(seed)
    drawn = (0.6 * torch.randn(O, generator=g) - 0.5).float()
    lv = drawn if lv is None else lv
    centre = 2.0 * torch.randn(B, O, generator=g)
    out = (centre[None] + 0.4 * torch.randn(S, B, O, generator=g) * torch.exp(0.5 * lv)).float()
    sd = torch.exp(0.5 * lv)
    y = (centre + (4.0 * torch.rand(B, O, generator=g) - 2.0) * sd).float()
    for _ in range(200):
        v = ref.metrics(out.numpy(), y.numpy(), lv.numpy())["pit"] * PIT_BINS
        close = torch.from_numpy(np.abs(v - np.round(v)) < 2 * MARGIN)
        if not bool(close.any()):
            break
        y = torch.where(close, (centre + (4.0 * torch.rand(B, O, generator=g) - 2.0) * sd).float(), y)
    else:
        raise AssertionError("no inputs with the PIT margin")
    mean_out = (centre + 0.1 * torch.randn(B, O, generator=g)).float()
    if spoil and B * O > 8:
        y.view(-1)[2], y.view(-1)[B * O - 3] = float("nan"), float("inf")
        out[S - 1].view(-1)[5] = float("inf")
    return out, y, lv, mean_out


def _padded(out, dev):
    """The (S, B, O) block as the member GEMM leaves it: member stride pad4(B * O) (+ 4 to make every shape padded), NaN between."""
    S, B, O = out.shape
    ms = -(-B * O // 4) * 4 + 4
    buf = torch.full((S, ms), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :B * O] = out.reshape(S, -1).to(dev)
    return buf[:, :B * O].view(S, B, O)


def _check_rows(rows, out, y, lv, S):
    """The per-element outputs of one call against the references; returns them as float32 numpy arrays."""
    k = {n: v.cpu().numpy() for n, v in rows.items()}
    want = ref.metrics(out.numpy(), None if y is None else y.numpy(), lv.numpy())
    for n in ("pred_mean", "epistemic_var"):
        fin = np.isfinite(want[n])
        assert np.array_equal(k[n][fin].view(np.int32), want[n][fin].view(np.int32)), n
        assert not np.isfinite(k[n][~fin]).any(), n
    fin = np.isfinite(out.numpy()).all(0)
    worst = {}
    for n, bar in (("aleatoric_var", 1e-6 * want["aleatoric_var"]), ("total_std", 1e-6 * want["total_std"]),
                   ("sq_err", 1e-6 * np.abs(want["sq_err"]) + 1e-30),
                   ("log_density", 1e-6 * (want["log_density_mag"] + np.abs(want["log_density"]) + math.log(S) + 1.0)),
                   ("pit", np.full(fin.shape, 1e-6))):
        sel = fin & (want["valid"] if n in ("sq_err", "log_density", "pit") else True)
        if n in ("sq_err", "log_density", "pit"):
            assert np.isnan(k[n][~want["valid"]]).all(), n                         # NaN without a valid target
        if sel.any():
            with np.errstate(invalid="ignore"):
                diff = np.abs(k[n].astype(np.float64) - want[n])
            worst[n] = float((diff[sel] / bar[sel]).max())
            assert worst[n] <= 1.0, (n, worst[n])
    print("eval_regression S=%d rows: worst |value - ref| / bar %s" % (S, {n: "%.3g" % v for n, v in worst.items()}))
    return k


@pytest.mark.parametrize("tensor_lv", (False, True), ids=("float_lv", "tensor_lv"))
@pytest.mark.parametrize("with_mean", (False, True), ids=("no_mean", "mean"))
@pytest.mark.parametrize("S,B,O", SHAPES)
def test_rows_and_totals_against_the_references(bnn, dev, S, B, O, with_mean, tensor_lv):
    ev = bnn.evaluate
    # one noise level for the pass: a number for every unit, or a (units,) tensor
    lv = _inputs(1, 1, O, 99)[2] if tensor_lv else torch.full((O,), -0.75)
    batches = [_inputs(S, B, O, 1000 * S + 10 * B + O + k, lv=lv) for k in range(2)]
    for o, y, l, _ in batches:                                         # the margin, with the reference alone, no element dropped
        assert ref.pit_margin(o.numpy(), y.numpy(), l.numpy(), PIT_BINS) >= MARGIN
    lv_arg = lv.to(dev) if tensor_lv else -0.75
    accs = [ev.RegressionAccumulator(O, S, dev, lv_arg, pit_bins=PIT_BINS) for _ in range(2)]
    kernel = []
    for o, y, _, mo in batches:
        od, yd = _padded(o, dev), y.to(dev)
        mod = mo.to(dev) if with_mean else None
        rows = accs[0].update(od, yd, mod)
        kernel.append(_check_rows(rows, o, y, lv, S))
        rows2 = accs[1].update(od, yd, mod)
        assert all(_same(rows[n], rows2[n]) for n in rows)
        alone = ev.ensemble_regression(od, yd, lv_arg)                 # the per-element part alone: the same bits
        assert sorted(alone) == sorted(rows) and all(_same(rows[n], alone[n]) for n in rows)
    assert torch.equal(accs[0]._totals, accs[1]._totals)               # two passes: bit-identical totals
    spoiled = B * O > 8
    if spoiled:
        with pytest.raises(IndexError):
            accs[0].result()
    r = accs[0].result(strict=False)
    per = [(o, y, lv, mo if with_mean else None) for o, y, _, mo in batches]
    c, s, a, hist = ref.totals(per, PIT_BINS, kernel=kernel)
    for n in c:
        assert r[n] == c[n], (n, r[n], c[n])
    assert r["elements"] == 2 * B * O and r["bad_targets"] == (4 if spoiled else 0) and r["nonfinite_elements"] == (2 if spoiled else 0)
    assert np.array_equal(r["pit_hist"], hist), (r["pit_hist"], hist)
    assert int(r["pit_hist"].sum()) == r["scored_elements"]
    for n in s:
        print("%s_sum got %.17g ref %.17g" % (n, r[n + "_sum"], s[n]))
        assert abs(r[n + "_sum"] - s[n]) <= ref.DBL * a[n] + 1e-300, n
    # the derived numbers against the float64 reference's own totals (the per-element bars, summed)
    c64, s64, a64, _ = ref.totals(per, PIT_BINS)
    n_s = c64["scored_elements"]
    assert abs(r["rmse"] - math.sqrt(s64["sq_err"] / n_s)) <= 1e-6 * r["rmse"] + 1e-30
    assert abs(r["mae"] - s64["abs_err"] / n_s) <= 1e-6 * r["mae"] + 1e-30
    assert abs(r["mean_log_density"] - s64["log_density"] / n_s) <= 1e-5 * (a64["log_density"] / n_s + 10.0)
    if with_mean:
        assert abs(r["rmse_posterior_mean"] - math.sqrt(s64["posterior_mean_sq_err"] / n_s)) <= 1e-6 * r["rmse_posterior_mean"] + 1e-30
    else:
        assert r["rmse_posterior_mean"] is None
    cov = r["coverage"](0.9)
    assert cov == hist[1:19].sum() / hist.sum()
    if n_s > 100:
        sst = s64["y2"] - s64["y"] ** 2 / n_s
        assert abs(r["r2"] - (1.0 - s64["sq_err"] / sst)) <= 1e-5 and 0.5 < r["r2"] < 1.0


def test_a_target_far_from_every_member_has_a_finite_log_density(bnn, dev):
    """y 1e3 noise standard deviations from the members: every member's density underflows (exp(-5e5)), log(mean(exp)) is -inf,
    the streaming logsumexp is finite and within the bar of the float64 value; the PIT saturates at 0 / 1."""
    ev = bnn.evaluate
    S, B, O = 4, 6, 2
    g = torch.Generator().manual_seed(3)
    lv = torch.tensor([-1.0, 0.5])
    out = torch.randn(S, B, O, generator=g)
    y = out.mean(0) + 1e3 * torch.exp(0.5 * lv) * torch.tensor([1.0, -1.0])
    rows = ev.ensemble_regression(out.to(dev), y.to(dev), lv.to(dev))
    k = _check_rows(rows, out, y, lv, S)
    assert np.isfinite(k["log_density"]).all() and float(k["log_density"].max()) < -4e5
    t = -0.5 * (ref.LOG_2PI + lv.numpy().astype(np.float64) + ((y[None] - out).numpy().astype(np.float64) ** 2) * np.exp(-lv.numpy().astype(np.float64)))
    with np.errstate(divide="ignore"):
        assert np.isneginf(np.log(np.exp(t).mean(0))).all()                        # the naive form
    assert (k["pit"][:, 0] == 1.0).all() and (k["pit"][:, 1] == 0.0).all()
    # in an accumulator such elements land in the first / last bin (the clamp), and one -inf member output drops its element
    acc = ev.RegressionAccumulator(O, S, dev, lv.to(dev), pit_bins=PIT_BINS)
    o2 = out.clone()
    o2[1, 0, 0] = float("-inf")
    acc.update(o2.to(dev), y.to(dev))
    r = acc.result()
    assert r["pit_hist"][0] == B and r["pit_hist"][-1] == B - 1 and r["nonfinite_elements"] == 1 and r["scored_elements"] == 2 * B - 1
    assert math.isfinite(r["mean_log_density"])


def test_a_live_log_var_is_read_at_every_update(bnn, dev):
    ev = bnn.evaluate
    out, y, lv, _ = _inputs(3, 9, 2, 5, spoil=False)
    live = lv.clone().to(dev)
    acc = ev.RegressionAccumulator(2, 3, dev, live)
    a = acc.update(out.to(dev), y.to(dev))["aleatoric_var"].clone()
    live += 1.0                                                         # in place: the accumulator holds the tensor, not a copy
    b = acc.update(out.to(dev), y.to(dev))["aleatoric_var"]
    assert float((a.cpu() - torch.exp(lv)).abs().max()) <= 1e-6 * float(torch.exp(lv).max())
    assert float((b / a - math.e).abs().max()) <= 1e-5
    with pytest.raises(ValueError, match="built for"):
        acc.update(out[:2].to(dev), y.to(dev))
    with pytest.raises(ValueError, match="target must be"):
        acc.update(out.to(dev), y[:4].to(dev))
    with pytest.raises(ValueError, match="mean_outputs"):
        acc.update(out.to(dev), y.to(dev), y[:4].to(dev))


# ------------------------------------------------------------------------------------------------------------- the wiring
DIMS = (12, 16, 2)
SEED = 21


def _net(bnn, dev, kind="lrt"):
    torch.manual_seed(5)
    if kind == "lrt":
        net = bnn.lrt.BayesianNetwork(DIMS, head="identity")
    else:
        net = bnn.mnf.BayesianNetwork(DIMS, 2, z_flow_type="Planar", r_flow_type="Planar", head="identity")
    return net.to(dev).eval()


def _data(dev, n, B, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, DIMS[0], generator=g).to(dev), torch.randn(B, DIMS[-1], generator=g).to(dev)) for _ in range(n)]


@pytest.mark.parametrize("kind", ("lrt", "mnf"))
def test_evaluate_batches_equals_the_hand_rolled_loop(bnn, dev, kind):
    ev = bnn.evaluate
    S, B = 4, 70
    net = _net(bnn, dev, kind)
    lv = torch.tensor([-0.3, 0.4], device=dev)
    data = _data(dev, 3, B, 8)
    for model in (net, ev.freeze(net, "alpha"), ev.freeze(net, "mpm")):
        acc = ev.RegressionAccumulator(DIMS[-1], S, dev, lv)
        bnn.manual_seed(SEED)
        res = ev.evaluate_batches(model, data, S, acc=acc)
        rng_after = bnn.ops.RngState.get(dev).t.clone()
        hand = ev.RegressionAccumulator(DIMS[-1], S, dev, lv)
        bnn.manual_seed(SEED)
        with torch.no_grad():
            for x, y in data:
                o = model.ensemble(x, S) if ev._is_frozen(model) else ev.ensemble_forward(model, x, S)
                hand.update(o, y, model(x, sample=False))
        assert torch.equal(acc._totals, hand._totals) and torch.equal(rng_after, bnn.ops.RngState.get(dev).t)
        assert res["elements"] == 3 * B * DIMS[-1] == res["scored_elements"] and res["rmse_posterior_mean"] is not None
        assert res["rmse"] == hand.result()["rmse"] and int(res["pit_hist"].sum()) == res["scored_elements"]
        no_mean = ev.RegressionAccumulator(DIMS[-1], S, dev, lv)
        assert ev.evaluate_batches(model, data, S, acc=no_mean, posterior_mean=False)["rmse_posterior_mean"] is None
    with pytest.raises(ValueError, match="RegressionAccumulator"):
        ev.evaluate_batches(net, data, S)
    with pytest.raises(ValueError, match="RegressionAccumulator"):
        ev.ensemble_eval(net, data[0][0], None, S)


@pytest.mark.parametrize("kind", ("lrt", "mnf"))
def test_graphed_eval_step_equals_eager_updates_bitwise(bnn, dev, kind):
    ev = bnn.evaluate
    S, B, O = 10, 100, DIMS[-1]
    fz = ev.freeze(_net(bnn, dev, kind), "mpm")
    lv = torch.tensor([-0.3, 0.4], device=dev)
    data = _data(dev, 3, B, 4)
    acc_g = ev.RegressionAccumulator(O, S, dev, lv)
    bnn.manual_seed(SEED)
    acc_g.update(fz.ensemble(data[0][0], S), data[0][1])                          # totals that must survive the build
    st = bnn.ops.RngState.get(dev)
    before, rng_before = acc_g._totals.clone(), st.t.clone()
    step = bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], S, acc_g)
    assert torch.equal(acc_g._totals, before) and torch.equal(st.t, rng_before)
    assert (acc_g.updates, acc_g.posterior_mean_updates) == (1, 0)
    acc_g.reset()
    bnn.manual_seed(SEED)
    got = [{k: v.clone() for k, v in step(x, y).items()} for x, y in data]
    rng_g = st.t.clone()
    acc_e = ev.RegressionAccumulator(O, S, dev, lv)
    bnn.manual_seed(SEED)
    for (x, y), rows_g in zip(data, got):
        rows_e = acc_e.update(fz.ensemble(x, S), y, fz(x, sample=False))
        assert sorted(rows_e) == sorted(rows_g)
        for k in rows_e:
            assert _same(rows_e[k], rows_g[k]), k
    assert torch.equal(acc_g._totals, acc_e._totals)
    assert torch.equal(rng_g, st.t)                                               # the Philox offset advanced as the eager calls do
    assert (acc_g.updates, acc_g.posterior_mean_updates) == (3, 3) and acc_g.result()["elements"] == 3 * B * O
    with pytest.raises(ValueError, match="RegressionAccumulator"):
        bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], S, ev.EvalAccumulator(2, S, dev))
    with pytest.raises(ValueError, match="uncertainty"):
        bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], S, acc_g, uncertainty=ev.UncertaintyAccumulator(2, S, dev))
