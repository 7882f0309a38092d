"""GPU tier of the frozen evaluation model (evaluate.freeze / FrozenNetwork; include/lbbnn.h lbbnn_frozen_operands +
lbbnn_frozen_members): the alpha model equals the live network's ensemble from the same Philox offset, the median
probability model equals (a) the existing kernels on a copy whose fp32 alpha is exactly 0 / 1 and (b) the fp64 oracle on the
regenerated draws; kept_rows / density / e0 are exact; chunking changes no bit; the snapshot is a snapshot; every operand
byte the GEMMs read was written; ensemble_eval / predictive_entropy take a frozen model.

Bars (tests/test_parity_gpu.py): TOL = 1e-4 the contract, TIGHT = 5e-6 for fp32 outputs, 2e-5 for bf16x3, as rel_err; the
element-wise form |out - ref| <= 1e-6 max|ref| + 1e-4 |ref|.

mpm inputs: lambdal = seeded U(-3, 3) pushed at least 1e-3 away from the cut, then row 0 and column 0 of every layer set
to -2.  Before anything is compared ``_mpm_inputs`` asserts per layer 0 < kept < O * I and, at threshold 0.5 for layers of
at least 192 weights, 0.25 <= density <= 0.6 (computed from lambdal in torch, not by the code under test)."""
import copy

import pytest
import torch

from conftest import elementwise_violation, rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4
TIGHT = 5e-6
BAR = {"fp32": TIGHT, "bf16x3": 2e-5}

# (family, dims, planar transforms)
NETS = [("lrt", (784, 400, 600, 10), 0), ("mnf", (784, 400, 600, 10), 2), ("lrt", (20, 16, 12, 3), 0),
        ("mnf", (20, 16, 12, 3), 4), ("lrt", (64, 48, 40, 20), 0), ("mnf", (64, 48, 40, 20), 2),
        ("lrt", (2048, 64, 32, 10), 0), ("mnf", (2048, 64, 32, 10), 4),
        ("lrt", (50, 37, 29, 3), 0)]                 # in_features % 4 != 0: outside the member GEMM's rule (chain of single GEMMs)
IDS = ["%s-%s%s" % (f, "-".join(map(str, d)), "-T%d" % t if t else "") for f, d, t in NETS]
BS = [(1, 10), (100, 10), (257, 1), (100, 1), (1, 1), (257, 10)]
SEED, OFF = 3, 5


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


def _layers(net):
    return [net.l1, net.l2, net.l3]


def _net(bnn, dev, family, dims, T, seed=11):
    torch.manual_seed(seed)
    if family == "lrt":
        net = bnn.lrt.BayesianNetwork(dims)
    else:
        net = bnn.mnf.BayesianNetwork(dims, T, z_flow_type="Planar", r_flow_type="Planar")
    return net.to(dev).eval()


def _cut(threshold):
    return float(torch.logit(torch.tensor(threshold, dtype=torch.float64)).float())


def _mpm_inputs(net, threshold=0.5, seed=7):
    """Overwrite lambdal as the module docstring says and assert the conditions on these inputs; returns the kept masks."""
    cut = _cut(threshold)
    g = torch.Generator().manual_seed(seed)
    masks = []
    for l in _layers(net):
        O, I = l.out_features, l.in_features
        lam = torch.empty(O, I).uniform_(-3, 3, generator=g)
        d = lam - cut
        lam = torch.where(d.abs() < 2e-3, cut + torch.where(d < 0, -2e-3, 2e-3), lam)
        lam[0, :] = -2.0
        lam[:, 0] = -2.0
        assert float((lam - cut).abs().min()) >= 1e-3
        with torch.no_grad():
            l.lambdal.copy_(lam)
        keep = lam > cut
        kept = int(keep.sum())
        assert 0 < kept < O * I, (O, I, kept)
        if threshold == 0.5:
            assert not keep[0].any() and not keep[:, 0].any()            # the fully pruned row and column
            if O * I >= 192:
                assert 0.25 <= kept / (O * I) <= 0.6, (O, I, kept / (O * I))
        masks.append(keep)
    return masks


def _x(dev, B, I, seed=1):
    return torch.rand(B, I, generator=torch.Generator().manual_seed(seed + B)).to(dev)


def _pinned_copy(net, masks, value):
    """A copy of the network whose lambdal is +value where the weight is kept and -value elsewhere."""
    c = copy.deepcopy(net)
    with torch.no_grad():
        for l, keep in zip(_layers(c), masks):
            l.lambdal.copy_(torch.where(keep, value, -value).to(l.lambdal.device))
    return c


# --------------------------------------------------------------------------- 1. alpha model against the live network
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("family,dims,T", NETS, ids=IDS)
def test_alpha_model_equals_live_ensemble(bnn, dev, precision, family, dims, T, prec):
    """Same draws, so the difference is operand rounding only.  (Measured: bitwise equal for every case here -- the kernel
    shares K1's device functions -- but the assertion is the bar.)"""
    ev = bnn.evaluate
    net = _net(bnn, dev, family, dims, T)
    with torch.no_grad():
        for l in _layers(net):
            l.lambdal.uniform_(-3, 3)                 # gates that vary (the default init has every alpha in (0.5, 0.73))
    precision(prec)
    fz = ev.freeze(net)
    assert fz.gates == "alpha" and fz.dims == tuple(dims) and list(fz.parameters()) == []
    st = bnn.ops.RngState.get(dev)
    for B, S in BS:
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        ref = ev.ensemble_forward(net, x, S)
        assert int(st.t[1]) == OFF + S
        bnn.manual_seed(SEED, OFF)
        out = fz.ensemble(x, S)
        assert int(st.t[1]) == OFF + S
        assert out.shape == ref.shape == (S, B, dims[-1])
        e = rel_err(out, ref)
        print("alpha-vs-live %s %s B=%d S=%d rel_err %.3g bitwise %s" % (family, dims, B, S, e, torch.equal(out, ref)))
        assert e < BAR[prec], (B, S, e)
        # ... and the posterior-mean branch against the live network's
        bnn.manual_seed(SEED, OFF)
        with torch.no_grad():
            ref0 = net(x, sample=False)
        bnn.manual_seed(SEED, OFF)
        out0 = fz(x, sample=False)
        assert out0.shape == (B, dims[-1]) and rel_err(out0, ref0) < BAR[prec]


# --------------------------------------------------------------------------- 2. mpm model through the existing kernels
@pytest.mark.parametrize("threshold", [0.5, 0.1])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("family,dims,T", NETS, ids=IDS)
def test_mpm_model_equals_existing_kernels_on_pinned_gates(bnn, dev, precision, family, dims, T, prec, threshold):
    ev = bnn.evaluate
    net = _net(bnn, dev, family, dims, T)
    masks = _mpm_inputs(net, threshold)
    pinned = _pinned_copy(net, masks, 200.0)
    for l in _layers(pinned):
        a = torch.sigmoid(l.lambdal.detach())
        assert bool(((a == 0) | (a == 1)).all())      # fp32 alpha exactly 0 / 1 (also as rcp(1 + exp2(.)): exp gives inf / 0)
    precision(prec)
    fz = ev.freeze(net, "mpm", threshold=threshold)
    for B, S in BS:
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        ref = ev.ensemble_forward(pinned, x, S)
        bnn.manual_seed(SEED, OFF)
        out = fz.ensemble(x, S)
        e = rel_err(out, ref)
        print("mpm-vs-pinned %s %s B=%d S=%d rel_err %.3g" % (family, dims, B, S, e))
        assert out.shape == (S, B, dims[-1]) and e < BAR[prec], (B, S, e)
        if S > 1:
            assert not torch.equal(out[0], out[1])


# --------------------------------------------------------------------------- 3. mpm model against fp64
def _oracle_member(bnn, fz, net, masks, x, m, stochastic, z_used):
    """Member m in float64: lambdal = +-1000 (fp64 alpha exactly 1 / 0), the z the member used, eps regenerated at the
    documented stream / offset / row offset through lbbnn_philox_normal."""
    ops, dev = bnn.ops, x.device
    rng_m = torch.tensor([SEED, OFF + m], dtype=torch.int64, device=dev)
    P, noise = [], []
    for i, (l, keep) in enumerate(zip(_layers(net), masks)):
        p = {k: getattr(l, k).detach().double().cpu() for k in ("weight_mu", "weight_rho", "bias_mu", "bias_rho")}
        p["lambdal"] = torch.where(keep, 1000.0, -1000.0).double()
        a = orc.alpha_of(p["lambdal"])
        assert bool(((a == 0) | (a == 1)).all())
        eps = ops.philox_normal(rng_m, ops.STREAM_EPS_OUT * 64 + l._layer_id, x.shape[0], l.out_features,
                                row_base=l.row_offset).double().cpu() if stochastic else None
        if fz.family == "mnf":
            p["q0_mean"] = z_used[i][m].double().cpu()                   # z0 = q0_mean + 0 * eps_z, no transforms: z itself
            p["q0_log_var"] = torch.full_like(p["q0_mean"], -float("inf"))
            noise.append({"eps_z": torch.zeros(1, l.in_features, dtype=torch.float64), "eps_out": eps})
        else:
            noise.append(eps)
        P.append(p)
    x64 = x.double().cpu()
    if fz.family == "mnf":
        ident = orc.Flow("Planar", [])
        out, _ = orc.mnf_network_forward(x64, P, [ident] * 3, [None] * 3, noise, stochastic=stochastic, compute_kl=False)
    else:
        out, _ = orc.lrt_network_forward(x64, P, noise, stochastic=stochastic, compute_kl=False)
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("family,dims,T", NETS, ids=IDS)
def test_mpm_model_against_fp64_oracle(bnn, dev, precision, family, dims, T, prec):
    ev = bnn.evaluate
    net = _net(bnn, dev, family, dims, T)
    masks = _mpm_inputs(net, 0.5)
    precision(prec)
    fz = ev.freeze(net, "mpm")
    for B, S in [(100, 10), (257, 1), (1, 10)]:
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        out = fz.ensemble(x, S, keep_z=True)
        z = fz.last_z
        if family == "mnf":
            assert [tuple(t.shape) for t in z] == [(S, I) for I in dims[:-1]]
            if S > 1:
                assert not torch.equal(z[0][0], z[0][1])
        else:
            assert z == [None] * 3
        for m in range(S):
            ref = _oracle_member(bnn, fz, net, masks, x, m, True, z)
            e, v = rel_err(out[m], ref), elementwise_violation(out[m], ref)
            if m == 0:
                print("mpm-vs-fp64 %s %s %s B=%d m=%d rel_err %.3g elementwise %.3g" % (family, dims, prec, B, m, e, v))
            assert e < TOL and v <= 1.0, (B, m, e, v)
    # sample=False against the oracle's stochastic=False branch (an MNF model still draws z: recover it as member 0's)
    x = _x(dev, 100, dims[0])
    bnn.manual_seed(SEED, OFF)
    fz.ensemble(x, 1, keep_z=True)
    z = fz.last_z
    bnn.manual_seed(SEED, OFF)
    out0 = fz(x, sample=False)
    ref0 = _oracle_member(bnn, fz, net, masks, x, 0, False, z)
    e, v = rel_err(out0, ref0), elementwise_violation(out0, ref0)
    print("mpm-mean-vs-fp64 %s %s %s rel_err %.3g elementwise %.3g" % (family, dims, prec, e, v))
    assert e < TOL and v <= 1.0, (e, v)


# --------------------------------------------------------------------------- 4. kept_rows, density, e0, tails
@pytest.mark.parametrize("gates", ["mpm", "alpha"])
@pytest.mark.parametrize("threshold", [0.5, 0.1, 0.9])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("family,dims,T", NETS, ids=IDS)
def test_kept_rows_density_and_e0_exact(bnn, dev, precision, family, dims, T, prec, threshold, gates):
    ev, ops = bnn.evaluate, bnn.ops
    net = _net(bnn, dev, family, dims, T)
    masks = _mpm_inputs(net, threshold)
    precision(prec)
    fz = ev.freeze(net, gates, threshold=threshold)
    assert fz.threshold == threshold and fz.gates == gates
    total = 0
    for i, (l, keep) in enumerate(zip(_layers(net), masks)):
        O, I = l.out_features, l.in_features
        cut = torch.tensor(_cut(threshold), dtype=torch.float32)
        rows = (l.lambdal.detach().cpu() > cut).sum(1)
        assert torch.equal(rows, keep.sum(1))
        assert fz.kept_rows[i].dtype == torch.int32 and torch.equal(fz.kept_rows[i].cpu().long(), rows)
        assert fz.kept[i] == int(rows.sum())
        total += int(rows.sum())
        e0 = getattr(fz, "e0_%d" % i).cpu()
        assert e0.shape == (O, ops.operand_ld(I))
        assert bool((e0[:, I:] == 0).all())                               # the zero tail
        mu = l.weight_mu.detach().cpu()
        if gates == "mpm":
            assert torch.equal(e0[:, :I][keep], mu[keep])                 # kept: weight_mu itself
            assert bool((e0[:, :I][~keep] == 0).all())                    # pruned: exactly 0.0
        else:
            assert rel_err(e0[:, :I], mu.double() * orc.alpha_of(l.lambdal.detach().double().cpu())) < TIGHT
        bias_var = getattr(fz, "bias_var_%d" % i)
        assert rel_err(bias_var, orc.sigma_of(l.bias_rho.detach().double().cpu()) ** 2) < TIGHT      # never gated
        if not fz._split[i]:
            e_w, var_w = getattr(fz, "e_w_%d" % i).cpu(), getattr(fz, "var_w_%d" % i).cpu()
            assert torch.equal(e_w, e0)
            s2 = orc.sigma_of(l.weight_rho.detach().double().cpu()) ** 2
            a = keep.double() if gates == "mpm" else orc.alpha_of(l.lambdal.detach().double().cpu())
            assert rel_err(var_w[:, :I], s2 * a ** 2) < TIGHT             # a^2, not a
            assert elementwise_violation(var_w[:, :I], s2 * a ** 2) <= 1.0
            assert bool((var_w[:, I:] == 0).all())
            if gates == "mpm":
                assert bool((var_w[:, :I][~keep] == 0).all())
    n_w = sum(dims[i] * dims[i + 1] for i in range(3))
    assert isinstance(fz.density, float) and fz.density == total / n_w


# --------------------------------------------------------------------------- 5. chunks, offsets, forward
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("family,dims,T", NETS, ids=IDS)
def test_chunks_offsets_and_single_forward(bnn, dev, precision, family, dims, T, prec):
    ev = bnn.evaluate
    net = _net(bnn, dev, family, dims, T)
    _mpm_inputs(net, 0.5)
    precision(prec)
    st = bnn.ops.RngState.get(dev)
    for gates in ("alpha", "mpm"):
        fz = ev.freeze(net, gates)
        for B, S in [(100, 10), (257, 10), (1, 10)]:
            x = _x(dev, B, dims[0])
            bnn.manual_seed(SEED, OFF)
            whole = fz.ensemble(x, S, keep_z=True)
            z_whole = fz.last_z
            assert int(st.t[1]) == OFF + S
            for mm in (1, 3):
                bnn.manual_seed(SEED, OFF)
                part = fz.ensemble(x, S, max_members=mm, keep_z=True)
                assert int(st.t[1]) == OFF + S
                assert torch.equal(part, whole), (gates, B, mm)
                for a, b in zip(fz.last_z, z_whole):
                    assert (a is None and b is None) or torch.equal(a, b)
                bnn.manual_seed(SEED, OFF)
                assert torch.equal(ev.ensemble_forward(fz, x, S, max_members=mm), whole)
            bnn.manual_seed(SEED, OFF)
            one = fz.ensemble(x, 1)
            assert torch.equal(one[0], whole[0])
            bnn.manual_seed(SEED, OFF)
            single = fz(x, sample=True)
            assert int(st.t[1]) == OFF + 1
            assert single.shape == (B, dims[-1]) and torch.equal(single, one[0])
            with pytest.raises(ValueError):
                ev.ensemble_forward(fz, x, S, gates="mpm")


# --------------------------------------------------------------------------- 6. snapshot semantics
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("family,dims,T", [NETS[0], NETS[1], NETS[3], NETS[8]], ids=[IDS[0], IDS[1], IDS[3], IDS[8]])
def test_snapshot_and_refresh(bnn, dev, precision, family, dims, T, prec):
    ev = bnn.evaluate
    net = _net(bnn, dev, family, dims, T)
    _mpm_inputs(net, 0.5)
    precision(prec)
    x = _x(dev, 100, dims[0])
    for gates in ("alpha", "mpm"):
        fz = ev.freeze(net, gates)
        ptrs = {k: v.data_ptr() for k, v in fz.named_buffers()}
        bnn.manual_seed(SEED, OFF)
        before = fz.ensemble(x, 3)
        kept_before = fz.kept
        with torch.no_grad():
            for l in _layers(net):
                l.weight_mu.mul_(1.5).add_(0.01)
                l.bias_mu.add_(0.25)
                l.lambdal.neg_()
                if family == "mnf":
                    l.q0_mean.add_(0.5)
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(fz.ensemble(x, 3), before)                     # the frozen model did not follow
        assert fz.kept == kept_before
        assert fz.refresh() is fz
        assert {k: v.data_ptr() for k, v in fz.named_buffers()} == ptrs   # into the same buffers
        bnn.manual_seed(SEED, OFF)
        after = fz.ensemble(x, 3)
        assert not torch.equal(after, before)
        fresh = ev.freeze(net, gates)
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(fresh.ensemble(x, 3), after)
        assert fresh.kept == fz.kept and fz.kept != kept_before


# --------------------------------------------------------------------------- 7. every operand byte was written
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("family,dims,T", NETS, ids=IDS)
def test_nan_filled_buffers(bnn, dev, precision, monkeypatch, family, dims, T, prec):
    """Every buffer of the frozen model (operands, member operands, z, hidden activations, outputs) is handed out full of
    NaN: a byte the kernels read without having written it (an operand tail, a member's row) would surface in the outputs."""
    ev = bnn.evaluate
    net = _net(bnn, dev, family, dims, T)
    _mpm_inputs(net, 0.5)
    precision(prec)
    x = _x(dev, 100, dims[0])
    clean = {}
    for gates in ("alpha", "mpm"):
        bnn.manual_seed(SEED, OFF)
        clean[gates] = ev.freeze(net, gates).ensemble(x, 3, max_members=2)

    def nan_empty(*size, **kw):
        return torch.full(*size, float("nan"), **kw)
    monkeypatch.setattr(ev, "_empty", nan_empty)
    for gates in ("alpha", "mpm"):
        fz = ev.freeze(net, gates)
        for i in range(3):
            for name in ("e0", "e_w", "var_w", "bias_var", "bias_mu"):
                assert bool(torch.isfinite(getattr(fz, "%s_%d" % (name, i))).all()), (name, i)
        bnn.manual_seed(SEED, OFF)
        out = fz.ensemble(x, 3, max_members=2)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out, clean[gates])
        assert bool(torch.isfinite(fz(x, sample=False)).all())


# --------------------------------------------------------------------------- 8. ensemble_eval / predictive_entropy
@pytest.mark.parametrize("family,dims,T", [NETS[0], NETS[1], NETS[5], NETS[8]], ids=[IDS[0], IDS[1], IDS[5], IDS[8]])
def test_ensemble_eval_and_entropy(bnn, dev, family, dims, T):
    ev = bnn.evaluate
    net = _net(bnn, dev, family, dims, T)
    _mpm_inputs(net, 0.5)
    fz = ev.freeze(net, "mpm")
    B, S, C = 100, 10, dims[-1]
    x = _x(dev, B, dims[0])
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(2)).to(dev)
    bnn.manual_seed(SEED, OFF)
    r = ev.ensemble_eval(fz, x, y, S)
    assert set(r) == {"outputs", "pred_ensemble", "pred_posterior_mean", "density", "correct_ensemble",
                      "correct_posterior_mean"}
    assert r["outputs"].shape == (S, B, C) and r["pred_ensemble"].shape == (B,) and r["pred_posterior_mean"].shape == (B,)
    assert r["density"].shape == (S,) and bool((r["density"] == torch.tensor(fz.density, dtype=torch.float32)).all())
    assert torch.equal(r["pred_ensemble"], r["outputs"].mean(0).argmax(1))
    assert r["correct_ensemble"] == int((r["pred_ensemble"] == y).sum())
    assert r["correct_posterior_mean"] == int((r["pred_posterior_mean"] == y).sum())
    assert rel_err(r["outputs"].exp().sum(-1), torch.ones(S, B)) < 1e-5      # log-probabilities
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(fz.ensemble(x, S), r["outputs"])
    assert set(ev.ensemble_eval(fz, x, None, 2)) == {"outputs", "pred_ensemble", "pred_posterior_mean", "density"}
    h = ev.predictive_entropy(r["outputs"])
    p = torch.sigmoid(r["outputs"].double())
    p = (p / p.sum(-1, keepdim=True)).mean(0)
    assert h.shape == (B,) and rel_err(h, -(p * p.log()).sum(-1)) < 1e-5
