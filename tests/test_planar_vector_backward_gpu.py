"""GPU tier: the vector-sized backward of a planar MNF layer (csrc/vector_bwd.hip) called directly, in all three forms of V2
and through both of its kernels, against float64 autograd of the objective it differentiates (tests/planar_vector_ref.py).

Bars (planar_vector_ref.check_leaves), set before any kernel was run:
  vector leaf       max-norm < 5e-5 (the bar test_planar_backward_all_hip_vs_oracle_autograd holds these gradients to) AND
                    element-wise |got - ref| <= 1e-4 |ref| + A_ELEM max|ref|, A_ELEM = 1.1e-5 = three times the worst
                    remainder the float32 reference itself shows over the table (3.6e-6)
  one-element leaf  (flow-bias gradients, everything at I = 1: sums that cancel) max(5e-5, 4 E32) of the value, E32 = the
                    error of the float32 reference on that leaf and those inputs; at most 1 % of them above 5e-5 and none
                    above 1e-3 (test_one_element_bars_stay_narrow; the host tier asserts the same over seeds 0-5)
  exact zeros       a leaf whose reference is exactly zero must be exactly zero
Measured on an MI355X when this was written (every test prints its figures): vector leaves 9.3e-6 max-norm at most
((2500, 3, 16, 16) without the KL branch; 5.5e-6 in the register form), element-wise remainder 1.6e-6 at most, one-element
leaves at most 0.27 of their bar; V1 2.2e-7.  Three arithmetic slips put into a scratch build (the chain's w gradient
reading z one transform late; the register form taking the r flow's last u from the z flow; 3e-4 on the gv_sum term of
the chain's bias loop) each failed every case of section a that runs the line.
Every output buffer is filled with NaN before the call (the ``poison`` fixture), so an element a kernel does not write
cannot pass on what an earlier call left in the same memory.

Cases run per form (section a, each with and without the KL branch): register 10, LDS chain 6 (4 through the single-entry
kernel, 2 through the batch kernel), global-work chain 3 (1 single-entry, 2 batch); the other sections add argument
variants, in-kernel draws, mixed groups, the rc == -2 path and the order in which the dynamic-LDS attribute is raised."""
import pytest
import torch

import planar_vector_ref as pv
from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture
def poison(monkeypatch):
    """torch.empty / empty_like on the GPU hand out NaN-filled float buffers while a test runs."""
    real_empty, real_like = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(float("nan")) if t.is_cuda and t.is_floating_point() else t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(real_like(*a, **k)))


def _case_id(c):
    return "%s-%s" % (c[0], "x".join(str(v) for v in c[1:5])) + ("-batch" if c[5] == "batch" else "")


def _params(dd, fl, T):
    return [(dd["%s.%d.u" % (fl, t)], dd["%s.%d.w" % (fl, t)], dd["%s.%d.b" % (fl, t)]) for t in range(T)]


def _call_v2(ops, dd, Tz, Tr, has_kl, variant=pv.FULL, explicit=True, rng=None, layer_id=0, defer=None):
    v = dict(variant)
    return ops.mnf_flow_planar_backward(
        dd["q0_mean"], dd["q0_log_var"], _params(dd, "z_flow", Tz), _params(dd, "r_flow", Tr),
        eps_fwd=dd["eps_fwd"] if explicit else None, eps_kl=dd["eps_kl"] if explicit and has_kl else None,
        r0_b1=dd["r0_b1"], r0_b2=dd["r0_b2"], aux=dd["aux"] if has_kl else None,
        dz_fwd=dd["dz_fwd"] if v["dz_fwd"] else None, dz_kl=dd["dz_kl"] if has_kl and v["dz_kl"] else None,
        g_kl=dd["g_kl"] if has_kl else None, bias_mu=dd["bias_mu"], bias_rho=dd["bias_rho"], g_sum=dd["g_sum"],
        gv_sum=dd["gv_sum"] if v["gv_sum"] else None, priors=ops.Priors(), rng=rng, layer_id=layer_id, defer=defer)


def _flat(out):
    """The dict of ops.mnf_flow_planar_backward under the leaf names of the reference, on the CPU."""
    r = {k: out[k].cpu() for k in ("q0_mean", "q0_log_var", "r0_b1", "r0_b2", "bias_mu", "bias_rho")}
    for fl in ("z_flow", "r_flow"):
        for t, g3 in enumerate(out[fl]):
            for k, g in zip(("u", "w", "b"), g3):
                r["%s.%d.%s" % (fl, t, k)] = g.cpu()
    return r


def _on(dev, I, O, Tz, Tr, seed):
    return {k: v.to(dev) for k, v in pv.make_inputs(I, O, Tz, Tr, seed).items()}


def _report(tag, tally):
    vec, sc = tally.get("vector", []), tally.get("scalar", [])
    print("%s: vector max-norm %.3g remainder %.3g | one-element worst err/bar %.3g (%d leaves)" % (
        tag, max([v[0] for v in vec] + [0.0]), max([v[1] for v in vec] + [0.0]),
        max([s[1] / s[0] for s in sc] + [0.0]), len(sc)))


def _check(got, I, O, Tz, Tr, seed, has_kl, tag, variant=pv.FULL):
    r64, r32 = pv.references(I, O, Tz, Tr, seed, has_kl, variant)
    assert sorted(got) == sorted(r64)
    tally = {}
    bad = pv.check_leaves(got, r64, r32, pv.A_ELEM, tag, tally)
    _report(tag, tally)
    assert not bad, "\n".join(bad)


def _run(ops, dev, I, O, Tz, Tr, seed, has_kl, route, **kw):
    dd = _on(dev, I, O, Tz, Tr, seed)
    if route == "batch":
        pending = []
        out = _call_v2(ops, dd, Tz, Tr, has_kl, defer=pending, **kw)
        assert len(pending) == 1
        ops.mnf_flow_planar_backward_flush(pending)
    else:
        out = _call_v2(ops, dd, Tz, Tr, has_kl, **kw)
    return _flat(out)


# --------------------------------------------------------------------------- a. every table case against float64
@pytest.mark.parametrize("has_kl", [True, False], ids=["kl", "nokl"])
@pytest.mark.parametrize("case", pv.ALL_CASES, ids=_case_id)
def test_v2_every_form_against_float64(bnn, dev, poison, case, has_kl):
    f, I, O, Tz, Tr, route = case
    assert pv.form(I, Tz, Tr) == f
    got = _run(bnn.ops, dev, I, O, Tz, Tr, 0, has_kl, route)
    _check(got, I, O, Tz, Tr, 0, has_kl, _case_id(case))


def test_one_element_bars_stay_narrow():
    """The bars of the one-element leaves of section a, from the reference alone: at most 1 % above the floor, none above
    the ceiling."""
    bars = []
    for f, I, O, Tz, Tr, _ in pv.ALL_CASES:
        for has_kl in (True, False):
            r64, r32 = pv.references(I, O, Tz, Tr, 0, has_kl)
            bars += [pv.scalar_bar(r32[k], v) for k, v in r64.items() if v.numel() == 1 and float(v.abs().max()) != 0.0]
    wide = [b for b in bars if b > pv.SCALAR_FLOOR]
    print("one-element leaves %d, bars above the floor: %r" % (len(bars), wide))
    assert len(bars) >= 200
    assert len(wide) <= pv.SCALAR_WIDE_FRAC * len(bars) and max(bars) <= pv.SCALAR_CEIL


# --------------------------------------------------------------------------- b. argument variants
VARIANT_CASES = [("reg", 2047, 5, 2, 2), ("lds", 1025, 3, 5, 1), ("global", 4097, 3, 1, 1)]       # all single-entry calls


@pytest.mark.parametrize("off", ["dz_fwd", "dz_kl", "gv_sum"])
@pytest.mark.parametrize("f,I,O,Tz,Tr", VARIANT_CASES, ids=[c[0] for c in VARIANT_CASES])
def test_v2_optional_arguments_left_out(bnn, dev, poison, f, I, O, Tz, Tr, off):
    assert pv.form(I, Tz, Tr) == f
    variant = tuple((k, k != off) for k, _ in pv.FULL)
    assert variant in pv.VARIANTS
    for has_kl in ((True,) if off == "dz_kl" else (True, False)):
        assert (has_kl, variant) in pv.CONFIGS
        got = _run(bnn.ops, dev, I, O, Tz, Tr, 1, has_kl, "single", variant=variant)
        _check(got, I, O, Tz, Tr, 1, has_kl, "%s no %s kl=%d" % (f, off, has_kl), variant)


# --------------------------------------------------------------------------- c. in-kernel draws
@pytest.mark.parametrize("L", [0, 3, 15])
@pytest.mark.parametrize("f,I,O,Tz,Tr,route", [("reg", 1025, 1200, 1, 4, "single"), ("lds", 100, 3, 5, 2, "single"),
                                                ("global", 4097, 3, 1, 1, "batch")], ids=["reg", "lds", "global"])
def test_v2_in_kernel_draws_equal_the_same_draws_handed_in(bnn, dev, poison, f, I, O, Tz, Tr, route, L):
    ops = bnn.ops
    assert pv.form(I, Tz, Tr) == f
    bnn.manual_seed(1234, 7)
    snap = ops.RngState.get(dev).t.clone()
    dd = _on(dev, I, O, Tz, Tr, 2)
    dd["eps_fwd"] = ops.philox_normal(snap, ops.STREAM_EPS_Z * 64 + L, 0, I)
    dd["eps_kl"] = ops.philox_normal(snap, ops.STREAM_EPS_Z2 * 64 + L, 0, I)
    assert dd["eps_fwd"].shape == (I,) and not torch.equal(dd["eps_fwd"], dd["eps_kl"])
    assert 0.5 < float(dd["eps_fwd"].std()) < 1.5 and 0.5 < float(dd["eps_kl"].std()) < 1.5
    if L:
        assert not torch.equal(dd["eps_fwd"], ops.philox_normal(snap, ops.STREAM_EPS_Z * 64, 0, I))
    for has_kl in (True, False):
        outs = []
        for explicit in (True, False):
            pending = [] if route == "batch" else None
            out = _call_v2(ops, dd, Tz, Tr, has_kl, explicit=explicit, rng=None if explicit else snap, layer_id=L,
                           defer=pending)
            if pending is not None:
                ops.mnf_flow_planar_backward_flush(pending)
            outs.append(_flat(out))
        for k, ref in outs[0].items():
            assert bool(torch.isfinite(ref).all()), k
            if float(ref.abs().max()) == 0.0:
                assert float(outs[1][k].abs().max()) == 0.0, k
            else:
                assert rel_err(outs[1][k], ref) < 1e-6, (k, has_kl)


@pytest.mark.parametrize("L", [0, 3, 15])
def test_v1_in_kernel_draws_equal_the_same_draws_handed_in(bnn, dev, poison, L):
    ops = bnn.ops
    O, I = 1200, 784
    bnn.manual_seed(4321, 3)
    snap = ops.RngState.get(dev).t.clone()
    d = {k: v.to(dev) for k, v in pv.make_v1_inputs(O, I, 2).items()}
    eps = ops.philox_normal(snap, ops.STREAM_EPS_ACT * 64 + L, 0, O)
    assert 0.5 < float(eps.std()) < 1.5
    a = ops.mnf_aux_backward(d["act_mu"], d["act_var"], eps, d["r0_b1"], d["r0_b2"], d["zb_last"], d["g_kl"])
    b = ops.mnf_aux_backward(d["act_mu"], d["act_var"], None, d["r0_b1"], d["r0_b2"], d["zb_last"], d["g_kl"], rng=snap,
                             layer_id=L)
    for x, y, n in zip(a, b, ("da_mu", "da_var", "aux")):
        x, y = (x[:1], y[:1]) if n == "aux" else (x, y)
        assert bool(torch.isfinite(x).all()) and rel_err(y, x) < 1e-6, n


# --------------------------------------------------------------------------- d. batching
REG_A, REG_B = (5, 7, 3, 3), (1025, 1200, 1, 4)
LDS_B, LDS_TOP = (2049, 3, 1, 1), (4096, 3, 1, 1)
GLB_A, GLB_B = (4097, 3, 1, 1), (2049, 3, 4, 4)
GROUPS = [[LDS_B], [REG_A, GLB_A], [REG_B, LDS_B, GLB_B], [REG_A, LDS_TOP, GLB_A, REG_B],
          [REG_A, LDS_B, GLB_A, REG_B, GLB_B, LDS_TOP]]                   # the last one: two launches (4 + 2)


@pytest.fixture
def batch_calls(monkeypatch):
    """[(n, rc)] of every lbbnn_mnf_flow_planar_backward_batch call and the count of single-entry calls."""
    from bnn_amd import _lib
    lib = _lib.lib()
    log = {"batch": [], "single": 0}
    real_b, real_s = lib.lbbnn_mnf_flow_planar_backward_batch, lib.lbbnn_mnf_flow_planar_backward

    def batch(arr, n, stream):
        rc = real_b(arr, n, stream)
        log["batch"].append((n, rc))
        return rc

    def single(a, stream):
        log["single"] += 1
        return real_s(a, stream)

    monkeypatch.setattr(lib, "lbbnn_mnf_flow_planar_backward_batch", batch)
    monkeypatch.setattr(lib, "lbbnn_mnf_flow_planar_backward", single)
    return log


@pytest.mark.parametrize("group", GROUPS, ids=[str(len(g)) for g in GROUPS])
def test_v2_mixed_groups_through_the_batch_kernel(bnn, dev, poison, batch_calls, group):
    """reg + LDS-chain + global-chain layers in one launch.  A register-form layer is bitwise what its single call gives
    (the source promises it: the single entry point takes the same kernel with n = 1).  The chain layers are held to the
    float64 bars; they were bitwise equal to their single-entry-kernel results too when this was written (the report line
    says so on every run), which the source does not promise."""
    ops = bnn.ops
    pending, outs, dds = [], [], []
    for k, (I, O, Tz, Tr) in enumerate(group):
        dds.append(_on(dev, I, O, Tz, Tr, 3))
        outs.append(_call_v2(ops, dds[-1], Tz, Tr, True, defer=pending))
    assert len(pending) == len(group) and batch_calls["batch"] == []
    ops.mnf_flow_planar_backward_flush(pending)
    assert pending == []
    assert batch_calls["batch"] == [(min(4, len(group) - i), 0) for i in range(0, len(group), 4)]
    assert batch_calls["single"] == 0
    for (I, O, Tz, Tr), out, dd in zip(group, outs, dds):
        f, got = pv.form(I, Tz, Tr), _flat(out)
        alone = _flat(_call_v2(ops, dd, Tz, Tr, True))
        same = all(torch.equal(got[k], alone[k]) for k in got)
        print("%s %r: batched == single call bitwise: %s" % (f, (I, O, Tz, Tr), same))
        if f == "reg":
            assert same, (I, O, Tz, Tr)
        _check(got, I, O, Tz, Tr, 3, True, "group of %d, %s %r" % (len(group), f, (I, O, Tz, Tr)))


def test_v2_group_with_a_long_flow_falls_back_to_single_calls(bnn, dev, poison, batch_calls):
    """A flow of five transforms does not fit the batch kernel's argument block: the batch call returns LBBNN_E_SHAPE
    before launching and the flush issues every layer of that group alone."""
    ops = bnn.ops
    group = [(100, 3, 5, 2), REG_A, LDS_B, GLB_A]
    pending, outs = [], []
    for I, O, Tz, Tr in group:
        outs.append(_call_v2(ops, _on(dev, I, O, Tz, Tr, 4), Tz, Tr, True, defer=pending))
    ops.mnf_flow_planar_backward_flush(pending)
    assert batch_calls["batch"] == [(4, -2)]
    assert batch_calls["single"] == 4                # (the register-form one re-enters the batch entry with n = 1, unseen here)
    for (I, O, Tz, Tr), out in zip(group, outs):
        _check(_flat(out), I, O, Tz, Tr, 4, True, "rc == -2 group, %r" % ((I, O, Tz, Tr),))


@pytest.mark.parametrize("route,small,large", [("single", (1025, 3, 5, 1), LDS_TOP), ("batch", LDS_B, LDS_TOP)])
def test_v2_dynamic_lds_is_raised_in_either_order(bnn, dev, poison, route, small, large):
    """Both LDS sizes are above 64 KiB, so each kernel raises its dynamic-LDS attribute once per new maximum: the largest
    workspace after a smaller one and a smaller one after the largest, whatever ran in this process before."""
    for shape in (small, large, small, large):
        I, O, Tz, Tr = shape
        assert pv.form(I, Tz, Tr) == "lds" and 4 * pv.workspace_floats(I, Tz, Tr) > pv.LDS_RAISE
        got = _run(bnn.ops, dev, I, O, Tz, Tr, 5, True, route)
        _check(got, I, O, Tz, Tr, 5, True, "%s %r" % (route, shape))


# --------------------------------------------------------------------------- e. V1
def _v1(ops, d, **kw):
    da_mu, da_var, aux = ops.mnf_aux_backward(d["act_mu"], d["act_var"], d["eps_act"], d["r0_b1"], d["r0_b2"], d["zb_last"],
                                              d["g_kl"], **kw)
    return {"da_mu": da_mu.cpu(), "da_var": da_var.cpu(), "aux0": aux[:1].cpu()}


@pytest.mark.parametrize("O,I", pv.V1_CASES)
def test_v1_against_float64(bnn, dev, poison, O, I):
    d = pv.make_v1_inputs(O, I, 0)
    got = _v1(bnn.ops, {k: v.to(dev) for k, v in d.items()})
    tally = {}
    bad = pv.check_leaves(got, pv.v1_reference(d), pv.v1_reference(d, torch.float32), pv.A_ELEM, "V1 %r" % ((O, I),), tally)
    _report("V1 %r" % ((O, I),), tally)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_v1_batch_is_bitwise_the_single_calls(bnn, dev, poison, n):
    ops = bnn.ops
    items = []
    for k in range(n):
        O, I = pv.V1_CASES[k]
        d = {key: v.to(dev) for key, v in pv.make_v1_inputs(O, I, 1 + k).items()}
        d["zb_last"] = torch.full((1,), 1.0 + 0.1 * k, device=dev)
        items.append(dict(d, rng=None, layer_id=k))
    g_kl = items[0]["g_kl"]
    outs = ops.mnf_aux_backward_batch(items, g_kl)
    assert len(outs) == n
    for it, (da_mu, da_var, aux) in zip(items, outs):
        alone = _v1(ops, dict(it, g_kl=g_kl), layer_id=it["layer_id"])
        assert bool(torch.isfinite(da_mu).all()) and bool(torch.isfinite(da_var).all())
        assert torch.equal(da_mu.cpu(), alone["da_mu"]) and torch.equal(da_var.cpu(), alone["da_var"])
        assert torch.equal(aux[:1].cpu(), alone["aux0"])


# --------------------------------------------------------------------------- f. layer level
def _oracle_grads(p, noise, x, wgt, T, train, dtype):
    """(out, x.grad, {parameter: grad}) of the oracle's MNF layer under autograd in ``dtype``."""
    from oracle import lbbnn_oracle as orc
    pc = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    xc = x.detach().to(dtype).clone().requires_grad_(True)
    zf = orc.flow_from_state("z_flow", "Planar", pc, T)
    rf = orc.flow_from_state("r_flow", "Planar", pc, T)
    o, kl, _ = orc.mnf_forward(xc, pc, zf, rf, {k: v.to(dtype) for k, v in noise.items()}, stochastic=True, compute_kl=train)
    ((o * wgt.to(dtype)).sum() + (kl / 60 if train else 0)).backward()
    return o.detach(), xc.grad, {k: v.grad for k, v in pc.items()}


_LAYER_SEED = {}


def _layer_seed(bnn, B, I, O, T):
    """Seed of _mnf_planar_case for this shape: B + I + O as in test_planar_backward_all_hip_vs_oracle_autograd, or the
    first of B + I + O + 1000 k at which the oracle in float32 holds E32_VEC on every parameter gradient, in training and
    in evaluation mode -- the conditioning rule of planar_vector_ref, from the reference alone.  (At (8, 4097, 4, 1),
    seed 4109, evaluation mode, the float32 oracle itself is 1.96e-4 off on the flow-bias gradient, a sum of 4097 products
    that cancels, and the kernels 1.09e-4 on the w gradient that carries it; seed 6109 is the first kept there, 3069 at
    (8, 2049, 12, 4) where 2069 gives 2.1e-5 for both.)"""
    import test_parity_gpu as tp
    key = (B, I, O, T)
    if key not in _LAYER_SEED:
        wgt = torch.randn(B, O, generator=torch.Generator().manual_seed(5))
        for k in range(16):
            seed = B + I + O + 1000 * k
            _, p, noise, x = tp._mnf_planar_case(bnn, "cpu", B, I, O, T, seed=seed)
            worst = 0.0
            for train in (True, False):
                g64 = _oracle_grads(p, noise, x, wgt, T, train, torch.float64)[2]
                g32 = _oracle_grads(p, noise, x, wgt, T, train, torch.float32)[2]
                worst = max([worst] + [rel_err(g32[n], g) for n, g in g64.items() if g is not None and float(g.abs().max())])
            if worst <= pv.E32_VEC:
                _LAYER_SEED[key] = seed
                break
        else:
            raise RuntimeError("no well-conditioned draw at %r" % (key,))
    return _LAYER_SEED[key]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,I,O,T", [(8, 100, 12, 5), (8, 2049, 12, 4), (8, 4097, 4, 1)])
def test_layer_backward_in_the_chain_forms_vs_oracle_autograd(bnn, dev, B, I, O, T, train):
    """bnn.mnf.BayesianLinear with planar flows whose V2 takes the LDS chain (T = 5), the global-work chain (2049, T = 4)
    and the global-work chain beyond the LDS limit (4097, T = 1): the recipe and the bars of
    test_planar_backward_all_hip_vs_oracle_autograd."""
    import test_parity_gpu as tp
    assert pv.form(I, T, T) == ("lds" if T == 5 else "global")
    layer, p, noise, x = tp._mnf_planar_case(bnn, dev, B, I, O, T, seed=_layer_seed(bnn, B, I, O, T))
    layer.train(train)
    layer.noise = {k: v.to(dev) for k, v in noise.items() if train or k in ("eps_z", "eps_out")}
    xg = x.to(dev).requires_grad_(True)
    out = layer(xg, sample=True)
    wgt = torch.randn(B, O, generator=torch.Generator().manual_seed(5))
    loss = (out * wgt.to(dev)).sum() + (layer.kl / 60 if train else 0)
    loss.backward()
    o, xgrad, ref = _oracle_grads(p, noise, x, wgt, T, train, torch.float64)
    assert rel_err(out.detach().cpu().double(), o) < tp.TOL
    assert rel_err(xg.grad.cpu().double(), xgrad) < tp.TOL
    worst = ("", 0.0)
    for name, prm in layer.named_parameters():
        if ref[name] is None or float(ref[name].abs().max()) == 0.0:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, name
            continue
        err = rel_err(prm.grad.cpu().double(), ref[name])
        worst = max(worst, (name, err), key=lambda v: v[1])
        assert err < 5e-5, (name, err)
    print("layer %r train=%s: worst parameter gradient %s %.3g" % ((B, I, O, T), train, worst[0], worst[1]))
