"""GPU tier: the planar-flow forward (K3) and the KL tail (K5) of csrc/mnf_flow.hip called directly, in every kernel form,
against float64 (tests/planar_forward_ref.py).  The host tier (tests/test_planar_forward_forms_host.py) asserts the form of
every case through lbbnn_flow_planar_form / lbbnn_kl_finalize_form and the conditioning of the inputs.

Bars, set before any kernel was run:
  z_fwd, z_kl       max-norm < 5e-6 (TIGHT, the bar test_planar_flow_vs_golden holds a planar z to); the inputs displace z by
                    at least 0.1 max|z0|, so this is a statement about the flow
  one number        (scal[0..4], kl_layer, kl_out) |got - ref64| <= max(5e-6 S, 4 E32): S the sum of the magnitudes of the terms
                    the number is a sum of (a log-det: max(1, Sum_t Sum_i |u_i w_i|)), E32 the error of the float32 restatement
                    on the same inputs; the host tier asserts that no bar of the tables lies above 5e-6 S
  draws             a call that draws in the kernel equals, bit for bit, the same call handed the same draws
Every output is allocated with 8 guard floats behind it and filled with NaN before the call (the ``poison`` fixture): what a
kernel must not write has to be NaN afterwards, what it must write cannot pass on an earlier call's bits.

Measured on an MI355X when this was written (every test prints its figures); no form exceeded a bar:
  form      z max-norm   log_det_q   log_q0    log_det_r   z_b[-1]   forward log-det     (one-number figures in units of S)
  vec       2.5e-7       6.7e-8      1.1e-7    8.9e-8      1.7e-7    8.1e-8
  fast      5.8e-7       9.3e-8      3.6e-7    9.3e-8      9.3e-8    3.9e-7
  lds       1.8e-7       7.9e-8      3.6e-7    6.5e-8      4.2e-8    3.6e-7
  generic   1.8e-7       8.7e-9      2.9e-8    1.8e-8      2.9e-8    1.4e-8
  batched   1.5e-7       8.2e-8      9.0e-8    8.6e-8      1.8e-7    5.8e-8              (lbbnn_layers_prepare, all groups)
  K5: kl_layer 5.2e-8 S at most through lbbnn_kl_finalize (both forms; the worst at O = 6081), 7.7e-8 S through
  lbbnn_layers_prepare and lbbnn_layers_finalize (staged and unstaged).  The worst one-number figure is 0.08 of its bar
  (fast, I = 1).
Section d: the fast form's z equals the lds form's bit for bit at I = 257 and is 4.8e-8 of max|z| off at I = 2049 (z_fwd);
the register form's z0 differs from the fast form's in 26 of 256 elements, by 5.2e-8 of max|z| at most.  Both comments in
csrc/mnf_flow.hip claimed equal bits and were corrected.

Three arithmetic slips, each put alone into a scratch build, failed every case of sections a / e that runs the line:
  1. sign of log_det_r in the vec form: all 24 vec cases with the KL branch and an r flow, and the two batched groups whose
     launch takes the vec form (n2-vec, n3-nokl-between);
  2. the r flow's first bias read from the z flow's slot in the fast form: all 31 fast cases with the KL branch, Tz >= 1 and
     Tr >= 1 (18 by length, 12 by alignment, the one at the budget edge) and the groups n3-fast-lrt and n4-fast; the nine
     (0, 2) cases have no z-flow slot and passed;
  3. -0.5 log pi dropped from log_rb in kl_finalize_all_kernel: all seven groups of the all-layers tail.
Cases of section a per form: vec 66, fast 76, lds 14, generic 6; K5 single entry: lds 23, generic 3 (5 more in the output
variants, 6 with in-kernel draws); 6 batched groups (n = 2, 3, 4), 8 all-layers groups (n = 1 .. 4, 3 of them unstaged)."""
import math

import pytest
import torch

import planar_forward_ref as pf

pytestmark = pytest.mark.gpu
GUARD = 8


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


class Out:
    """An output of n floats with GUARD floats behind it (and, offset, one float in front: the view then starts one float
    past a 16-byte boundary), all NaN."""

    def __init__(self, dev, n, offset=False):
        lead = 4 if offset else 0
        self.buf = torch.empty(lead + n + GUARD, dtype=torch.float32, device=dev)
        assert bool(torch.isnan(self.buf).all())
        self.v = self.buf[lead - 3:lead - 3 + n] if offset else self.buf[:n]
        assert self.v.data_ptr() % 16 == (4 if offset else 0) and self.v.is_contiguous()
        self.lo, self.n = (lead - 3 if offset else 0), n

    def untouched_outside(self):
        b = self.buf.cpu()
        return bool(torch.isnan(b[:self.lo]).all()) and bool(torch.isnan(b[self.lo + self.n:]).all())

    def cpu(self):
        return self.v.cpu()


def _in(t, dev, offset=False):
    """An input on the device; offset: as a contiguous view one float past a 16-byte boundary."""
    if not offset:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=dev)
    v = buf[1:1 + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _k3(ops, dev, d, Tz, Tr, want_kl, offset=None, explicit=True, rng=None, layer_id=0, with_scal=True):
    """One lbbnn_mnf_flow_planar call on the inputs d.  Returns {'z_fwd', 'z_kl', 'scal'} on the CPU (NaN where nothing was
    written) after checking that nothing outside the outputs was written."""
    dd = {k: _in(v, dev, k == offset) for k, v in d.items()}
    zf, zk, sc = Out(dev, d["q0_mean"].numel(), offset == "z_fwd"), Out(dev, d["q0_mean"].numel(), offset == "z_kl"), Out(dev, 8)
    ops.mnf_flow_planar(dd["q0_mean"], dd["q0_log_var"], pf.flow_params(dd, "z", Tz), pf.flow_params(dd, "r", Tr) if want_kl else [],
                        eps_fwd=dd["eps_fwd"] if explicit else None, eps_kl=dd["eps_kl"] if explicit and want_kl else None,
                        rng=rng, layer_id=layer_id, z_fwd=zf.v, z_kl=zk.v, scal=sc.v if (with_scal or want_kl) else None,
                        want_kl=want_kl)
    torch.cuda.synchronize()
    assert zf.untouched_outside() and zk.untouched_outside() and sc.untouched_outside(), "a guard float was written"
    got = {"z_fwd": zf.cpu(), "z_kl": zk.cpu(), "scal": sc.cpu()}
    _written_exactly(got, want_kl, with_scal or want_kl)
    return got


def _written_exactly(got, want_kl, scal_passed):
    """Section b: z_fwd always; z_kl and scal[0..3] with the KL branch only; scal[4] exactly when scal is passed; scal[5..7] never."""
    assert bool(torch.isfinite(got["z_fwd"]).all())
    assert bool(torch.isnan(got["scal"][5:]).all())
    assert bool(torch.isfinite(got["scal"][4])) == bool(scal_passed)
    if want_kl:
        assert bool(torch.isfinite(got["z_kl"]).all()) and bool(torch.isfinite(got["scal"][:4]).all())
    else:
        assert bool(torch.isnan(got["z_kl"]).all()) and bool(torch.isnan(got["scal"][:4]).all())


def _check_k3(got, r64, r32, want_kl, tag):
    """The bars of one K3 call; prints the figures, returns the failures."""
    bad, line = [], []
    for k in ("z_fwd", "z_kl") if want_kl else ("z_fwd",):
        err = pf.rel_err(got[k], r64[k])
        line.append("%s %.3g" % (k, err))
        if not err < pf.TIGHT:
            bad.append("%s %s: max-norm %.3g (bar %.3g)" % (tag, k, err, pf.TIGHT))
    for name, (bar, S) in pf.k3_bars(r64, r32).items():
        i = pf.SCAL_NAMES.index(name)
        err = abs(float(got["scal"][i]) - r64["scal"][i])
        line.append("%s %.3g/S (bar %.3g/S)" % (name, err / S, bar / S))
        if not err <= bar:
            bad.append("%s %s: off by %.3g = %.3g S (bar %.3g = %.3g S; got %.9g, reference %.9g)" % (
                tag, name, err, err / S, bar, bar / S, float(got["scal"][i]), r64["scal"][i]))
    print("K3 %s: %s" % (tag, " | ".join(line)))
    return bad


# --------------------------------------------------------------------------- a / b. K3, every table case against float64
@pytest.mark.parametrize("case", pf.K3_CASES, ids=pf.k3_id)
def test_k3_every_form_against_float64(bnn, dev, poison, case):
    form, I, Tz, Tr, want_kl, offset, special = case
    assert pf.k3_case_form(case) == form
    d = pf.make_inputs(I, pf.K3_O, Tz, Tr, 0, special)
    r64, r32 = pf.k3_references(I, Tz, Tr, 0, want_kl, tuple(sorted(special.items())) if special else None)
    got = _k3(bnn.ops, dev, d, Tz, Tr, want_kl, offset)
    bad = _check_k3(got, r64, r32, want_kl, pf.k3_id(case))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", [c for c in pf.K3_CASES if not c[4] and c[1] in (8, 65, 257, 1025, 16384) and c[5] is None],
                         ids=pf.k3_id)
def test_k3_forward_block_without_scal_writes_z_only(bnn, dev, poison, case):
    form, I, Tz, Tr, want_kl, offset, special = case
    d = pf.make_inputs(I, pf.K3_O, Tz, Tr, 0, special)
    got = _k3(bnn.ops, dev, d, Tz, Tr, False, with_scal=False)
    assert bool(torch.isnan(got["scal"]).all())
    assert pf.rel_err(got["z_fwd"], pf.k3_references(I, Tz, Tr, 0, False, None)[0]["z_fwd"]) < pf.TIGHT


# --------------------------------------------------------------------------- c. in-kernel draws, per form
DRAW_CASES = [(pf.VEC, 256, 2, 2), (pf.FAST, 65, 1, 3), (pf.FAST, 2052, 2, 2), (pf.LDS, 257, 3, 2), (pf.LDS, 1025, 8, 6),
              (pf.GENERIC, 3073, 2, 2)]


@pytest.mark.parametrize("L", [3, 70])
@pytest.mark.parametrize("form,I,Tz,Tr", DRAW_CASES, ids=["%s-%d" % (pf.FORM_NAME[c[0]], c[1]) for c in DRAW_CASES])
def test_k3_in_kernel_draws_equal_the_same_draws_handed_in(bnn, dev, poison, form, I, Tz, Tr, L):
    ops = bnn.ops
    bnn.manual_seed(1234, 7)
    snap = ops.RngState.get(dev).t[:2].clone()
    d = dict(pf.make_inputs(I, pf.K3_O, Tz, Tr, 0))
    # the kernels keep the low six bits of the layer id: the stream of layer 70 is that of layer 6, not EPS_Z2's
    d["eps_fwd"] = ops.philox_normal(snap, ops.STREAM_EPS_Z * 64 + (L & 63), 0, I).cpu()
    d["eps_kl"] = ops.philox_normal(snap, ops.STREAM_EPS_Z2 * 64 + (L & 63), 0, I).cpu()
    assert d["eps_fwd"].shape == (I,) and not torch.equal(d["eps_fwd"], d["eps_kl"])
    assert 0.5 < float(d["eps_fwd"].std()) < 1.5 and 0.5 < float(d["eps_kl"].std()) < 1.5
    if L >= 64:
        assert not torch.equal(d["eps_fwd"], ops.philox_normal(snap, ops.STREAM_EPS_Z * 64 + L, 0, I).cpu())
    for want_kl in (True, False):
        if pf.k3_form([(I, Tz, Tr, want_kl, 1)]) != form:
            continue
        a = _k3(ops, dev, d, Tz, Tr, want_kl, explicit=True, layer_id=L)
        b = _k3(ops, dev, d, Tz, Tr, want_kl, explicit=False, rng=snap, layer_id=L)
        for k in ("z_fwd", "z_kl", "scal"):
            assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), (k, want_kl)
        assert torch.equal(ops.RngState.get(dev).t[:2], snap)            # K3 reads the state, it does not advance it


# --------------------------------------------------------------------------- K5, single entry
def _k5(ops, dev, d, mnf, *, kl_layer=True, kl_out=False, accumulate=None, eps=True, rng=None, layer_id=0, scal=None):
    """One lbbnn_kl_finalize call.  Returns (kl_layer, kl_out) as floats (NaN: not written)."""
    dd = {k: v.to(dev) for k, v in d.items()}
    sc = Out(dev, 8)
    sc.v.copy_((d["scal_k5"] if scal is None else scal).to(dev))
    kl_l, kl_o = Out(dev, 1), Out(dev, 1)
    if accumulate is not None:
        kl_o.v.fill_(accumulate)
    m = dict(act_mu=dd["act_mu"], act_var=dd["act_var"], eps_act=dd["eps_act"] if eps else None, r0_b1=dd["r0_b1"],
             r0_b2=dd["r0_b2"], scal=sc.v, rng=rng, layer_id=layer_id) if mnf else {}
    ops.kl_finalize(dd["kl_rows"], dd["bias_mu"], dd["bias_rho"], priors=ops.Priors(), kl_layer=kl_l.v if kl_layer else None,
                    kl_out=kl_o.v if kl_out else None, accumulate=accumulate is not None, **m)
    torch.cuda.synchronize()
    assert kl_l.untouched_outside() and kl_o.untouched_outside() and sc.untouched_outside()
    assert torch.equal(sc.cpu()[:4], (d["scal_k5"] if scal is None else scal)[:4])                      # an input: left alone
    return float(kl_l.cpu()), float(kl_o.cpu())


def _check_k5(got, r64, r32, tag):
    bar, err = pf.k5_bar(r64, r32), abs(got - r64["kl"])
    print("K5 %s: kl off by %.3g/S (bar %.3g/S; smallest term %.3g of the sum)" % (tag, err / r64["S"], bar / r64["S"],
                                                                                  pf.smallest_term_share(r64)))
    assert err <= bar, "%s: kl %.9g, reference %.9g: off by %.3g = %.3g S (bar %.3g S)" % (tag, got, r64["kl"], err,
                                                                                           err / r64["S"], bar / r64["S"])


def _k5_refs(d, mnf, scal=None):
    s = (d["scal_k5"] if scal is None else scal) if mnf else None
    return pf.k5_reference(d, s), pf.k5_reference(d, s, torch.float32)


@pytest.mark.parametrize("form,O,I,mnf", pf.K5_CASES, ids=["%s-%dx%d-%s" % ("lds" if c[0] else "generic", c[1], c[2],
                                                                             "mnf" if c[3] else "lrt") for c in pf.K5_CASES])
def test_k5_every_form_against_float64(bnn, dev, poison, form, O, I, mnf):
    assert pf.k5_form([(O, I, mnf, 1)]) == form
    d = pf.make_k5_inputs(O, I, 0, mnf)
    kl_l, kl_o = _k5(bnn.ops, dev, d, mnf)
    assert math.isnan(kl_o)
    _check_k5(kl_l, *_k5_refs(d, mnf), "%r" % ((O, I, mnf),))


@pytest.mark.parametrize("form,O,I,mnf", pf.K5_VARIANT_CASES, ids=["%s-%dx%d-%s" % ("lds" if c[0] else "generic", c[1], c[2],
                                                                                     "mnf" if c[3] else "lrt") for c in pf.K5_VARIANT_CASES])
def test_k5_output_variants(bnn, dev, poison, form, O, I, mnf):
    """kl_layer alone, kl_out alone, both, and accumulate=True onto a known value."""
    assert pf.k5_form([(O, I, mnf, 1)]) == form
    d = pf.make_k5_inputs(O, I, 1, mnf)
    r64, r32 = _k5_refs(d, mnf)
    a = _k5(bnn.ops, dev, d, mnf, kl_layer=True, kl_out=False)
    b = _k5(bnn.ops, dev, d, mnf, kl_layer=False, kl_out=True)
    c = _k5(bnn.ops, dev, d, mnf, kl_layer=True, kl_out=True)
    assert math.isnan(a[1]) and math.isnan(b[0])
    assert a[0] == b[1] == c[0] == c[1]                                   # one value, stored where asked
    _check_k5(a[0], r64, r32, "%r kl_layer" % ((O, I, mnf),))
    base = float(torch.tensor(0.37 * abs(r64["kl"]), dtype=torch.float32))
    e = _k5(bnn.ops, dev, d, mnf, kl_layer=True, kl_out=True, accumulate=base)
    assert e[0] == a[0]
    assert e[1] == float(torch.tensor(base, dtype=torch.float32) + torch.tensor(a[0], dtype=torch.float32))   # one fp32 add


K5_DRAW_CASES = [(pf.K5_LDS, 65, 300), (pf.K5_LDS, 3000, 300), (pf.K5_GENERIC, 700, 16384)]


@pytest.mark.parametrize("L", [2, 69])
@pytest.mark.parametrize("form,O,I", K5_DRAW_CASES, ids=["lds-65", "lds-3000", "generic-700"])
def test_k5_in_kernel_draws_equal_the_same_draws_handed_in(bnn, dev, poison, form, O, I, L):
    ops = bnn.ops
    assert pf.k5_form([(O, I, 1, 1)]) == form
    bnn.manual_seed(4321, 3)
    snap = ops.RngState.get(dev).t[:2].clone()
    d = dict(pf.make_k5_inputs(O, I, 2))
    d["eps_act"] = ops.philox_normal(snap, ops.STREAM_EPS_ACT * 64 + (L & 63), 0, O).cpu()
    assert 0.5 < float(d["eps_act"].std()) < 1.5
    a = _k5(ops, dev, d, True, layer_id=L)
    b = _k5(ops, dev, d, True, eps=False, rng=snap, layer_id=L)
    assert math.isfinite(a[0]) and a[0] == b[0]
    _check_k5(b[0], *_k5_refs(d, True), "%r drawn in the kernel, layer id %d" % ((O, I), L))


# --------------------------------------------------------------------------- descriptors on tensors the test owns
class Layer:
    """One lbbnn_layer_desc_t over tensors this object owns.  I, O, flows and draws from planar_forward_ref.make_inputs; with
    weights (rows <= 8) for lbbnn_layers_prepare, vectors only for lbbnn_layers_finalize."""

    def __init__(self, ops, dev, desc, d, I, O, Tz, Tr, want_kl, mnf, layer_id, weights, eps_act=True, members=1):
        self.d, self.I, self.O, self.Tz, self.Tr, self.want_kl, self.mnf = d, I, O, Tz, Tr, want_kl, mnf
        self.t = {k: v.to(dev) for k, v in d.items()}
        t, ld = self.t, ops.operand_ld(max(I, 1))
        g = torch.Generator().manual_seed(100 + layer_id)
        if weights:
            from oracle import lbbnn_oracle as orc
            self.w = {k: v.to(dev) for k, v in orc.init_lrt_params(I, O, g).items() if k.startswith(("weight", "lambdal"))}
            self.w["r0_c"] = (0.1 * torch.randn(I, generator=g)).to(dev)
            self.e_w, self.var_w = Out(dev, members * O * ld), Out(dev, O * ld)
            self.bias_var = Out(dev, O)
            desc.weight_mu, desc.weight_rho, desc.lambdal = (self.w[k].data_ptr() for k in ("weight_mu", "weight_rho", "lambdal"))
            desc.e_w, desc.var_w, desc.bias_var = self.e_w.v.data_ptr(), self.var_w.v.data_ptr(), self.bias_var.v.data_ptr()
            desc.r0_c = self.w["r0_c"].data_ptr() if mnf else None
            self.kl_rows, self.act_mu, self.act_var = Out(dev, O), Out(dev, O), Out(dev, O)
            desc.kl_rows, desc.act_mu, desc.act_var = (o.v.data_ptr() for o in (self.kl_rows, self.act_mu, self.act_var))
        else:
            desc.kl_rows, desc.act_mu, desc.act_var = (t[k].data_ptr() for k in ("kl_rows", "act_mu", "act_var"))
        desc.bias_mu, desc.bias_rho = t["bias_mu"].data_ptr(), t["bias_rho"].data_ptr()
        desc.priors = ops.Priors()
        desc.O, desc.I, desc.layer_id, desc.stochastic, desc.want_kl, desc.split = O, max(I, 1), layer_id, 1, int(want_kl), 0
        self.kl_layer = Out(dev, 1)
        desc.kl_layer = self.kl_layer.v.data_ptr()
        self.z_fwd, self.z_kl, self.scal = Out(dev, members * ld if members > 1 else max(I, 1)), Out(dev, max(I, 1)), Out(dev, 8)
        if mnf:
            desc.r0_b1, desc.r0_b2 = t["r0_b1"].data_ptr(), t["r0_b2"].data_ptr()
            # (lbbnn_layers_finalize reads of q0_mean only that it is not NULL: an MNF layer)
            desc.q0_mean, desc.q0_log_var = (t[k].data_ptr() for k in (("q0_mean", "q0_log_var") if weights else ("r0_b1", "r0_b2")))
            for fl, T, f in (("z", Tz, desc.z_flow), ("r", Tr, desc.r_flow)):
                f.T = T
                for k in range(T):
                    f.u[k], f.w[k], f.b[k] = (t["%s.%d.%s" % (fl, k, c)].data_ptr() for c in "uwb")
            if members == 1 and weights:
                desc.eps_z, desc.eps_z2 = t["eps_fwd"].data_ptr(), t["eps_kl"].data_ptr()
            desc.eps_act = t["eps_act"].data_ptr() if eps_act else None
            desc.z_fwd, desc.z_kl, desc.scal = self.z_fwd.v.data_ptr(), self.z_kl.v.data_ptr(), self.scal.v.data_ptr()
            if not weights:
                self.scal.v.copy_(t["scal_k5"])

    def outs(self):
        return [o for o in (self.z_fwd, self.z_kl, self.scal, self.kl_layer, getattr(self, "e_w", None), getattr(self, "var_w", None),
                            getattr(self, "bias_var", None)) if o is not None] + (
            [self.kl_rows, self.act_mu, self.act_var] if hasattr(self, "e_w") else [])


# --------------------------------------------------------------------------- batched launches through lbbnn_layers_prepare
def _prepare_group(bnn, dev, layers_spec, seeds=None):
    from bnn_amd import _lib
    descs = (_lib.LayerDesc * len(layers_spec))()
    layers = []
    for k, (I, O, Tz, Tr, kl, mnf) in enumerate(layers_spec):
        d = pf.make_inputs(I, O, Tz, Tr, (seeds or {}).get(k, 10 + k))
        layers.append(Layer(bnn.ops, dev, descs[k], d, I, O, Tz, Tr, kl, mnf, k + 1, True))
    _lib.check(_lib.lib().lbbnn_layers_prepare(descs, len(layers), None, _stream()), "lbbnn_layers_prepare")
    torch.cuda.synchronize()
    for L in layers:
        assert all(o.untouched_outside() for o in L.outs())
    return layers


def _check_prepared_layer(L, tag):
    bad = []
    if L.mnf:
        got = {"z_fwd": L.z_fwd.cpu(), "z_kl": L.z_kl.cpu(), "scal": L.scal.cpu()}
        _written_exactly(got, L.want_kl, True)
        r64, r32 = pf.k3_reference(L.d, L.want_kl), pf.k3_reference(L.d, L.want_kl, torch.float32)
        bad += _check_k3(got, r64, r32, L.want_kl, tag)
    else:
        assert bool(torch.isnan(L.z_fwd.cpu()).all()) and bool(torch.isnan(L.scal.cpu()).all())
    if L.want_kl:
        # K5 on what K1 and K3 left on the device
        k5_in = dict(L.d, kl_rows=L.kl_rows.cpu(), **({"act_mu": L.act_mu.cpu(), "act_var": L.act_var.cpu()} if L.mnf else {}))
        assert bool(torch.isfinite(k5_in["kl_rows"]).all())
        s = L.scal.cpu() if L.mnf else None
        _check_k5(float(L.kl_layer.cpu()), pf.k5_reference(k5_in, s), pf.k5_reference(k5_in, s, torch.float32), tag)
    else:
        assert math.isnan(float(L.kl_layer.cpu())) and bool(torch.isnan(L.kl_rows.cpu()).all())
    return bad


@pytest.mark.parametrize("name", sorted(pf.PREPARE_GROUPS))
def test_batched_prepare_every_layer_against_float64(bnn, dev, poison, name):
    form, spec = pf.PREPARE_GROUPS[name]
    assert pf.k3_form([(I, Tz, Tr, kl, 1) for I, O, Tz, Tr, kl, mnf in spec if mnf]) == form
    bad = []
    for k, L in enumerate(_prepare_group(bnn, dev, spec)):
        bad += _check_prepared_layer(L, "%s[%d] %r" % (name, k, spec[k]))
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------- d. claims the source makes
@pytest.mark.parametrize("I", [257, 2049])
def test_fast_form_z_against_the_step_by_step_form(bnn, dev, poison, I):
    """The same (2, 2) layer alone (fast form: one reduction for the whole chain) and beside a (3, 2) companion (lds form: one
    reduction per transform), both against float64 and against each other.  The source called the fast form's z
    "bit-identical to the step-by-step form".  It is at I = 257 and it is not at I = 2049 (z_fwd 4.8e-8 of max|z| apart when
    this was written): z is summed in the same order, but tanh of transform t is taken of w_t.z_0 + Sum_s th_s (w_t.u_s) in
    the one and of w_t.z_t, on the rounded z_t, in the other.  The comment now says so; the pair is held to the bar of a z."""
    a_spec, comp = (I, 3, 2, 2, True, True), (64, 3, 3, 2, True, True)
    assert pf.k3_form([(I, 2, 2, 1, 1)]) == pf.FAST and pf.k3_form([(I, 2, 2, 1, 1), (64, 3, 2, 1, 1)]) == pf.LDS
    alone = _prepare_group(bnn, dev, [a_spec])[0]
    beside = _prepare_group(bnn, dev, [a_spec, comp])[0]
    bad = _check_prepared_layer(alone, "alone (fast)") + _check_prepared_layer(beside, "beside a (3, 2) layer (lds)")
    assert not bad, "\n".join(bad)
    for k, x, y in (("z_fwd", alone.z_fwd, beside.z_fwd), ("z_kl", alone.z_kl, beside.z_kl)):
        x, y = x.cpu(), y.cpu()
        print("fast against lds, I = %d, %s: bitwise equal %s, worst difference %.3g of max|z|" % (I, k, torch.equal(x, y), pf.rel_err(x, y)))
        assert pf.rel_err(x, y) < pf.TIGHT, k


def test_register_form_z0_against_the_lds_forms(bnn, dev, poison):
    """Tz = 0, where z_fwd IS z0 = q0_mean + exp(q0_log_var)^.5 eps: 16-byte aligned inputs (register form: hardware exp2 with
    the residual put back, v_sqrt_f32) against the same inputs with q0_mean one float off (fast form: expf, sqrtf).
    The source said "same draws, same z0 bits": the draws are the same, the z0 are not -- 26 of 256 elements differed, by at
    most 5.2e-8 of max|z|, when this was written; the comment now says so, and the pair is held to the bars instead."""
    I, Tz, Tr = 256, 0, 4
    assert pf.k3_form([(I, Tz, Tr, 1, 1)]) == pf.VEC and pf.k3_form([(I, Tz, Tr, 1, 0)]) == pf.FAST
    d = pf.make_inputs(I, pf.K3_O, Tz, Tr, 0)
    v = _k3(bnn.ops, dev, d, Tz, Tr, True)
    f = _k3(bnn.ops, dev, d, Tz, Tr, True, offset="q0_mean")
    r64, r32 = pf.k3_references(I, Tz, Tr, 0, True, None)
    bad = _check_k3(v, r64, r32, True, "vec") + _check_k3(f, r64, r32, True, "fast")
    assert not bad, "\n".join(bad)
    for k in ("z_fwd", "z_kl"):
        diff = (v[k].double() - f[k].double()).abs()
        print("vec against fast, %s = z0: bitwise equal %s, %d of %d elements differ, worst difference %.3g of max|z|" % (
            k, torch.equal(v[k], f[k]), int((diff > 0).sum()), I, pf.rel_err(v[k], f[k])))
        assert pf.rel_err(v[k], f[k]) < pf.TIGHT


# --------------------------------------------------------------------------- e. the all-layers tail
def _finalize_group(bnn, dev, name, eps_from=None):
    """lbbnn_layers_finalize on FINALIZE_GROUPS[name].  eps_from: {layer: eps_act tensor} to hand in instead of drawing.
    Returns (layers, kl_total or None, rng before, rng after)."""
    from bnn_amd import _lib
    ops = bnn.ops
    staged, spec, draws, advance = pf.FINALIZE_GROUPS[name]
    assert pf.k5_form([(O, I, mnf, act) for O, I, mnf, act in spec], all_layers=True) == staged
    descs = (_lib.LayerDesc * len(spec))()
    layers = []
    for k, (O, I, mnf, active) in enumerate(spec):
        d = dict(pf.make_k5_inputs(O, I, 20 + k, mnf))
        if eps_from is not None and mnf:
            d["eps_act"] = eps_from[k]
        layers.append(Layer(ops, dev, descs[k], d, I, O, 0, 0, active, mnf, 62 + k, False, eps_act=not draws or eps_from is not None))
    bnn.manual_seed(99, 11)
    rng = ops.RngState.get(dev).t[:2].clone()
    before = rng.clone()
    all_active = all(s[3] for s in spec)
    total = Out(dev, 1)
    _lib.check(_lib.lib().lbbnn_layers_finalize(descs, len(spec), rng.data_ptr(), advance, total.v.data_ptr() if all_active else None,
                                                _stream()), "lbbnn_layers_finalize")
    torch.cuda.synchronize()
    assert total.untouched_outside() and all(L.kl_layer.untouched_outside() for L in layers)
    return layers, (float(total.cpu()) if all_active else None), before, rng


@pytest.mark.parametrize("name", sorted(pf.FINALIZE_GROUPS))
def test_all_layers_tail_against_float64(bnn, dev, poison, name):
    ops = bnn.ops
    staged, spec, draws, advance = pf.FINALIZE_GROUPS[name]
    layers, total, before, after = _finalize_group(bnn, dev, name)
    assert int(after[0]) == int(before[0]) and int(after[1]) == int(before[1]) + advance       # advanced once, by `advance`
    eps = None
    if draws:
        # the draws are those of the offset BEFORE the advance
        eps = {k: ops.philox_normal(before, ops.STREAM_EPS_ACT * 64 + ((62 + k) & 63), 0, s[0]).cpu() for k, s in enumerate(spec) if s[2]}
        again, total2, _, _ = _finalize_group(bnn, dev, name, eps_from=eps)
        assert [float(L.kl_layer.cpu()) for L in again] == [float(L.kl_layer.cpu()) for L in layers] and total2 == total
    kls = []
    for k, (L, (O, I, mnf, active)) in enumerate(zip(layers, spec)):
        got = float(L.kl_layer.cpu())
        if not active:
            assert math.isnan(got)
            continue
        d = dict(L.d, eps_act=eps[k]) if (draws and mnf) else L.d
        _check_k5(got, *_k5_refs(d, mnf), "%s[%d] %r" % (name, k, (O, I, mnf)))
        kls.append(got)
    if total is not None:
        fold = torch.zeros((), dtype=torch.float32)
        for v in kls:
            fold = fold + torch.tensor(v, dtype=torch.float32)
        assert total == float(fold), (total, float(fold))                   # the fp32 left fold of what the kernel wrote
    else:
        assert name == "n3-inactive"


# --------------------------------------------------------------------------- f. return codes that launch nothing
@pytest.mark.parametrize("I,Tz,why", [(256, 5, "more than 4 transforms"), (2048, 8, "past the LDS budget")])
def test_member_dimension_is_refused_outside_the_short_chain_forms(bnn, dev, poison, I, Tz, why):
    from bnn_amd import _lib
    assert pf.k3_form([(I, Tz, 0, 0, 1)]) in (pf.LDS, pf.GENERIC) and pf.k3_form([(I, Tz, 0, 0, 1)], members=3) == -2
    assert pf.k3_form([(I, 4, 0, 0, 1)], members=3) == pf.VEC
    descs = (_lib.LayerDesc * 1)()
    L = Layer(bnn.ops, dev, descs[0], pf.make_inputs(I, 4, Tz, 0, 30), I, 4, Tz, 0, False, True, 1, True, members=3)
    rng = bnn.ops.RngState.get(dev).t[:2].clone()
    before = rng.clone()
    rc = _lib.lib().lbbnn_ensemble_operands(descs, 1, 3, rng.data_ptr(), 1, _stream())
    torch.cuda.synchronize()
    assert rc == -2, (rc, why)
    assert torch.equal(rng, before)
    for o in L.outs():
        assert bool(torch.isnan(o.buf).all())                              # nothing was launched


def test_total_with_an_inactive_layer_is_refused(bnn, dev, poison):
    from bnn_amd import _lib
    spec = pf.FINALIZE_GROUPS["n3-inactive"][1]
    descs = (_lib.LayerDesc * len(spec))()
    layers = [Layer(bnn.ops, dev, descs[k], pf.make_k5_inputs(O, I, 20 + k, mnf), I, O, 0, 0, active, mnf, 62 + k, False)
              for k, (O, I, mnf, active) in enumerate(spec)]
    total = Out(dev, 1)
    rng = bnn.ops.RngState.get(dev).t[:2].clone()
    before = rng.clone()
    rc = _lib.lib().lbbnn_layers_finalize(descs, len(spec), rng.data_ptr(), 5, total.v.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == -1
    assert torch.equal(rng, before) and bool(torch.isnan(total.buf).all())
    assert all(bool(torch.isnan(L.kl_layer.buf).all()) for L in layers)
