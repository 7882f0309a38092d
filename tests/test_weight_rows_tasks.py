"""GPU tier: the two-wave row tasks of the weight pass (weight_row_tasks_kernel, csrc/weight_pass.hip) through the raw entry
points, at the shapes where the split of a row between its two waves can go wrong.

A row of I floats is G = ceil(ld / 256) float4 groups of 64 lanes (ld = I rounded up to 32); wave 0 takes the first
ceil(G / 2) groups, wave 1 the rest.  I = 8: G = 1, wave 1 has no group.  256: G = 1, full.  260: G = 2, the second group nearly
empty (1 + 6 tail lanes).  516: G = 3 (odd).  784: G = 4.  1200: G = 5 (the headline rows).  1280: G = 5, every lane in use.

Checks:
  * operands and row scales are BYTE-equal to the generic producer: the generic kernel's fp32 operands (taken by giving it
    parameters off a 16-byte boundary), put into each 16-bit format on the host with the format's own exact operations
    (RNE conversions, an exact power-of-two scale) -- the relation lbbnn_weight_operands_t == K1 that the suite relies on;
  * the row sums (kl_rows, act_mu, act_var) are within the fp64 bars of test_weight_pass_vs_oracle (5e-6 / 2e-5 / 5e-6),
    byte-equal between two calls, byte-equal between the operand formats, and byte-equal to tests/golden/weight_rows_sums.npz,
    recorded from the one-wave row kernel this one replaces (``python tests/test_weight_rows_tasks.py record <out.npz>``)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import lbbnn_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES_I = (8, 256, 260, 516, 784, 1200, 1280)
SHAPES_O = (1, 3, 17)
TIGHT = 5e-6          # test_parity_gpu.py: the bar of test_weight_pass_vs_oracle (act_mu: 2e-5)
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_rows_sums.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture(scope="module")
def sums_golden():
    return np.load(GOLDEN_FILE, allow_pickle=False)


def _params(I, O):
    """The parameter ranges of test_weight_pass_vs_oracle (the reference's init distributions), the three per-column vectors,
    bias_rho -- fp32 on the CPU."""
    g = torch.Generator().manual_seed(1000 * I + O)
    q = orc.init_mnf_params(I, O, g)
    return {"mu": q["weight_mu"], "rho": q["weight_rho"], "lam": q["lambdal"], "zf": 1 + 0.1 * torch.randn(I, generator=g),
            "zk": 1 + 0.1 * torch.randn(I, generator=g), "rc": q["r0_c"], "brho": q["bias_rho"]}


def _off16(t, dev):
    """A device copy of t whose data pointer is 4 bytes past a 16-byte boundary: the weight pass takes its generic kernel."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _run(bnn, dev, d, O, I, *, split=0, z=True, sums=True, mu_key="mu"):
    """One weight-pass call; returns the outputs (NaN-filled beforehand, so an unwritten element shows)."""
    ops = bnn.ops
    ld = ops.operand_ld(I)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    o = {"e_w": nan(O, ld), "var_w": nan(O, ld), "bias_var": nan(O)}
    kw = {}
    if split >= 2:
        o["e_scale"], o["v_scale"] = nan(O), nan(O)
        kw.update(e_scale=o["e_scale"], v_scale=o["v_scale"])
    if sums:
        o["kl_rows"] = nan(O)
        kw["kl_rows"] = o["kl_rows"]
        if z:
            o["act_mu"], o["act_var"] = nan(O), nan(O)
            kw.update(act_mu=o["act_mu"], act_var=o["act_var"])
    if z:
        kw.update(z_fwd=d["zf"], z_kl=d["zk"] if sums else None, r0_c=d["rc"] if sums else None)
    ops.weight_pass(d[mu_key], d["rho"], d["lam"], bias_rho=d["brho"], priors=bnn.Priors(), e_w=o["e_w"], var_w=o["var_w"],
                    bias_var=o["bias_var"], split=split, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _units(hi, lo):
    """(O, ld) 16-bit hi and lo values -> the bytes of the hi | lo unit layout: per 32 k one 128-B line of eight 16-B units,
    unit 2g = hi of k in [8g, 8g + 8), unit 2g + 1 = lo of the same k."""
    O, ld = hi.shape
    h = hi.contiguous().view(torch.int16).view(O, ld // 32, 4, 1, 8)
    l = lo.contiguous().view(torch.int16).view(O, ld // 32, 4, 1, 8)
    return torch.cat([h, l], dim=3).reshape(O, 2 * ld)


def _pow2_scale(m):
    """The row kernel's exact power-of-two scale for a row maximum m (puts it into [2^13, 2^14)) and its inverse; 1 for m = 0."""
    _, e = torch.frexp(m)                            # m = mant * 2^e, mant in [0.5, 1)
    s = torch.where(m > 0, torch.ldexp(torch.ones_like(m), 14 - e), torch.ones_like(m))
    return s, 1.0 / s


def _expect(E, V, split):
    """The bytes a format holds, from the generic producer's fp32 operands (O, ld): int16 views (int32 for fp32)."""
    if split == 0:
        return {"e_w": E.view(torch.int32), "var_w": V.view(torch.int32)}
    if split == 1:
        out = {}
        for k, W in (("e_w", E), ("var_w", V)):
            hi = W.to(torch.bfloat16)
            out[k] = _units(hi, (W - hi.float()).to(torch.bfloat16))
        return out
    se, ie = _pow2_scale(E.abs().amax(dim=1))
    sv, iv = _pow2_scale(V.amax(dim=1))
    Es, Vs = E * se[:, None], V * sv[:, None]
    hi = Es.to(torch.float16)
    out = {"e_w": _units(hi, (Es - hi.float()).to(torch.float16)), "e_scale": ie.view(torch.int32), "v_scale": iv.view(torch.int32)}
    vh = Vs.to(torch.float16)
    if split == 3:
        out["var_w"] = vh.view(torch.int16)            # plain fp16 rows: the first O * ld halves of the buffer
    else:
        out["var_w"] = _units(vh, (Vs - vh.float()).to(torch.float16))
    return out


def _check_operands(got, want, split, tag):
    for k, w in want.items():
        g = got[k]
        if k.endswith("scale") or split == 0:
            g = g.view(torch.int32)
        elif k == "var_w" and split == 3:
            g = g.contiguous().view(torch.int16).reshape(-1)[:w.numel()].view(w.shape)
        else:
            g = g.contiguous().view(torch.int16)
        assert torch.equal(g, w), (tag, k)


_REF = {}


def _reference(bnn, dev, I, O):
    """Per shape, computed once: device parameters (aligned and off-boundary), the generic kernel's outputs with and without
    the per-column vectors, and the fp64 row sums."""
    if (I, O) not in _REF:
        p = _params(I, O)
        d = {k: v.to(dev) for k, v in p.items()}
        d["mu_off"] = _off16(p["mu"], dev)
        gen = {z: _run(bnn, dev, d, O, I, z=z, mu_key="mu_off") for z in (True, False)}
        q = {k: v.double() for k, v in p.items()}
        alpha, sigma = orc.alpha_of(q["lam"]), orc.sigma_of(q["rho"])
        kl_rows = lambda zk: orc.kl_weight_elem(q["mu"] * zk, sigma, alpha, orc.Priors()).sum(1)
        ref = {True: {"kl_rows": kl_rows(q["zk"]), "act_mu": (q["rc"] * q["zk"] * q["mu"] * alpha).sum(1),
                      "act_var": (q["rc"] ** 2 * sigma ** 2 * alpha ** 2).sum(1)},
               False: {"kl_rows": kl_rows(torch.ones(I, dtype=torch.float64))},
               "bias_var": orc.sigma_of(q["brho"]) ** 2}
        _REF[(I, O)] = (d, gen, ref)
    return _REF[(I, O)]


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("O", SHAPES_O)
@pytest.mark.parametrize("I", SHAPES_I)
def test_row_tasks_operands_scales_and_sums(bnn, dev, sums_golden, I, O):
    d, gen, ref = _reference(bnn, dev, I, O)
    for z in (True, False):
        E, V = gen[z]["e_w"], gen[z]["var_w"]
        assert bool((E[:, I:] == 0).all()) and bool((V[:, I:] == 0).all()) and bool(torch.isfinite(E).all())
        first = None
        for split in (0, 1, 2, 3):
            want = _expect(E, V, split)
            for sums in (True, False):
                got = _run(bnn, dev, d, O, I, split=split, z=z, sums=sums)
                tag = (I, O, z, split, sums)
                _check_operands(got, want, split, tag)
                assert _rel(got["bias_var"], ref["bias_var"]) < TIGHT, tag
                if not sums:
                    continue
                names = ("kl_rows", "act_mu", "act_var") if z else ("kl_rows",)
                for k in names:
                    e = _rel(got[k], ref[z][k])
                    print(tag, k, "rel err %.2e" % e)
                    assert e < (2e-5 if k == "act_mu" else TIGHT), (tag, k, e)
                    gold = torch.from_numpy(sums_golden["%s_%d_%d_%s" % (k, I, O, "z" if z else "noz")])
                    assert torch.equal(got[k].view(torch.int32), gold.view(torch.int32)), (tag, k, "golden")
                if first is None:
                    first = got
                    again = _run(bnn, dev, d, O, I, split=split, z=z, sums=True)
                    for k in names:
                        assert torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)), (tag, k, "second call")
                else:
                    for k in names:
                        assert torch.equal(first[k].view(torch.int32), got[k].view(torch.int32)), (tag, k, "across formats")


def test_row_tasks_mixed_format_launch(bnn, dev):
    """One launch that mixes a row-scaled fp16 layer with the fp32 10-row head (the fused fp16 forward's weight pass): every
    layer's operands, scales and row sums are byte-equal to a launch of its own on the z vectors the forward used."""
    bnn.manual_seed(11, 3)
    net = bnn.mnf.BayesianNetwork((784, 96, 10), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
    net.set_precision("fp16x3")
    x = torch.rand(5, 784, device=dev)
    with torch.no_grad():
        net(x, sample=True)
        net.kl()
    torch.cuda.synchronize()
    layers = net._layers()
    assert [l._split_now for l in layers] == [2, 0]
    for l in layers:
        ws = l._workspace()
        O, I = l.out_features, l.in_features
        d = {"mu": l.weight_mu.detach(), "rho": l.weight_rho.detach(), "lam": l.lambdal.detach(), "zf": ws.z_fwd, "zk": ws.z_kl,
             "rc": l.r0_c.detach(), "brho": l.bias_rho.detach()}
        got = _run(bnn, dev, d, O, I, split=l._split_now)
        eq = lambda a, b: torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))
        for k in ("e_w", "var_w", "kl_rows", "act_mu", "act_var", "bias_var") + (("e_scale", "v_scale") if l._split_now else ()):
            assert eq(getattr(ws, k), got[k]), (I, O, k)
    net.set_precision(None)


def test_row_tasks_ensemble_members(bnn, dev):
    """Three ensemble members on gridDim.y: member m's e_w is byte-equal to the generic producer's with member m's z; var_w
    and bias_var are written once."""
    from bnn_amd import _lib, ops
    bnn.manual_seed(12, 5)
    net = bnn.mnf.BayesianNetwork((260, 516, 3), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).eval()
    layers, S = net._layers(), 3
    n = len(layers)
    descs = (_lib.LayerDesc * n)()
    keep, outs = [], []
    for i, l in enumerate(layers):
        l._split_now = 0
        keep.append(l._fill_desc(descs[i], (True, False, i < n - 1), None))
        ld = ops.operand_ld(l.in_features)
        e = torch.full((S, l.out_features, ld), float("nan"), device=dev)
        z = torch.full((S, ld), float("nan"), device=dev)
        descs[i].e_w, descs[i].z_fwd, descs[i].eps_z = e.data_ptr(), z.data_ptr(), None
        outs.append((e, z))
    rng = ops.RngState.get(dev).t
    _lib.check(_lib.lib().lbbnn_ensemble_operands(descs, n, S, rng.data_ptr(), 1, torch.cuda.current_stream(dev).cuda_stream),
               "lbbnn_ensemble_operands")
    torch.cuda.synchronize()
    for l, (e, z) in zip(layers, outs):
        O, I = l.out_features, l.in_features
        ws = l._workspace()
        for m in range(S):
            d = {"mu_off": _off16(l.weight_mu.detach(), dev), "rho": l.weight_rho.detach(), "lam": l.lambdal.detach(),
                 "zf": z[m, :I].contiguous(), "brho": l.bias_rho.detach()}
            gen = _run(bnn, dev, d, O, I, z=True, sums=False, mu_key="mu_off")
            assert torch.equal(e[m].cpu().view(torch.int32), gen["e_w"].view(torch.int32)), (I, O, m)
            assert torch.equal(ws.var_w.cpu().view(torch.int32), gen["var_w"].view(torch.int32)), (I, O, m)
            assert torch.equal(ws.bias_var.cpu().view(torch.int32), gen["bias_var"].view(torch.int32)), (I, O, m)
    del keep


def _record(path):
    """Row sums of every shape as THIS build computes them -> path (run on the build the fixtures are to pin)."""
    import bnn_amd
    dev, out = torch.device("cuda:0"), {}
    for I in SHAPES_I:
        for O in SHAPES_O:
            d = {k: v.to(dev) for k, v in _params(I, O).items()}
            for z in (True, False):
                got = _run(bnn_amd, dev, d, O, I, z=z)
                for k in ("kl_rows", "act_mu", "act_var") if z else ("kl_rows",):
                    out["%s_%d_%d_%s" % (k, I, O, "z" if z else "noz")] = got[k].numpy()
    np.savez(path, **out)
    print("recorded %d arrays -> %s" % (len(out), path))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "record":
    _record(sys.argv[2])
