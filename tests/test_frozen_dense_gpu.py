"""GPU tier of the frozen evaluation model for RNVP / MNF-type z flows (evaluate.freeze(net, gates, dense=True);
include/lbbnn.h lbbnn_flow_dense_members + lbbnn_frozen_members_dense).

1. the members' draws are the loop's, bit for bit: the masks equal philox_bits_ref.mask_bits at offset live + m AND the
   masks the single forward at that offset used; the offset ends at live + S;
2. every member's z against orc.mnf_sample_z in float64 on philox_ref.normal_vector and those masks: rel_err < TIGHT for
   layers of at most 784 inputs (the bar K4r, the same matrix-core arithmetic, is held to); for the 1200-wide layers no
   bar is known, so the single forward's own z is measured against the same fp64 value in the same test and
   err_new <= max(TIGHT, 2 * err_loop) is required (two fp32 sums in different orders scatter independently around the
   exact value);
3. every member's outputs (gates alpha, mpm at 0.5 and 0.1) and the posterior-mean branch against the fp64 oracle on the
   same eps_z, masks and eps_out: rel_err < TOL (the contract) and the element-wise form;
4. the alpha model against the loop of single forwards, both measured against fp64: err_new <= max(BAR, 2 * err_loop);
   never asserted bitwise equal (another summation order), no argmax compared;
5. housekeeping: chunks, single forward, kept_rows / density, snapshot / refresh, NaN-filled buffers, ensemble_eval,
   predictive_entropy, ensemble_forward(batched=True), a planar network with dense=True.

Inputs: lambdal ~ N(0, 2) (both sides of either cut; asserted), q0_mean = 1 + 0.1 N(0,1), q0_log_var = -6 + 0.5 N(0,1)
(z around 1 with a visible draw; the device normals are within 2e-5 of philox_ref's, tests/test_philox_ref.py, so with
std ~ 0.05 the fp64 z of test 2 is good to ~1e-6 of max|z|).  Members S in {1, 10, 17, 33}, batches B in {0, 1, 100}: every
combination, every member, every row."""
import pytest
import torch

import philox_ref
from conftest import elementwise_violation, rel_err
from oracle import lbbnn_oracle as orc
from philox_bits_ref import mask_bits

pytestmark = pytest.mark.gpu

TOL = 1e-4
TIGHT = 5e-6
BAR = {"fp32": TIGHT, "bf16x3": 2e-5}

# (z / r flow kind, dims, transforms)
NETS = [("RNVP", (784, 1200, 1200, 10), 2), ("RNVP", (784, 400, 600, 10), 2), ("MNF", (784, 96, 64, 10), 2),
        ("RNVP", (20, 16, 12, 3), 1), ("MNF", (4, 8, 4, 2), 8)]
IDS = ["%s-%s-T%d" % (k, "-".join(map(str, d)), t) for k, d, t in NETS]
SS = [1, 10, 17, 33]
BS = [0, 1, 100]
SMAX = max(SS)
SEED, OFF = 3, 5
GATES = [("alpha", 0.5), ("mpm", 0.5), ("mpm", 0.1)]

_CACHE = {}          # fp64 results, shared by the precisions and the tests (same seeds -> same inputs)


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


def _cut(threshold):
    return float(torch.logit(torch.tensor(threshold, dtype=torch.float64)).float())


def _net(bnn, dev, kind, dims, T, seed=11):
    torch.manual_seed(seed)
    net = bnn.mnf.BayesianNetwork(dims, T, z_flow_type=kind, r_flow_type=kind)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for l in _layers(net):
            O, I = l.out_features, l.in_features
            l.lambdal.copy_(2.0 * torch.randn(O, I, generator=g))
            l.q0_mean.copy_(1.0 + 0.1 * torch.randn(I, generator=g))
            l.q0_log_var.copy_(-6.0 + 0.5 * torch.randn(I, generator=g))
            for thr in (0.5, 0.1):                          # the median model is neither empty nor full
                kept = int((l.lambdal > _cut(thr)).sum())
                assert 0 < kept < O * I, (O, I, thr, kept)
    return net.to(dev).eval()


def _x(dev, B, I, seed=1):
    return torch.rand(B, I, generator=torch.Generator().manual_seed(seed + B)).to(dev)


def _key(kind, dims, T, *rest):
    return (kind, tuple(dims), T) + tuple(rest)


def _state(net, kind, T):
    """Per layer the float64 CPU parameters and the z flow of the oracle."""
    P, zf = [], []
    for l in _layers(net):
        sd = {k: v.detach().double().cpu() for k, v in l.state_dict().items()}
        P.append(sd)
        zf.append(orc.flow_from_state("z_flow", kind, sd, T))
    return P, zf


def _masks_ref(net, m):
    """Per layer (T, I): the masks of member m by the draw contract."""
    return [torch.from_numpy(mask_bits(SEED, OFF + m, l._layer_id, l.in_features, len(l.z_flow.transforms)))
            for l in _layers(net)]


def _z64(bnn, net, kind, dims, T, m):
    """Member m's z per layer in float64 (orc.mnf_sample_z on philox_ref.normal_vector and the masks of the contract)."""
    key = _key(kind, dims, T, "z", m)
    if key not in _CACHE:
        P, zf = _state(net, kind, T)
        out = []
        for l, p, f, mk in zip(_layers(net), P, zf, _masks_ref(net, m)):
            I = l.in_features
            eps = torch.from_numpy(philox_ref.normal_vector(SEED, OFF + m, bnn.ops.STREAM_EPS_Z * 64 + l._layer_id, I))
            z, _, _ = orc.mnf_sample_z(p, eps.reshape(1, I), f, [r.double().reshape(1, I) for r in mk])
            out.append(z)
        _CACHE[key] = out
    return _CACHE[key]


def _out64(bnn, net, kind, dims, T, x, m, gates, threshold, stochastic=True):
    """Member m's outputs in float64: the same eps_z (the device's draw), masks and eps_out, handed to the oracle as
    one-row (1, I) draws; gates = alpha, or lambdal > logit(threshold) as +-1000 (fp64 alpha exactly 1 / 0)."""
    B = x.shape[0]
    key = _key(kind, dims, T, "out", B, m, gates, threshold, stochastic)
    if key in _CACHE:
        return _CACHE[key]
    ops, dev = bnn.ops, x.device
    P, zf = _state(net, kind, T)
    rng_m = torch.tensor([SEED, OFF + m, 0, 0], dtype=torch.int64, device=dev)
    noise = []
    for l, p, mk in zip(_layers(net), P, _masks_ref(net, m)):
        I, O, L = l.in_features, l.out_features, l._layer_id
        if gates == "mpm":
            keep = l.lambdal.detach().cpu() > _cut(threshold)                  # compared in fp32, as the kernel does
            p["lambdal"] = torch.where(keep, 1000.0, -1000.0).double()
            a = orc.alpha_of(p["lambdal"])
            assert bool(((a == 0) | (a == 1)).all())
        n = {"eps_z": ops.philox_normal(rng_m, ops.STREAM_EPS_Z * 64 + L, 0, I).double().cpu().reshape(1, I),
             "zmask": [r.double().reshape(1, I) for r in mk]}
        if stochastic:
            n["eps_out"] = ops.philox_normal(rng_m, ops.STREAM_EPS_OUT * 64 + L, B, O, row_base=l.row_offset).double().cpu()
        noise.append(n)
    out, _ = orc.mnf_network_forward(x.double().cpu(), P, zf, [None] * 3, noise, stochastic=stochastic, compute_kl=False)
    _CACHE[key] = out
    return out


def _single_forward(bnn, net, x, m):
    """The loop's m-th forward: (outputs, per layer the masks it used (T, I), per layer its z)."""
    bnn.manual_seed(SEED, OFF + m)
    with torch.no_grad():
        out = net(x, sample=True).clone()
    masks = [torch.stack([v.reshape(-1) for v in l._last_masks["zmask"]]).clone() for l in _layers(net)]
    z = [l._workspace().z_fwd[:l.in_features].clone() for l in _layers(net)]
    return out, masks, z


# --------------------------------------------------------------------------- 1. the draws are the loop's
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kind,dims,T", NETS, ids=IDS)
def test_member_draws_are_the_loops_bit_for_bit(bnn, dev, precision, kind, dims, T, prec):
    ev = bnn.evaluate
    net = _net(bnn, dev, kind, dims, T)
    precision(prec)
    fz = ev.freeze(net, "alpha", dense=True)
    assert fz.flows == "dense" and fz.family == "mnf" and list(fz.parameters()) == []
    st = bnn.ops.RngState.get(dev)
    loop = [_single_forward(bnn, net, _x(dev, 1, dims[0]), m) for m in range(SMAX)]
    for i, l in enumerate(_layers(net)):
        assert l._last_masks["_in_kernel"]
    ref = [_masks_ref(net, m) for m in range(SMAX)]
    for B in BS:
        x = _x(dev, B, dims[0])
        for S in SS:
            bnn.manual_seed(SEED, OFF)
            out = fz.ensemble(x, S, keep_z=True, keep_masks=True)
            assert int(st.t[1]) == OFF + S
            assert out.shape == (S, B, dims[-1])
            assert [tuple(t.shape) for t in fz.last_masks] == [(S, T, I) for I in dims[:-1]]
            assert [tuple(t.shape) for t in fz.last_z] == [(S, I) for I in dims[:-1]]
            for i in range(3):
                got = fz.last_masks[i].cpu()
                for m in range(S):
                    assert torch.equal(got[m], ref[m][i]), (B, S, i, m)
                    assert torch.equal(got[m], loop[m][1][i].cpu()), (B, S, i, m)
                if S > 1:
                    assert not torch.equal(got[0], got[1])
                    assert not torch.equal(fz.last_z[i][0], fz.last_z[i][1])


# --------------------------------------------------------------------------- 2. z against fp64
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kind,dims,T", NETS, ids=IDS)
def test_member_z_against_fp64(bnn, dev, precision, kind, dims, T, prec):
    """Bars in the module docstring; the measured pairs (err_new, err_loop) are printed and recorded in DESIGN.md."""
    ev = bnn.evaluate
    net = _net(bnn, dev, kind, dims, T)
    precision(prec)
    fz = ev.freeze(net, "mpm", dense=True)                   # (z is not gated: the gates mode must not matter)
    loop = [_single_forward(bnn, net, _x(dev, 1, dims[0]), m) for m in range(SMAX)]
    worst = {}
    for B in BS:
        x = _x(dev, B, dims[0])
        for S in SS:
            bnn.manual_seed(SEED, OFF)
            fz.ensemble(x, S, keep_z=True)
            for m in range(S):
                ref = _z64(bnn, net, kind, dims, T, m)
                for i, I in enumerate(dims[:-1]):
                    e_new, e_loop = rel_err(fz.last_z[i][m], ref[i]), rel_err(loop[m][2][i], ref[i])
                    w = worst.setdefault(I, [0.0, 0.0])
                    w[0], w[1] = max(w[0], e_new), max(w[1], e_loop)
                    bar = TIGHT if I <= 784 else max(TIGHT, 2 * e_loop)
                    assert e_new < bar if I <= 784 else e_new <= bar, (B, S, m, i, e_new, e_loop)
    for I, (a, b) in sorted(worst.items()):
        print("z-vs-fp64 %s %s %s I=%d err_new %.3g err_loop %.3g" % (kind, dims, prec, I, a, b))


# --------------------------------------------------------------------------- 3. outputs against fp64
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kind,dims,T", NETS, ids=IDS)
def test_member_outputs_against_fp64(bnn, dev, precision, kind, dims, T, prec):
    ev = bnn.evaluate
    net = _net(bnn, dev, kind, dims, T)
    precision(prec)
    for gates, thr in GATES:
        fz = ev.freeze(net, gates, threshold=thr, dense=True)
        worst = 0.0
        for B in BS:
            x = _x(dev, B, dims[0])
            for S in SS:
                bnn.manual_seed(SEED, OFF)
                out = fz.ensemble(x, S)
                assert out.shape == (S, B, dims[-1])
                if B == 0:
                    continue                                # no rows: the shape is the whole statement
                assert bool(torch.isfinite(out).all())
                for m in range(S):
                    ref = _out64(bnn, net, kind, dims, T, x, m, gates, thr)
                    e, v = rel_err(out[m], ref), elementwise_violation(out[m], ref)
                    worst = max(worst, e)
                    assert e < TOL and v <= 1.0, (gates, thr, B, S, m, e, v)
            if B:
                # sample=False: the mean branch, z drawn at the live offset (member 0's)
                bnn.manual_seed(SEED, OFF)
                out0 = fz(x, sample=False)
                assert int(bnn.ops.RngState.get(dev).t[1]) == OFF + 1
                ref0 = _out64(bnn, net, kind, dims, T, x, 0, gates, thr, stochastic=False)
                e, v = rel_err(out0, ref0), elementwise_violation(out0, ref0)
                assert out0.shape == (B, dims[-1]) and e < TOL and v <= 1.0, (gates, thr, B, e, v)
        print("out-vs-fp64 %s %s %s gates=%s@%g worst rel_err %.3g" % (kind, dims, prec, gates, thr, worst))


# --------------------------------------------------------------------------- 4. the alpha model against the loop
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kind,dims,T", NETS, ids=IDS)
def test_alpha_model_against_the_loop(bnn, dev, precision, kind, dims, T, prec):
    """Same seed and offset, both sides against the fp64 value of test 3; the measured pairs are printed and recorded in
    DESIGN.md."""
    ev = bnn.evaluate
    net = _net(bnn, dev, kind, dims, T)
    precision(prec)
    fz = ev.freeze(net, "alpha", dense=True)
    st = bnn.ops.RngState.get(dev)
    worst = [0.0, 0.0]
    for B in BS:
        x = _x(dev, B, dims[0])
        for S in SS:
            bnn.manual_seed(SEED, OFF)
            new = fz.ensemble(x, S)
            assert int(st.t[1]) == OFF + S
            bnn.manual_seed(SEED, OFF)
            with torch.no_grad():
                loop = torch.stack([net(x, sample=True) for _ in range(S)])
            assert int(st.t[1]) == OFF + S
            assert new.shape == loop.shape == (S, B, dims[-1])
            if B == 0:
                continue
            ref = torch.stack([_out64(bnn, net, kind, dims, T, x, m, "alpha", 0.5) for m in range(S)])
            e_new, e_loop = rel_err(new, ref), rel_err(loop, ref)
            worst = [max(worst[0], e_new), max(worst[1], e_loop)]
            assert e_new <= max(BAR[prec], 2 * e_loop), (B, S, e_new, e_loop)
    print("alpha-vs-loop %s %s %s err_new %.3g err_loop %.3g" % (kind, dims, prec, worst[0], worst[1]))


# --------------------------------------------------------------------------- 5. housekeeping
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kind,dims,T", NETS, ids=IDS)
def test_chunks_single_forward_and_counts(bnn, dev, precision, kind, dims, T, prec):
    ev = bnn.evaluate
    net = _net(bnn, dev, kind, dims, T)
    precision(prec)
    st = bnn.ops.RngState.get(dev)
    for gates, thr in GATES:
        fz = ev.freeze(net, gates, threshold=thr, dense=True)
        total = 0
        for i, l in enumerate(_layers(net)):
            rows = (l.lambdal.detach().cpu() > torch.tensor(_cut(thr), dtype=torch.float32)).sum(1)
            assert torch.equal(fz.kept_rows[i].cpu().long(), rows)
            total += int(rows.sum())
        assert fz.density == total / sum(dims[i] * dims[i + 1] for i in range(3))
        for B in BS:
            x = _x(dev, B, dims[0])
            for S in (17, 33):
                bnn.manual_seed(SEED, OFF)
                whole = fz.ensemble(x, S, keep_z=True, keep_masks=True)
                z_whole, m_whole = fz.last_z, fz.last_masks
                for mm in (1, 5, 16):
                    bnn.manual_seed(SEED, OFF)
                    part = fz.ensemble(x, S, max_members=mm, keep_z=True, keep_masks=True)
                    assert int(st.t[1]) == OFF + S
                    assert torch.equal(part, whole), (gates, B, S, mm)
                    for a, b in zip(fz.last_z + fz.last_masks, z_whole + m_whole):
                        assert torch.equal(a, b)
                    bnn.manual_seed(SEED, OFF)
                    assert torch.equal(ev.ensemble_forward(fz, x, S, max_members=mm), whole)
                if B:
                    for m in range(1, S):
                        assert not torch.equal(whole[m], whole[0])
            bnn.manual_seed(SEED, OFF)
            one = fz.ensemble(x, 1)
            assert torch.equal(one[0], whole[0])
            bnn.manual_seed(SEED, OFF)
            single = fz(x, sample=True)
            assert int(st.t[1]) == OFF + 1
            assert single.shape == (B, dims[-1]) and torch.equal(single, one[0])


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kind,dims,T", NETS, ids=IDS)
def test_snapshot_and_refresh(bnn, dev, precision, kind, dims, T, prec):
    ev = bnn.evaluate
    precision(prec)
    for gates in ("alpha", "mpm"):
        net = _net(bnn, dev, kind, dims, T)
        x = _x(dev, 100, dims[0])
        fz = ev.freeze(net, gates, dense=True)
        names = [k for k, _ in fz.named_buffers()]
        for tr in net.l1.z_flow.transforms:                  # every coupling parameter has its copy
            assert len([k for k in names if k.startswith("zflow_0_0_")]) == len(list(tr.parameters()))
        assert not any("r_flow" in k or k.startswith("rflow") for k in names)
        ptrs = {k: v.data_ptr() for k, v in fz.named_buffers()}
        bnn.manual_seed(SEED, OFF)
        before = fz.ensemble(x, 3)
        kept_before = fz.kept
        head = "t" if kind == "RNVP" else "g"
        with torch.no_grad():
            for l in _layers(net):
                for tr in l.z_flow.transforms:
                    getattr(tr, head).weight.add_(0.05)
                    getattr(tr, head).bias.add_(0.5)
                l.lambdal.neg_()
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(fz.ensemble(x, 3), before)                     # the frozen model did not follow
        assert fz.kept == kept_before
        assert fz.refresh() is fz
        assert {k: v.data_ptr() for k, v in fz.named_buffers()} == ptrs   # into the same buffers
        bnn.manual_seed(SEED, OFF)
        after = fz.ensemble(x, 3, keep_z=True)
        z_after = fz.last_z
        assert not torch.equal(after, before)
        fresh = ev.freeze(net, gates, dense=True)
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(fresh.ensemble(x, 3, keep_z=True), after)
        for a, b in zip(fresh.last_z, z_after):
            assert torch.equal(a, b)
        assert fresh.kept == fz.kept and fz.kept != kept_before


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kind,dims,T", NETS, ids=IDS)
def test_nan_filled_buffers(bnn, dev, precision, monkeypatch, kind, dims, T, prec):
    """Every buffer of the frozen model (operands, coupling-network copies, z, masks, member operands, hidden activations,
    outputs) is handed out full of NaN: an element the kernels read without having written it would surface."""
    ev = bnn.evaluate
    net = _net(bnn, dev, kind, dims, T)
    precision(prec)
    x = _x(dev, 100, dims[0])
    clean = {}
    for gates in ("alpha", "mpm"):
        bnn.manual_seed(SEED, OFF)
        fz = ev.freeze(net, gates, dense=True)
        out = fz.ensemble(x, 19, max_members=17, keep_z=True, keep_masks=True)
        clean[gates] = (out, fz.last_z, fz.last_masks)

    def nan_empty(*size, **kw):
        return torch.full(*size, float("nan"), **kw)
    monkeypatch.setattr(ev, "_empty", nan_empty)
    for gates in ("alpha", "mpm"):
        fz = ev.freeze(net, gates, dense=True)
        for k, v in fz.named_buffers():
            if v.is_floating_point():
                assert bool(torch.isfinite(v).all()), k
        bnn.manual_seed(SEED, OFF)
        out = fz.ensemble(x, 19, max_members=17, keep_z=True, keep_masks=True)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out, clean[gates][0])
        for a, b in zip(fz.last_z + fz.last_masks, clean[gates][1] + clean[gates][2]):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(fz(x, sample=False)).all())


@pytest.mark.parametrize("kind,dims,T", NETS, ids=IDS)
def test_ensemble_eval_entropy_and_batched_form(bnn, dev, kind, dims, T):
    ev = bnn.evaluate
    net = _net(bnn, dev, kind, dims, T)
    fz = ev.freeze(net, "mpm", dense=True)
    B, S, C = 100, 10, dims[-1]
    x = _x(dev, B, dims[0])
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(2)).to(dev)
    bnn.manual_seed(SEED, OFF)
    r = ev.ensemble_eval(fz, x, y, S)
    assert set(r) == {"outputs", "pred_ensemble", "pred_posterior_mean", "density", "correct_ensemble",
                      "correct_posterior_mean"}
    assert r["outputs"].shape == (S, B, C) and r["pred_ensemble"].shape == (B,) and r["pred_posterior_mean"].shape == (B,)
    assert r["density"].shape == (S,) and bool((r["density"] == torch.tensor(fz.density, dtype=torch.float32)).all())
    assert rel_err(r["outputs"].exp().sum(-1), torch.ones(S, B)) < 1e-5      # log-probabilities
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(fz.ensemble(x, S), r["outputs"])
    h = ev.predictive_entropy(r["outputs"])
    assert h.shape == (B,) and bool(torch.isfinite(h).all())
    # ensemble_forward(batched=True) on the network itself is the frozen alpha model; batched=None keeps the loop's bits
    st = bnn.ops.RngState.get(dev)
    for S in SS:
        bnn.manual_seed(SEED, OFF)
        a = ev.ensemble_forward(net, x, S, batched=True)
        assert int(st.t[1]) == OFF + S
        bnn.manual_seed(SEED, OFF)
        b = ev.freeze(net, "alpha", dense=True).ensemble(x, S)
        assert torch.equal(a, b)
        bnn.manual_seed(SEED, OFF)
        c = ev.ensemble_forward(net, x, S)
        bnn.manual_seed(SEED, OFF)
        with torch.no_grad():
            d = torch.stack([net(x, sample=True) for _ in range(S)])
        assert torch.equal(c, d)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("family,dims,T", [("mnf", (784, 400, 600, 10), 2), ("mnf", (20, 16, 12, 3), 4),
                                           ("lrt", (784, 400, 600, 10), 0)])
def test_planar_and_lrt_networks_with_dense_flag_keep_their_bits(bnn, dev, precision, family, dims, T, prec):
    ev = bnn.evaluate
    torch.manual_seed(11)
    net = bnn.lrt.BayesianNetwork(dims) if family == "lrt" else \
        bnn.mnf.BayesianNetwork(dims, T, z_flow_type="Planar", r_flow_type="Planar")
    net = net.to(dev).eval()
    with torch.no_grad():
        for l in _layers(net):
            l.lambdal.normal_(0, 2)
    precision(prec)
    x = _x(dev, 100, dims[0])
    for gates in ("alpha", "mpm"):
        a, b = ev.freeze(net, gates), ev.freeze(net, gates, dense=True)
        assert a.flows == b.flows == ("planar" if family == "mnf" else None)
        assert [k for k, _ in a.named_buffers()] == [k for k, _ in b.named_buffers()]
        for S in (10, 17):
            bnn.manual_seed(SEED, OFF)
            oa = a.ensemble(x, S, keep_z=True)
            bnn.manual_seed(SEED, OFF)
            ob = b.ensemble(x, S, keep_z=True, keep_masks=True)
            assert torch.equal(oa, ob) and b.last_masks is None
            for za, zb in zip(a.last_z, b.last_z):
                assert (za is None and zb is None) or torch.equal(za, zb)


def test_a_copied_or_moved_model_addresses_its_own_buffers(bnn, dev):
    """The transforms of the dense z flows are arrays of device addresses, and the member buffers are kept across calls: a deep
    copy, or a model moved or cast, must address its own buffers.  (16, 12, 3): two layers with in_features % 4 == 0, the
    smallest model whose transforms cover more than one layer."""
    import copy
    ev = bnn.evaluate
    torch.manual_seed(11)
    net = bnn.mnf.BayesianNetwork((16, 12, 3), 2, z_flow_type="RNVP", r_flow_type="RNVP").to(dev).eval()
    fz = ev.freeze(net, "alpha", dense=True)
    B, S = 5, 3
    x = _x(dev, B, 16)
    bnn.manual_seed(SEED, OFF)
    want = fz.ensemble(x, S)
    assert want.shape == (S, B, 3) and bool(torch.isfinite(want).all())
    twin = copy.deepcopy(fz)
    poisoned = [b.fill_(float("nan")) for k, b in fz.named_buffers() if k.startswith(("zflow_", "q0_", "e0_"))]
    assert len(poisoned) > 6                                      # the original's flows and operands are no longer usable
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(twin.ensemble(x, S), want)
    old = dict(twin.named_buffers())
    moved = twin.double().float()                                # every float buffer replaced (a cast leaves int32 ones in place)
    for k, b in moved.named_buffers():
        if b.is_floating_point():
            assert b.data_ptr() != old[k].data_ptr(), k
            old[k].fill_(float("nan"))                           # still alive: a stale address reads NaN, not freed memory
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(moved.ensemble(x, S), want)
    with pytest.raises(RuntimeError, match="data is on"):
        moved.cpu().ensemble(x, S)
