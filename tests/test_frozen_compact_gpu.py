"""GPU tier of the compact median-probability model (evaluate.freeze(net, "mpm", compact=True) / CompactFrozenNetwork;
include/lbbnn.h lbbnn_frozen_operands_compact, lbbnn_frozen_members_compact, lbbnn_gather_columns): the compact operands are
the full model's, gathered, bit for bit; the posterior mean equals the full model's; every stochastic member equals the fp64
oracle on the regenerated draws (eps_out indexed by the COMPACT column, scattered to the live units); chunking changes no
bit; every byte read was written; the evaluation stack takes a compact model; the input gather is exact and absent when no
input is unneeded.

Bars (tests/test_frozen_gpu.py): TOL = 1e-4 the contract plus the element-wise form against fp64; BAR = 5e-6 for fp32
operands, 2e-5 for bf16x3, as rel_err.  Inputs: tests/frozen_compact_cases.py."""
import pytest
import torch

import frozen_compact_cases as cc
from conftest import elementwise_violation, rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4
BAR = {"fp32": 5e-6, "bf16x3": 2e-5}
SEED, OFF = 3, 5
PRECS = ["fp32", "bf16x3"]


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


_NETS = {}


def _net(bnn, dev, case):
    """The network of a case with the shared lambdal applied, and its keep masks (built once per module, never changed)."""
    if case not in _NETS:
        family, dims, T, head = case
        torch.manual_seed(11)
        if family == "lrt":
            net = bnn.lrt.BayesianNetwork(dims, head=head)
        else:
            net = bnn.mnf.BayesianNetwork(dims, T, z_flow_type="Planar", r_flow_type="Planar", head=head)
        net = net.to(dev).eval()
        lams, masks = cc.lambdals(dims)
        cc.apply(net, lams)
        _NETS[case] = (net, masks)
    return _NETS[case]


def _x(dev, B, I, seed=1):
    return torch.rand(B, I, generator=torch.Generator().manual_seed(seed + B)).to(dev)


def _live(masks):
    need = cc.brute_need(masks)
    sizes = cc.expected_live_sizes(need)
    live = []
    for nd, s in zip(need, sizes):
        dead = torch.nonzero(~nd).reshape(-1)
        live.append(torch.sort(torch.cat([torch.nonzero(nd).reshape(-1), dead[:s - int(nd.sum())]])).values)
    return need, live


# --------------------------------------------------------------------------- 1. operands
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_compact_operands_are_the_full_operands_gathered(bnn, dev, precision, case, prec):
    ev, ops = bnn.evaluate, bnn.ops
    family, dims, T, head = case
    net, masks = _net(bnn, dev, case)
    n = len(dims) - 1
    full = ev.freeze(net, "mpm")                                             # fp32 operands: plain rows to gather from
    precision(prec)
    fz = ev.freeze(net, "mpm", compact=True)
    need, live = _live(masks)
    assert isinstance(fz, ev.CompactFrozenNetwork) and isinstance(fz, ev.FrozenNetwork)
    assert fz.full_dims == tuple(dims) and fz.dims == tuple(t.numel() for t in live) and fz.head == head
    assert fz.needed == [int(nd.sum()) for nd in need]
    assert [t.cpu().long().tolist() for t in fz.live] == [t.tolist() for t in live]
    assert all(t.dtype == torch.int32 and t.is_cuda for t in fz.live)
    active = sum(int((k & need[i + 1][:, None] & need[i][None, :]).sum()) for i, k in enumerate(masks))
    total = sum(dims[i] * dims[i + 1] for i in range(n))
    assert fz.active_kept == active and fz.active_density == active / total
    assert fz.density == full.density == sum(int(k.sum()) for k in masks) / total
    assert 0 < fz.active_density <= fz.density and (n == 1 or fz.active_density < fz.density)   # (one layer: every kept weight is active)
    with pytest.raises(NotImplementedError, match="freeze again"):
        fz.refresh()
    for i in range(n):
        rows, cols = live[i + 1], live[i]
        O, I = rows.numel(), cols.numel()
        ld = ops.operand_ld(I)
        e0 = getattr(fz, "e0_%d" % i).cpu()
        ref_e0 = getattr(full, "e0_%d" % i).cpu()[rows][:, cols]
        ref_var = getattr(full, "var_w_%d" % i).cpu()[rows][:, cols]
        assert e0.shape == (O, ld)
        assert torch.equal(e0[:, :I], ref_e0), i
        assert bool((e0[:, I:] == 0).all())                                  # the zero tail
        e_w, var_w = getattr(fz, "e_w_%d" % i), getattr(fz, "var_w_%d" % i)
        assert fz._split[i] == (prec != "fp32" and ops.split_eligible(I, O) and (i == 0 or I % 4 == 0))
        if not fz._split[i]:
            assert torch.equal(e_w.cpu(), e0)
            assert torch.equal(var_w.cpu()[:, :I], ref_var) and bool((var_w.cpu()[:, I:] == 0).all())
        else:                                                                # the bf16 hi | lo units of the same values
            assert torch.equal(e_w.view(torch.int32), ops.format_operand(ref_e0.to(dev), split=True).view(torch.int32)), i
            assert torch.equal(var_w.view(torch.int32), ops.format_operand(ref_var.to(dev), split=True).view(torch.int32)), i
        assert torch.equal(fz.kept_rows[i].cpu().long(), masks[i][rows][:, cols].sum(1)), i
        assert fz.kept_rows[i].dtype == torch.int32
        assert torch.equal(getattr(fz, "bias_var_%d" % i).cpu(), getattr(full, "bias_var_%d" % i).cpu()[rows])
        assert torch.equal(getattr(fz, "bias_mu_%d" % i).cpu(), getattr(full, "bias_mu_%d" % i).cpu()[rows])
    if dims == (20, 16, 12, 3):
        assert not any(fz._split)                                            # every compact O <= 16: fp32 throughout


# --------------------------------------------------------------------------- 2. posterior mean against the full model
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_posterior_mean_equals_the_full_model(bnn, dev, precision, case, prec):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _ = _net(bnn, dev, case)
    precision(prec)
    full, fz = ev.freeze(net, "mpm"), ev.freeze(net, "mpm", compact=True)
    st = bnn.ops.RngState.get(dev)
    for B in (1, 100, 257):
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        ref = full(x, sample=False)
        bnn.manual_seed(SEED, OFF)
        out = fz(x, sample=False)
        assert int(st.t[1]) == OFF + (1 if family == "mnf" else 0)
        e = rel_err(out, ref)
        print("compact-mean-vs-full %s %s %s B=%d rel_err %.3g" % (family, dims, prec, B, e))
        assert out.shape == ref.shape == (B, dims[-1]) and e < BAR[prec], (B, e)
    if family == "mnf":                                                      # z: the full model's, bit for bit, at full width
        x = _x(dev, 100, dims[0])
        for S in (1, 10):
            bnn.manual_seed(SEED, OFF)
            full.ensemble(x, S, keep_z=True)
            bnn.manual_seed(SEED, OFF)
            fz.ensemble(x, S, keep_z=True)
            assert [tuple(z.shape) for z in fz.last_z] == [(S, I) for I in dims[:-1]]
            for a, b in zip(fz.last_z, full.last_z):
                assert torch.equal(a, b)
            if S > 1:
                assert not torch.equal(fz.last_z[0][0], fz.last_z[0][1])


# --------------------------------------------------------------------------- 3. stochastic members against fp64
def _oracle_member(bnn, fz, net, masks, x, m, stochastic, z_used):
    """Member m of the FULL network in float64: lambdal = +-1000 (fp64 alpha exactly 1 / 0), the full-width z the member
    used, and the eps of layer i regenerated at the COMPACT width -- stream STREAM_EPS_OUT * 64 + layer id, the layer's
    row_offset, Philox offset OFF + m -- scattered into the live columns of a full-width matrix (zeros elsewhere)."""
    ops, dev = bnn.ops, x.device
    rng_m = torch.tensor([SEED, OFF + m], dtype=torch.int64, device=dev)
    layers = net._layers()
    n = len(layers)
    live = [t.cpu().long() for t in fz.live]
    h = x.double().cpu()
    ident = orc.Flow("Planar", [])
    for i, (l, keep) in enumerate(zip(layers, masks)):
        p = {k: getattr(l, k).detach().double().cpu() for k in ("weight_mu", "weight_rho", "bias_mu", "bias_rho")}
        p["lambdal"] = torch.where(keep, 1000.0, -1000.0).double()
        a = orc.alpha_of(p["lambdal"])
        assert bool(((a == 0) | (a == 1)).all())
        eps = None
        if stochastic:
            e_c = ops.philox_normal(rng_m, ops.STREAM_EPS_OUT * 64 + l._layer_id, x.shape[0], fz.dims[i + 1],
                                    row_base=l.row_offset).double().cpu()
            eps = torch.zeros(x.shape[0], l.out_features, dtype=torch.float64)
            eps[:, live[i + 1]] = e_c
        if fz.family == "mnf":
            p["q0_mean"] = z_used[i][m].double().cpu()                       # z0 = q0_mean + 0 * eps_z, no transforms: z itself
            p["q0_log_var"] = torch.full_like(p["q0_mean"], -float("inf"))
            noise = {"eps_z": torch.zeros(1, l.in_features, dtype=torch.float64), "eps_out": eps}
            h, _, _ = orc.mnf_forward(h, p, ident, None, noise, stochastic=stochastic, compute_kl=False)
        else:
            h, _, _ = orc.lrt_forward(h, p, eps, stochastic=stochastic, compute_kl=False)
        if i < n - 1:
            h = torch.relu(h)
    return torch.sigmoid(h) if fz.head == "sigmoid" else torch.log_softmax(h, dim=1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_members_against_fp64_oracle(bnn, dev, precision, case, prec):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, masks = _net(bnn, dev, case)
    precision(prec)
    fz = ev.freeze(net, "mpm", compact=True)
    n = len(dims) - 1
    for B, S in [(100, 10), (257, 1), (1, 10)]:
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        out = fz.ensemble(x, S, keep_z=True)
        z = fz.last_z
        assert out.shape == (S, B, dims[-1])
        if family == "mnf":
            assert [tuple(t.shape) for t in z] == [(S, I) for I in dims[:-1]]
        else:
            assert z == [None] * n
        if S > 1:
            assert not torch.equal(out[0], out[1])
        for m in range(S):
            ref = _oracle_member(bnn, fz, net, masks, x, m, True, z)
            e, v = rel_err(out[m], ref), elementwise_violation(out[m], ref)
            if m == 0:
                print("compact-vs-fp64 %s %s %s B=%d rel_err %.3g elementwise %.3g" % (family, dims, prec, B, e, v))
            assert e < TOL and v <= 1.0, (B, m, e, v)
    x = _x(dev, 100, dims[0])                                                # the posterior mean against fp64 too
    bnn.manual_seed(SEED, OFF)
    fz.ensemble(x, 1, keep_z=True)
    z = fz.last_z
    bnn.manual_seed(SEED, OFF)
    out0 = fz(x, sample=False)
    ref0 = _oracle_member(bnn, fz, net, masks, x, 0, False, z)
    e, v = rel_err(out0, ref0), elementwise_violation(out0, ref0)
    print("compact-mean-vs-fp64 %s %s %s rel_err %.3g elementwise %.3g" % (family, dims, prec, e, v))
    assert e < TOL and v <= 1.0, (e, v)


# --------------------------------------------------------------------------- 4. chunks, offsets, forward
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_chunks_offsets_and_single_forward(bnn, dev, precision, case, prec):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _ = _net(bnn, dev, case)
    precision(prec)
    fz = ev.freeze(net, "mpm", compact=True)
    st = bnn.ops.RngState.get(dev)
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
            assert torch.equal(part, whole), (B, mm)
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


# --------------------------------------------------------------------------- 5. every byte read was written
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_nan_filled_buffers(bnn, dev, precision, monkeypatch, case, prec):
    """Every buffer of the compact model (operands, member operands, z, the gathered input, hidden activations, outputs) is
    handed out full of NaN: a byte the kernels read without having written it would surface in the outputs."""
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _ = _net(bnn, dev, case)
    precision(prec)
    x = _x(dev, 100, dims[0])
    bnn.manual_seed(SEED, OFF)
    clean = ev.freeze(net, "mpm", compact=True).ensemble(x, 3, max_members=2)
    bnn.manual_seed(SEED, OFF)
    clean0 = ev.freeze(net, "mpm", compact=True)(x, sample=False)

    def nan_empty(*size, **kw):
        return torch.full(*size, float("nan"), **kw)
    monkeypatch.setattr(ev, "_empty", nan_empty)
    fz = ev.freeze(net, "mpm", compact=True)
    for i in range(len(dims) - 1):
        for name in ("e0", "e_w", "var_w", "bias_var", "bias_mu"):
            assert bool(torch.isfinite(getattr(fz, "%s_%d" % (name, i))).all()), (name, i)
    bnn.manual_seed(SEED, OFF)
    out = fz.ensemble(x, 3, max_members=2)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, clean)
    bnn.manual_seed(SEED, OFF)
    out0 = fz(x, sample=False)
    assert bool(torch.isfinite(out0).all()) and torch.equal(out0, clean0)


# --------------------------------------------------------------------------- 6. the evaluation stack
@pytest.mark.parametrize("case", [cc.CASES[0], cc.CASES[1], cc.CASES[6]], ids=[cc.IDS[0], cc.IDS[1], cc.IDS[6]])
def test_the_stack_takes_a_compact_model(bnn, dev, case):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _ = _net(bnn, dev, case)
    fz = ev.freeze(net, "mpm", compact=True)
    B, S, C = 100, 10, dims[-1]
    g = torch.Generator().manual_seed(4)
    data = [(torch.rand(B, dims[0], generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)) for _ in range(3)]
    x, y = data[0]
    bnn.manual_seed(SEED, OFF)
    r = ev.ensemble_eval(fz, x, y, S)
    assert r["outputs"].shape == (S, B, C) and r["pred_ensemble"].shape == (B,) and r["pred_posterior_mean"].shape == (B,)
    assert bool((r["density"] == torch.tensor(fz.density, dtype=torch.float32)).all())
    assert r["correct_ensemble"] == int((r["outputs"].mean(0).argmax(1) == y).sum())
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(fz.ensemble(x, S), r["outputs"])
    # evaluate_batches with both accumulators against the eager updates
    acc, unc = ev.EvalAccumulator(C, S, dev), ev.UncertaintyAccumulator(C, S, dev)
    bnn.manual_seed(SEED, OFF)
    res = ev.evaluate_batches(fz, data, S, acc=acc, uncertainty=unc)
    acc_e, unc_e = ev.EvalAccumulator(C, S, dev), ev.UncertaintyAccumulator(C, S, dev)
    bnn.manual_seed(SEED, OFF)
    for xb, yb in data:
        o = fz.ensemble(xb, S)
        acc_e.update(o, yb, fz(xb, sample=False))
        unc_e.update(o, yb)
    assert torch.equal(acc._totals, acc_e._totals) and torch.equal(unc._totals, unc_e._totals)
    assert res["rows"] == 3 * B
    # the graphed step: a replay equals the eager step bitwise from the same offset
    acc_g = ev.EvalAccumulator(C, S, dev)
    step = bnn.graphs.make_graphed_eval_step(fz, x, y, S, acc_g)
    bnn.manual_seed(SEED, OFF)
    got = []
    for xb, yb in data:
        got.append({k: v.clone() for k, v in step(xb, yb).items()})
    acc_2 = ev.EvalAccumulator(C, S, dev)
    bnn.manual_seed(SEED, OFF)
    for (xb, yb), rows_g in zip(data, got):
        rows_e = acc_2.update(fz.ensemble(xb, S), yb, fz(xb, sample=False))
        assert sorted(rows_e) == sorted(rows_g)
        for k in rows_e:
            assert torch.equal(rows_e[k], rows_g[k]), k
    assert torch.equal(acc_g._totals, acc_2._totals) and acc_g.updates == 3


def test_sigmoid_head_feeds_the_accumulator(bnn, dev):
    ev = bnn.evaluate
    case = cc.CASES[7]
    family, dims, T, head = case
    net, _ = _net(bnn, dev, case)
    net, masks = _net(bnn, dev, case)
    fz = ev.freeze(net, "mpm", compact=True)
    assert fz.head == "sigmoid" and fz.full_dims == (20, 1)
    assert fz.dims == (cc.expected_live_sizes(cc.brute_need(masks))[0], 1) and fz.dims[0] < 20      # only the inputs shrink
    B, S = 100, 10
    x = _x(dev, B, 20)
    y = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(2)).to(dev)
    bnn.manual_seed(SEED, OFF)
    probs = fz.ensemble(x, S)
    bnn.manual_seed(SEED, OFF)
    logp = fz.ensemble(x, S, log_probs=True)
    assert probs.shape == (S, B, 1) and logp.shape == (S, B, 2)
    assert rel_err(logp[..., 1].exp(), probs[..., 0]) < 1e-5
    acc = ev.EvalAccumulator(2, S, dev)
    acc.update(logp, y)
    bnn.manual_seed(SEED, OFF)
    r = ev.ensemble_eval(fz, x, y.float(), S)
    assert torch.equal(r["outputs"], logp)
    assert acc.result()["rows"] == B and acc.result()["correct_ensemble"] == r["correct_ensemble"]


# --------------------------------------------------------------------------- 7. the input gather
@pytest.mark.parametrize("B", [0, 1, 257])
def test_gather_columns_equals_index_select(bnn, dev, B):
    from bnn_amd import _lib
    width, ldx = 50, 56                                                       # rows wider than the data: a strided ldx
    g = torch.Generator().manual_seed(9)
    buf = torch.rand(max(B, 1), ldx, generator=g).to(dev)
    x = buf[:B, :width]
    idx = torch.sort(torch.randperm(width, generator=g)[:29]).values.to(dev)
    for n_idx, ldo in ((29, 32), (28, 28), (1, 4)):
        ii = idx[:n_idx].to(torch.int32).contiguous()
        out = torch.full((B, ldo), float("nan"), device=dev)
        rc = _lib.lib().lbbnn_gather_columns(x.data_ptr() if B else None, ldx, ii.data_ptr(), n_idx, out.data_ptr() if B else None,
                                             ldo, B, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        assert torch.equal(out[:, :n_idx], torch.index_select(x, 1, ii.long()))
        assert bool((out[:, n_idx:] == 0).all())                              # the tail of the padded row is written too


def test_no_gather_when_no_input_is_unneeded_and_one_call_more_otherwise(bnn, dev):
    from bnn_amd import _lib
    ev = bnn.evaluate
    dims = (32, 24, 16, 3)
    for family in ("lrt", "mnf"):
        torch.manual_seed(11)
        net = (bnn.lrt.BayesianNetwork(dims) if family == "lrt" else
               bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")).to(dev).eval()
        with torch.no_grad():
            for l in net._layers():
                l.lambdal.fill_(2.0)                                          # everything kept: every input is needed
            net.l2.lambdal[:, 1::3] = -2.0                                    # ... but hidden units go
        x = _x(dev, 100, dims[0])

        def calls(model, f):
            _lib.RECORD = rec = []
            try:
                f(model)
            finally:
                _lib.RECORD = None
            return [c[0] for c in rec]
        full, fz = ev.freeze(net, "mpm"), ev.freeze(net, "mpm", compact=True)
        assert fz.dims == (32, 16, 16, 3) and fz._input_identity
        for f in (lambda m: m.ensemble(x, 10), lambda m: m(x, sample=False)):
            c_full, c_fz = calls(full, f), calls(fz, f)
            assert "lbbnn_gather_columns" not in c_fz
            assert len(c_fz) == len(c_full), (c_fz, c_full)                    # the same calls at smaller shapes
        assert fz._input(x).data_ptr() == x.data_ptr()                        # no copy either
        with torch.no_grad():
            net.l1.lambdal[:, 1::3] = -2.0                                    # now inputs go too: one gather per call
        full, fz = ev.freeze(net, "mpm"), ev.freeze(net, "mpm", compact=True)
        assert fz.dims == (24, 16, 16, 3) and not fz._input_identity
        for f in (lambda m: m.ensemble(x, 10), lambda m: m(x, sample=False)):
            c_full, c_fz = calls(full, f), calls(fz, f)
            assert c_fz.count("lbbnn_gather_columns") == 1 and len(c_fz) == len(c_full) + 1, (c_fz, c_full)
            if family == "mnf":
                assert c_fz.count("lbbnn_frozen_members_compact") == c_full.count("lbbnn_frozen_members") == 1
        bnn.manual_seed(SEED, OFF)
        ref = full(x, sample=False)
        bnn.manual_seed(SEED, OFF)
        assert rel_err(fz(x, sample=False), ref) < BAR["fp32"]


def test_a_copied_or_moved_model_addresses_its_own_buffers(bnn, dev):
    """The maps of a compact model are arrays of device addresses (the live_<b> index buffers), and the member buffers are kept
    across calls: a deep copy, or a model moved or cast, must address its own buffers.  The planar-MNF model of the test
    above in its second state: (32, 24, 16, 3) compacts to (24, 16, 16, 3), so the input is gathered too.  The original's
    index buffers are poisoned with zeros, which are in range at every boundary: a twin that read them would gather the wrong
    columns, never out of bounds."""
    import copy
    ev = bnn.evaluate
    dims = (32, 24, 16, 3)
    torch.manual_seed(11)
    net = bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).eval()
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.fill_(2.0)
        net.l2.lambdal[:, 1::3] = -2.0
        net.l1.lambdal[:, 1::3] = -2.0
    fz = ev.freeze(net, "mpm", compact=True)
    assert fz.dims == (24, 16, 16, 3) and not fz._input_identity
    B, S = 5, 3
    x = _x(dev, B, dims[0])
    bnn.manual_seed(SEED, OFF)
    want = fz.ensemble(x, S)
    assert want.shape == (S, B, 3) and bool(torch.isfinite(want).all())
    twin = copy.deepcopy(fz)
    for k, b in fz.named_buffers():
        b.fill_(float("nan")) if b.is_floating_point() else b.zero_()
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(twin.ensemble(x, S), want)
    old = dict(twin.named_buffers())
    moved = twin.double().float()                                # every float buffer replaced (a cast leaves int32 ones in place)
    for k, b in moved.named_buffers():
        if b.is_floating_point():
            assert b.data_ptr() != old[k].data_ptr(), k
            old[k].fill_(float("nan"))                           # still alive: a stale address reads NaN, not freed memory
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(moved.ensemble(x, S, keep_z=True), want)
    assert [tuple(z.shape) for z in moved.last_z] == [(S, 32), (S, 24), (S, 16)]      # z at the full widths
    with pytest.raises(RuntimeError, match="data is on"):
        moved.cpu().ensemble(x, S)
