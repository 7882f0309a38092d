"""GPU tier of the sparse median-probability model (evaluate.freeze(net, "mpm", sparse=True) / SparseFrozenNetwork;
include/lbbnn.h lbbnn_sparse_count / _pack / lbbnn_frozen_members_z / lbbnn_sparse_layer_members): the packed CSR equals the
torch builder and the dense model's fp32 operands bit for bit; members equal the fp64 oracle on the regenerated draws; the
draws are the dense median model's; the bits of an output depend on its member, row and unit alone; the empty row; the heads,
the accumulators and the graphed step; the refusals that need a device.

Bars (tests/test_parity_gpu.py): rel_err < TOL = 1e-4 the contract, elementwise_violation <= 1, and TIGHT = 5e-6 as rel_err
for fp32 outputs (the dense fp32 model meets it at 3.3e-7; sequential fp32 sums over the kept weights stay at or below 1e-6 of
max|out| at these widths and densities).  Inputs: tests/frozen_sparse_ref.py."""
import pytest
import torch

import frozen_sparse_ref as sr
from conftest import elementwise_violation, rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4
TIGHT = 5e-6
SEED, OFF = 3, 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    bnn_amd.set_precision("fp32")
    return bnn_amd


def _net(bnn, dev, case, threshold=0.5, seed=11):
    """The case's network with the reference lambdal of ``threshold``; returns (net, keep masks)."""
    family, dims, T, head = case
    torch.manual_seed(seed)
    if family == "lrt":
        net = bnn.lrt.BayesianNetwork(dims, head=head)
    else:
        net = bnn.mnf.BayesianNetwork(dims, T, z_flow_type="Planar", r_flow_type="Planar", head=head)
    net = net.to(dev).eval()
    lams, masks = sr.lambdals(dims, threshold)
    sr.apply(net, lams)
    return net, masks


def _x(dev, B, I, seed=1):
    return torch.rand(B, I, generator=torch.Generator().manual_seed(seed + B)).to(dev)


def _case(name):
    return sr.CASES[sr.IDS.index(name)]


# --------------------------------------------------------------------------- 1. the pack is exact
@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("case", sr.CASES, ids=sr.IDS)
def test_pack_is_exact(bnn, dev, monkeypatch, case, threshold):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, masks = _net(bnn, dev, case, threshold)
    dense = ev.freeze(net, "mpm", threshold=threshold)
    assert not any(dense._split)                                           # fp32 operands to compare with

    def nan_empty(*size, **kw):
        return torch.full(*size, float("nan"), **kw)
    monkeypatch.setattr(ev, "_empty", nan_empty)                           # a slot that was never packed stays NaN
    fz = ev.freeze(net, "mpm", threshold=threshold, sparse=True)
    assert isinstance(fz, ev.SparseFrozenNetwork) and ev._is_frozen(fz) and list(fz.parameters()) == []
    assert fz.dims == fz.full_dims == tuple(dims) and fz.head == head and fz.family == family and fz.gates == "mpm"
    for i in range(len(dims) - 1):
        for name in ("e0", "e_w", "var_w"):
            assert not hasattr(fz, "%s_%d" % (name, i))                    # no dense operand
    total, nbytes = 0, 0
    cut = sr.cut_of(threshold)
    for i, (l, keep) in enumerate(zip(net._layers(), masks)):
        O, I = l.out_features, l.in_features
        row_ptr, col, k = sr.csr_of(l.lambdal.detach().cpu(), cut)
        assert torch.equal(k, keep)
        got = [t.cpu() for t in fz.csr(i)]
        assert got[0].dtype == got[1].dtype == torch.int32 and got[2].dtype == got[3].dtype == torch.float32
        assert torch.equal(got[0], row_ptr) and torch.equal(got[1], col)
        assert torch.equal(got[2].view(torch.int32), l.weight_mu.detach().cpu()[keep].view(torch.int32))      # the bits of weight_mu
        var_w = dense._buf("var_w", i).cpu()[:, :I]
        assert torch.equal(sr.decode(got[0], got[1], got[3], O, I).view(torch.int32), var_w.view(torch.int32))
        assert bool((got[3] > 0).all())                                    # (decode's zeros are var_w's zeros: nothing kept there)
        assert torch.equal(fz._buf("bias_var", i).view(torch.int32), dense._buf("bias_var", i).view(torch.int32))
        assert torch.equal(fz._buf("bias_mu", i), l.bias_mu.detach())
        assert fz.kept_rows[i].dtype == torch.int32 and torch.equal(fz.kept_rows[i].cpu().long(), keep.sum(1))
        assert torch.equal(fz.kept_rows[i], dense.kept_rows[i])
        total += int(keep.sum())
        nbytes += 4 * (O + 1) + 12 * int(keep.sum()) + 8 * O
    assert type(fz.nnz) is int and fz.nnz == total and fz.kept == [int(k.sum()) for k in masks]
    assert type(fz.operand_bytes) is int and fz.operand_bytes == nbytes
    assert isinstance(fz.density, float) and fz.density == total / sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
    assert fz.density == dense.density
    # ... and the evaluation reads nothing that was not written: NaN-filled buffers give the bits of clean ones
    monkeypatch.undo()
    clean = ev.freeze(net, "mpm", threshold=threshold, sparse=True)
    x = _x(dev, 65, dims[0])
    bnn.manual_seed(SEED, OFF)
    want = clean.ensemble(x, 3, max_members=2)
    bnn.manual_seed(SEED, OFF)
    want0 = clean(x, sample=False)
    monkeypatch.setattr(ev, "_empty", nan_empty)
    bnn.manual_seed(SEED, OFF)
    out = fz.ensemble(x, 3, max_members=2)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, want)
    bnn.manual_seed(SEED, OFF)
    out0 = fz(x, sample=False)
    assert bool(torch.isfinite(out0).all()) and torch.equal(out0, want0)


# --------------------------------------------------------------------------- 2. members against fp64
def _oracle_member(bnn, fz, net, masks, x, m, stochastic, z_used):
    """Member m in float64 by the recipe of tests/test_frozen_gpu.py: lambdal = +-1000 (fp64 alpha exactly 1 / 0), the z the
    member used, eps regenerated at the documented stream / offset / row offset through lbbnn_philox_normal."""
    ops, dev = bnn.ops, x.device
    rng_m = torch.tensor([SEED, OFF + m], dtype=torch.int64, device=dev)
    layers = net._layers()
    h = x.double().cpu()
    ident = orc.Flow("Planar", [])
    for i, (l, keep) in enumerate(zip(layers, masks)):
        p = {k: getattr(l, k).detach().double().cpu() for k in ("weight_mu", "weight_rho", "bias_mu", "bias_rho")}
        p["lambdal"] = torch.where(keep, 1000.0, -1000.0).double()
        a = orc.alpha_of(p["lambdal"])
        assert bool(((a == 0) | (a == 1)).all())
        eps = ops.philox_normal(rng_m, ops.STREAM_EPS_OUT * 64 + l._layer_id, x.shape[0], l.out_features,
                                row_base=l.row_offset).double().cpu() if stochastic else None
        if fz.family == "mnf":
            p["q0_mean"] = z_used[i][m].double().cpu()                       # z0 = q0_mean + 0 * eps_z, no transforms: z itself
            p["q0_log_var"] = torch.full_like(p["q0_mean"], -float("inf"))
            noise = {"eps_z": torch.zeros(1, l.in_features, dtype=torch.float64), "eps_out": eps}
            h, _, _ = orc.mnf_forward(h, p, ident, None, noise, stochastic=stochastic, compute_kl=False)
        else:
            h, _, _ = orc.lrt_forward(h, p, eps, stochastic=stochastic, compute_kl=False)
        if i < len(layers) - 1:
            h = torch.relu(h)
    if fz.head == "sigmoid":
        return torch.sigmoid(h)
    return h if fz.head == "identity" else torch.log_softmax(h, dim=1)


@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("case", sr.CASES, ids=sr.IDS)
def test_members_against_fp64_oracle(bnn, dev, case, threshold):
    """Measured on an MI355X, worst over the (B, S) of a case: member rel_err 8.3e-8 (8-32-2) .. 6.7e-7 (784-400-600-10, LRT,
    threshold 0.5), elementwise form at most 0.031; posterior mean rel_err at most 4.7e-7.  Each case prints its own."""
    ev = bnn.evaluate
    family, dims, T, head = case
    net, masks = _net(bnn, dev, case, threshold)
    fz = ev.freeze(net, "mpm", threshold=threshold, sparse=True)
    worst = (0.0, 0.0)
    for B, S in sr.batch_sizes(dims):
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        out = fz.ensemble(x, S, keep_z=True)
        z = fz.last_z
        assert out.shape == (S, B, dims[-1])
        if family == "mnf":
            assert [tuple(t.shape) for t in z] == [(S, I) for I in dims[:-1]]
        else:
            assert z == [None] * (len(dims) - 1)
        for m in range(S):
            ref = _oracle_member(bnn, fz, net, masks, x, m, True, z)
            e, v = rel_err(out[m], ref), elementwise_violation(out[m], ref)
            worst = (max(worst[0], e), max(worst[1], v))
            assert e < TOL and v <= 1.0 and e < TIGHT, (B, m, e, v)
        if S > 1:
            assert not torch.equal(out[0], out[1])
    # sample=False against the oracle's stochastic=False branch (an MNF model still draws z: recover it as member 0's)
    B = sr.batch_sizes(dims)[0][0]
    x = _x(dev, B, dims[0])
    bnn.manual_seed(SEED, OFF)
    fz.ensemble(x, 1, keep_z=True)
    z = fz.last_z
    bnn.manual_seed(SEED, OFF)
    out0 = fz(x, sample=False)
    st = bnn.ops.RngState.get(dev)
    assert int(st.t[1]) == OFF + (1 if family == "mnf" else 0)
    ref0 = _oracle_member(bnn, fz, net, masks, x, 0, False, z)
    e0, v0 = rel_err(out0, ref0), elementwise_violation(out0, ref0)
    print("sparse-vs-fp64 %s %s threshold %g: members rel_err %.3g elementwise %.3g; mean forward rel_err %.3g elementwise %.3g"
          % (family, dims, threshold, worst[0], worst[1], e0, v0))
    assert out0.shape == (B, dims[-1]) and e0 < TOL and v0 <= 1.0 and e0 < TIGHT, (e0, v0)


# --------------------------------------------------------------------------- 3. the draws of the dense median model
@pytest.mark.parametrize("case", sr.CASES, ids=sr.IDS)
def test_same_draws_as_the_dense_median_model(bnn, dev, case):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _ = _net(bnn, dev, case)
    dense, fz = ev.freeze(net, "mpm"), ev.freeze(net, "mpm", sparse=True)
    st = bnn.ops.RngState.get(dev)
    for B, S in sr.batch_sizes(dims):
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        ref = dense.ensemble(x, S, keep_z=True)
        z_ref, off_ref = dense.last_z, int(st.t[1])
        bnn.manual_seed(SEED, OFF)
        out = fz.ensemble(x, S, keep_z=True)
        assert int(st.t[1]) == off_ref == OFF + S
        for a, b in zip(fz.last_z, z_ref):
            assert (a is None and b is None) or torch.equal(a, b)
        e = rel_err(out, ref)
        print("sparse-vs-dense %s %s B=%d S=%d rel_err %.3g" % (family, dims, B, S, e))
        assert out.shape == ref.shape and e < TIGHT, (B, S, e)
        bnn.manual_seed(SEED, OFF)
        ref0 = dense(x, sample=False)
        off0 = int(st.t[1])
        bnn.manual_seed(SEED, OFF)
        out0 = fz(x, sample=False)
        assert int(st.t[1]) == off0 and rel_err(out0, ref0) < TIGHT


# --------------------------------------------------------------------------- 4. bits depend on (member, row, unit) alone
@pytest.mark.parametrize("case", [c for c in sr.CASES if c[1] != sr.BIG], ids=[i for c, i in zip(sr.CASES, sr.IDS) if c[1] != sr.BIG])
def test_bits_depend_on_member_row_and_unit_alone(bnn, dev, case):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _ = _net(bnn, dev, case, 0.9)
    fz = ev.freeze(net, "mpm", threshold=0.9, sparse=True)
    st = bnn.ops.RngState.get(dev)
    x = _x(dev, 257, dims[0])
    bnn.manual_seed(SEED, OFF)
    whole = fz.ensemble(x, 10, keep_z=True)
    z_whole = fz.last_z
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(fz.ensemble(x, 10), whole)                          # two runs, the same bits
    bnn.manual_seed(SEED, OFF)
    part = fz.ensemble(x, 10, max_members=3, keep_z=True)
    assert int(st.t[1]) == OFF + 10 and torch.equal(part, whole)
    for a, b in zip(fz.last_z, z_whole):
        assert (a is None and b is None) or torch.equal(a, b)
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(ev.ensemble_forward(fz, x, 10, max_members=4), whole)
    for m in (0, 3, 9):
        bnn.manual_seed(SEED, OFF + m)
        assert torch.equal(fz.ensemble(x, 1)[0], whole[m]), m
        bnn.manual_seed(SEED, OFF + m)
        assert torch.equal(fz(x, sample=True), whole[m]), m
        assert int(st.t[1]) == OFF + m + 1
    # the first 64 rows as a batch of their own (one row per lane there, two per lane in the batch of 257)
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(fz.ensemble(x[:64], 10), whole[:, :64])
    # rows 192 .. 256 of the batch as a batch of their own: the layers' row_offset says where they lie
    net.set_row_offset(192)
    try:
        piece = ev.freeze(net, "mpm", threshold=0.9, sparse=True)
    finally:
        net.set_row_offset(0)
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(piece.ensemble(x[192:], 10, max_members=4), whole[:, 192:])


# --------------------------------------------------------------------------- 5. the empty row
@pytest.mark.parametrize("case", [_case("lrt-64-48-40-20"), _case("mnf-8-32-2-T2"), _case("lrt-2048-64-32-10")],
                         ids=["lrt-64-48-40-20", "mnf-8-32-2-T2", "lrt-2048-64-32-10"])
def test_empty_row(bnn, dev, case):
    """Unit 0 of the first layer keeps no weight: relu(bias_mu + sqrt(bias_var) * eps) from the regenerated eps, and
    relu(bias_mu) exactly without noise -- read from ONE lbbnn_sparse_layer_members call on the model's first layer."""
    from bnn_amd import _lib
    ev, ops = bnn.evaluate, bnn.ops
    family, dims, T, head = case
    net, masks = _net(bnn, dev, case)
    l = net._layers()[0]
    with torch.no_grad():
        l.bias_mu[0], l.bias_rho[0] = 0.05, -1.0                           # sigma = 0.31: the unit's ReLU sees both signs
    fz = ev.freeze(net, "mpm", sparse=True)
    O, I, B, S = dims[1], dims[0], 65, 3
    assert not bool(masks[0][0].any()) and int(fz.kept_rows[0][0]) == 0
    x = _x(dev, B, I)
    xt = ops.transpose_operand(x)                                          # [I][operand_ld(B)]
    row_ptr, col, mean, var = fz.csr(0)
    rng = torch.tensor([SEED, OFF], dtype=torch.int64, device=dev)
    bias_mu, bias_var = fz._buf("bias_mu", 0), fz._buf("bias_var", 0)
    stream_id = ops.STREAM_EPS_OUT * 64 + l._layer_id
    for flags in (ops.F_RELU, ops.F_RELU | ops.F_MEAN_ONLY):
        out = torch.full((S, B * O), float("nan"), device=dev)
        rc = _lib.lib().lbbnn_sparse_layer_members(
            row_ptr.data_ptr(), col.data_ptr(), mean.data_ptr(), var.data_ptr(), col.numel(), bias_mu.data_ptr(), bias_var.data_ptr(),
            xt.data_ptr(), xt.stride(0), 0, None, 0, rng.data_ptr(), stream_id, 7, 1, out.data_ptr(), O, B * O, 1, B, I, O, flags, S,
            torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        out = out.view(S, B, O)
        assert bool(torch.isfinite(out).all())
        if flags & ops.F_MEAN_ONLY:
            assert torch.equal(out[:, :, 0], torch.relu(bias_mu[0]).expand(S, B))
            continue
        for m in range(S):
            rng_m = torch.tensor([SEED, OFF + m], dtype=torch.int64, device=dev)
            eps = ops.philox_normal(rng_m, stream_id, B, O, row_base=7).double()
            ref = torch.relu(bias_mu[0].double() + bias_var[0].double().sqrt() * eps[:, 0])
            assert bool((ref > 0).any()) and bool((ref == 0).any()) and rel_err(out[m, :, 0], ref) < TIGHT


# --------------------------------------------------------------------------- 6. heads and consumers
def test_sigmoid_head_and_the_accumulator(bnn, dev):
    ev = bnn.evaluate
    case = _case("lrt-20-1")
    net, _ = _net(bnn, dev, case)
    fz = ev.freeze(net, "mpm", sparse=True)
    assert fz.head == "sigmoid" and fz.dims == (20, 1)
    B, S = 100, 10
    x = _x(dev, B, 20)
    y = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(2)).to(dev)
    bnn.manual_seed(SEED, OFF)
    probs = fz.ensemble(x, S)
    bnn.manual_seed(SEED, OFF)
    logp = fz.ensemble(x, S, log_probs=True)
    assert probs.shape == (S, B, 1) and logp.shape == (S, B, 2)
    assert bool(((probs > 0) & (probs < 1)).all()) and rel_err(logp[..., 1].exp(), probs[..., 0]) < 1e-5
    assert fz(x, sample=False).shape == (B, 1) and fz(x, sample=False, log_probs=True).shape == (B, 2)
    acc = ev.EvalAccumulator(2, S, dev)
    acc.update(logp, y)
    bnn.manual_seed(SEED, OFF)
    r = ev.ensemble_eval(fz, x, y.float(), S)
    assert torch.equal(r["outputs"], logp)
    assert acc.result()["rows"] == B and acc.result()["correct_ensemble"] == r["correct_ensemble"]


@pytest.mark.parametrize("case", [_case("lrt-64-48-40-20"), _case("mnf-64-48-40-20-T2")], ids=["lrt", "mnf"])
def test_the_stack_and_the_graphed_step_take_a_sparse_model(bnn, dev, case):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _ = _net(bnn, dev, case)
    fz = ev.freeze(net, "mpm", sparse=True)
    B, S, C = 100, 10, dims[-1]
    g = torch.Generator().manual_seed(4)
    data = [(torch.rand(B, dims[0], generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)) for _ in range(3)]
    x, y = data[0]
    bnn.manual_seed(SEED, OFF)
    r = ev.ensemble_eval(fz, x, y, S)
    assert r["outputs"].shape == (S, B, C) and bool((r["density"] == torch.tensor(fz.density, dtype=torch.float32)).all())
    assert r["correct_ensemble"] == int((r["outputs"].mean(0).argmax(1) == y).sum())
    assert rel_err(r["outputs"].exp().sum(-1), torch.ones(S, B)) < 1e-5      # log-probabilities (O = 20: torch's log_softmax)
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(fz.ensemble(x, S), r["outputs"])
    h = ev.predictive_entropy(r["outputs"])
    assert h.shape == (B,) and bool(torch.isfinite(h).all())
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


def test_identity_head_feeds_the_regression_accumulator(bnn, dev):
    ev = bnn.evaluate
    case = _case("mnf-8-32-2-T2")
    net, _ = _net(bnn, dev, case)
    fz = ev.freeze(net, "mpm", sparse=True)
    assert fz.head == "identity"
    B, S, O = 100, 10, 2
    g = torch.Generator().manual_seed(4)
    data = [(torch.rand(B, 8, generator=g).to(dev), torch.randn(B, O, generator=g).to(dev)) for _ in range(2)]
    acc = ev.RegressionAccumulator(O, S, dev, 0.0)
    bnn.manual_seed(SEED, OFF)
    res = ev.evaluate_batches(fz, data, S, acc=acc)
    acc_e = ev.RegressionAccumulator(O, S, dev, 0.0)
    bnn.manual_seed(SEED, OFF)
    for xb, yb in data:
        o = fz.ensemble(xb, S)
        assert o.shape == (S, B, O)
        acc_e.update(o, yb, fz(xb, sample=False))
    assert torch.equal(acc._totals, acc_e._totals)
    assert res["elements"] == 2 * B * O
    # predict_regression: the predictive mean is the mean of the model's own members from the same offset
    bnn.manual_seed(SEED, OFF)
    pred = ev.predict_regression(fz, data[0][0], S, 0.0)
    bnn.manual_seed(SEED, OFF)
    members = fz.ensemble(data[0][0], S)
    assert pred["pred_mean"].shape == (B, O) and rel_err(pred["pred_mean"], members.double().mean(0)) < 1e-5


# --------------------------------------------------------------------------- 7. refusals that need a device
def test_refusals_on_the_device(bnn, dev):
    ev = bnn.evaluate
    net, _ = _net(bnn, dev, _case("mnf-20-16-12-3-T4"))
    fz = ev.freeze(net, "mpm", sparse=True)
    x = _x(dev, 5, 20)
    with pytest.raises(ValueError, match=r"explain is not built for sparse=True models.*evaluate.freeze\(net, \"mpm\"\)"):
        ev.explain(fz, x)
    with pytest.raises(NotImplementedError, match=r"a sparse model does not refresh.*sparse=True"):
        fz.refresh()
    with pytest.raises(RuntimeError, match="evaluates on a HIP device tensor"):
        fz.ensemble(x.cpu(), 2)
    with pytest.raises(RuntimeError, match="evaluates on a HIP device tensor"):
        fz(x.cpu())
    with pytest.raises(ValueError, match="log_probs=True applies"):
        fz.ensemble(x, 2, log_probs=True)
    with pytest.raises(ValueError):
        ev.ensemble_forward(fz, x, 2, gates="mpm")
    assert "sparse" in repr(fz)


def test_a_copied_or_moved_model_addresses_its_own_buffers(bnn, dev):
    import copy
    ev = bnn.evaluate
    net, _ = _net(bnn, dev, _case("mnf-20-16-12-3-T4"))
    fz = ev.freeze(net, "mpm", sparse=True)
    x = _x(dev, 5, 20)
    bnn.manual_seed(SEED, OFF)
    want = fz.ensemble(x, 3)
    twin = copy.deepcopy(fz)
    for k, b in fz.named_buffers():
        b.fill_(float("nan")) if b.is_floating_point() else b.zero_()      # (zeros are in range for row_ptr and col)
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(twin.ensemble(x, 3), want)
    moved = twin.double().float()
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(moved.ensemble(x, 3), want) and moved.nnz == fz.nnz
