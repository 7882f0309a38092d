"""GPU tier of the threshold sweep (evaluate.threshold_sweep / ThresholdSweep / sweep_batches; include/lbbnn.h
lbbnn_sparse_count_levels / _pack_levels / lbbnn_sparse_layer_levels).

 1. pack: every level's CSR, bias_mu and bias_var are those of freeze(net, "mpm", threshold=t_j, sparse=True) bit for bit; kept
    and density equal torch's count of lambdal > cut_j; NaN-filled buffers hold no NaN afterwards (the segments tile them);
 2. members against the separately frozen models from the same seed, bit for bit, and where the live offset stands afterwards
    (K = 1, the set "one", is the plain sparse model bit for bit);
 3. members against float64: every level's CSR rebuilt on the CPU from lambdal > cut_j, frozen_sparse_ref.member_from_csr on
    eps and z regenerated from tests/philox_ref.py (z through the oracle's planar flow in float64) -- nothing of this check runs
    a kernel of the library; the empty last level of the set "four" is part of it;
 4. a level's bits do not depend on the other levels of its sweep;
 5. sweep_batches equals evaluate_batches of every level's own model; 6. the chosen level feeds explain_ensemble;
 7. moved, copied and reloaded sweeps; 8. the refusals that need a device.

Bars (tests/test_frozen_sparse_gpu.py, from tests/test_parity_gpu.py): rel_err < TIGHT = 5e-6 for fp32 outputs and
elementwise_violation <= 1.  Inputs: tests/threshold_sweep_ref.py."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

import frozen_sparse_ref as sr
import philox_ref
import threshold_sweep_ref as tr
from conftest import elementwise_violation, rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TIGHT = 5e-6
SEED, OFF = 3, 5
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    bnn_amd.set_precision("fp32")
    return bnn_amd


def _net(bnn, dev, case, name, seed=11):
    """The case's network with the reference lambdal of the threshold set ``name``; returns (net, masks[level][layer])."""
    family, dims, T, head = case
    thresholds, span, empty_last = tr.SETS[name]
    torch.manual_seed(seed)
    if family == "lrt":
        net = bnn.lrt.BayesianNetwork(dims, head=head)
    else:
        net = bnn.mnf.BayesianNetwork(dims, T, z_flow_type="Planar", r_flow_type="Planar", head=head)
    net = net.to(dev).eval()
    lams, masks = tr.lambdals(dims, thresholds, span=span, empty_last=empty_last)
    sr.apply(net, lams)
    return net, masks


def _setup(bnn, dev, case, name):
    """(net, masks, sweep, the K models frozen one by one) of a case and a threshold set, built once for the module."""
    key = (tr.CASES.index(case), name)
    if key not in _CACHE:
        net, masks = _net(bnn, dev, case, name)
        thresholds = tr.SETS[name][0]
        sw = bnn.evaluate.threshold_sweep(net, thresholds)
        fzs = [bnn.evaluate.freeze(net, "mpm", threshold=t, sparse=True) for t in thresholds]
        _CACHE[key] = (net, masks, sw, fzs)
    return _CACHE[key]


def _x(dev, B, I, seed=1):
    return torch.rand(B, I, generator=torch.Generator().manual_seed(seed + B)).to(dev)


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_GRID = [(c, n) for c in tr.CASES for n in tr.SETS]
_GRID_IDS = ["%s-%s" % (i, n) for i in tr.IDS for n in tr.SETS]


# --------------------------------------------------------------------------- 1. the pack is exact
@pytest.mark.parametrize("case,name", _GRID, ids=_GRID_IDS)
def test_pack_is_every_levels_own_model(bnn, dev, monkeypatch, case, name):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, masks, _, fzs = _setup(bnn, dev, case, name)
    thresholds = tr.SETS[name][0]
    K, n = len(thresholds), len(dims) - 1

    def nan_empty(*size, **kw):
        return torch.full(*size, float("nan"), **kw)
    monkeypatch.setattr(ev, "_empty", nan_empty)                           # a slot that was never packed stays NaN
    sw = ev.threshold_sweep(net, thresholds)
    monkeypatch.undo()
    assert isinstance(sw, ev.ThresholdSweep) and list(sw.parameters()) == [] and not ev._is_frozen(sw)
    assert sw.thresholds == tuple(thresholds) and sw.cuts == tuple(ev._cut(t) for t in thresholds)
    assert sw.dims == tuple(dims) and sw.head == head and sw.family == family
    want_kept = torch.tensor([[int(k.sum()) for k in masks[j]] for j in range(K)])
    assert sw.kept.dtype == torch.int64 and sw.kept.is_cuda and torch.equal(sw.kept.cpu(), want_kept)
    weights = sum(dims[i] * dims[i + 1] for i in range(n))
    assert sw.density.dtype == torch.float64 and sw.density.is_cuda
    assert torch.equal(sw.density.cpu(), want_kept.sum(1).double() / weights)
    assert all(type(v) is int for v in sw.nnz) and sw.nnz == want_kept.sum(1).tolist()
    assert (sw.nnz[-1] == 0) == tr.SETS[name][2]
    nbytes = 0
    lvls = [sw.model(j) for j in range(K)]
    for i, l in enumerate(net._layers()):
        O, I = l.out_features, l.in_features
        lam = l.lambdal.detach().cpu()
        cap = int(want_kept[:, i].sum())
        nbytes += 4 * (K * O + 1) + 12 * cap + 8 * O
        kept_rows, row_ptr = sw._buf("kept_rows", i), sw._buf("row_ptr", i)
        assert kept_rows.shape == (K, O) and kept_rows.dtype == torch.int32
        assert row_ptr.shape == (K * O + 1,) and row_ptr.dtype == torch.int32
        assert torch.equal(row_ptr.cpu(), sr.exclusive_scan(kept_rows.cpu().view(-1)))
        col, mean, var = (sw._buf(k, i) for k in ("col", "mean", "var"))
        assert col.shape == mean.shape == var.shape == (cap,)               # the K segments tile the buffers: no slot is spare
        assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all()) and bool((var > 0).all())
        assert bool(((col >= 0) & (col < I)).all())
        assert bool(torch.isfinite(sw._buf("bias_var", i)).all()) and bool(torch.isfinite(sw._buf("bias_mu", i)).all())
        for j, t in enumerate(thresholds):
            keep = lam > torch.tensor(sw.cuts[j], dtype=torch.float32)
            assert torch.equal(keep, masks[j][i])
            assert torch.equal(kept_rows[j].cpu().long(), keep.sum(1))
            lvl, one = lvls[j], fzs[j]
            for got, want in zip(lvl.csr(i), one.csr(i)):
                assert _bits(got, want), (i, j)
            assert torch.equal(lvl.csr(i)[1].cpu(), sr.csr_of(lam, sw.cuts[j])[1])             # columns ascend within a row
            assert _bits(lvl._buf("bias_mu", i), one._buf("bias_mu", i)) and _bits(lvl._buf("bias_var", i), one._buf("bias_var", i))
            assert torch.equal(lvl.kept_rows[i], one.kept_rows[i])
            # the level's arrays ARE the sweep's: views of its segment
            base = int(want_kept[:j, i].sum())
            assert lvl.csr(i)[2].numel() == int(want_kept[j, i])
            if int(want_kept[j, i]):
                assert lvl.csr(i)[2].data_ptr() == mean.data_ptr() + 4 * base and lvl.csr(i)[3].data_ptr() == var.data_ptr() + 4 * base
    assert type(sw.operand_bytes) is int and sw.operand_bytes == nbytes
    for j, lvl in enumerate(lvls):
        assert isinstance(lvl, ev.SparseFrozenNetwork) and lvl.threshold == thresholds[j] and lvl.cut == sw.cuts[j]
        assert lvl.nnz == sw.nnz[j] == fzs[j].nnz and lvl.density == fzs[j].density == float(sw.density[j])
    assert "thresholds=" in repr(sw)


# --------------------------------------------------------------------------- 2. members against the separate models
@pytest.mark.parametrize("case,name", _GRID, ids=_GRID_IDS)
def test_members_are_the_separate_models_bit_for_bit(bnn, dev, case, name):
    family, dims, T, head = case
    net, masks, sw, fzs = _setup(bnn, dev, case, name)
    K = len(fzs)
    st = bnn.ops.RngState.get(dev)
    forms = [False, True] if head == "sigmoid" else [False]
    for B, S in tr.batch_sizes(name):
        x = _x(dev, B, dims[0])
        for lp in forms:
            bnn.manual_seed(SEED, OFF)
            out = sw.ensemble(x, S, log_probs=lp)
            assert int(st.t[1]) == OFF + S                                  # as ONE model's ensemble advances it
            assert out.shape == (K, S, B, 2 if lp else dims[-1]) and bool(torch.isfinite(out).all())
            bnn.manual_seed(SEED, OFF)
            mean = sw(x, log_probs=lp)
            assert int(st.t[1]) == OFF + (1 if family == "mnf" else 0)
            assert mean.shape == (K, B, 2 if lp else dims[-1])
            for j, fz in enumerate(fzs):
                bnn.manual_seed(SEED, OFF)
                assert torch.equal(fz.ensemble(x, S, log_probs=lp), out[j]), (B, S, j)
                bnn.manual_seed(SEED, OFF)
                assert torch.equal(fz(x, sample=False, log_probs=lp), mean[j]), (B, j)
            if S > 1:
                assert not torch.equal(out[0, 0], out[0, 1])
        if K > 1:
            assert not torch.equal(out[0], out[1])
    # an empty batch: the shapes, and the offset moves as with rows
    bnn.manual_seed(SEED, OFF)
    assert sw.ensemble(x[:0], 3).shape == (K, 3, 0, dims[-1]) and int(st.t[1]) == OFF + 3
    bnn.manual_seed(SEED, OFF)
    assert sw(x[:0]).shape == (K, 0, dims[-1]) and int(st.t[1]) == OFF + (1 if family == "mnf" else 0)


# --------------------------------------------------------------------------- 3. members against fp64
def _draws64(bnn, net, B, s, stochastic):
    """Draw s in float64 from tests/philox_ref.py: per layer (z or None, eps or None).  z = the planar flow of q0_mean +
    exp(q0_log_var / 2) * eps_z (stream STREAM_EPS_Z * 64 + layer id, a vector draw) in the oracle's arithmetic; eps = the
    (B, O) matrix draw of stream STREAM_EPS_OUT * 64 + layer id at the layer's row offset; both at Philox offset OFF + s."""
    ops, out = bnn.ops, []
    for l in net._layers():
        z = None
        if l._mnf:
            I, Tn = l.in_features, len(l.z_flow.transforms)
            sd = {k: v.detach().double().cpu() for k, v in l.state_dict().items()}
            eps_z = torch.from_numpy(philox_ref.normal_vector(SEED, OFF + s, ops.STREAM_EPS_Z * 64 + l._layer_id, I))
            z, _, _ = orc.mnf_sample_z(sd, eps_z.reshape(1, I), orc.flow_from_state("z_flow", "Planar", sd, Tn))
        eps = torch.from_numpy(philox_ref.normal_matrix(SEED, OFF + s, ops.STREAM_EPS_OUT * 64 + l._layer_id, B, l.out_features,
                                                        row_base=l.row_offset)) if stochastic else None
        out.append((z, eps))
    return out


def _member64(net, masks_j, cut, x, draws, head, stochastic):
    layers = []
    for l, keep, (z, eps) in zip(net._layers(), masks_j, draws):
        lam = l.lambdal.detach().cpu()
        row_ptr, col, k = sr.csr_of(lam, cut)
        assert torch.equal(k, keep)
        p = {n: getattr(l, n).detach().double().cpu() for n in ("weight_mu", "weight_rho", "bias_mu", "bias_rho")}
        layers.append({"row_ptr": row_ptr, "col": col, "mean": p["weight_mu"][keep], "var": orc.sigma_of(p["weight_rho"])[keep] ** 2,
                       "bias_mu": p["bias_mu"], "bias_var": orc.sigma_of(p["bias_rho"]) ** 2, "z": z, "eps": eps})
    return sr.member_from_csr(x.double().cpu(), layers, head=head, stochastic=stochastic)


@pytest.mark.parametrize("case,name", _GRID, ids=_GRID_IDS)
def test_members_against_fp64(bnn, dev, case, name):
    """Each case prints its worst figures; measured on an MI355X over all cases, sets and levels: rel_err at most 2.5e-7,
    elementwise form at most 0.003.  The last level of the set "four" keeps no weight in any layer: its members are the
    chains head(bias_mu + sqrt(bias_var) * eps) through the ReLUs, held to the same bars."""
    family, dims, T, head = case
    net, masks, sw, _ = _setup(bnn, dev, case, name)
    K = len(sw.cuts)
    worst, worst0 = (0.0, 0.0), (0.0, 0.0)
    for B, S in tr.batch_sizes(name):
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        out = sw.ensemble(x, S)
        assert bool(torch.isfinite(out).all())
        for s in range(S):
            draws = _draws64(bnn, net, B, s, True)
            for j in range(K):
                ref = _member64(net, masks[j], sw.cuts[j], x, draws, head, True)
                e, v = rel_err(out[j, s], ref), elementwise_violation(out[j, s], ref)
                worst = (max(worst[0], e), max(worst[1], v))
                assert e < TIGHT and v <= 1.0, (B, S, j, s, e, v)
        bnn.manual_seed(SEED, OFF)
        mean = sw(x)
        draws = _draws64(bnn, net, B, 0, False)
        for j in range(K):
            ref = _member64(net, masks[j], sw.cuts[j], x, draws, head, False)
            e, v = rel_err(mean[j], ref), elementwise_violation(mean[j], ref)
            worst0 = (max(worst0[0], e), max(worst0[1], v))
            assert e < TIGHT and v <= 1.0, (B, j, e, v)
    if tr.SETS[name][2]:
        assert sw.nnz[-1] == 0 and all(int(k[-1].sum()) == 0 for k in (sw._buf("kept_rows", i) for i in range(len(dims) - 1)))
        assert bool(torch.isfinite(out[-1]).all()) and bool(torch.isfinite(mean[-1]).all())
        if S > 1:
            assert not torch.equal(out[-1, 0], out[-1, 1])                 # the bias draws differ between the members
    print("sweep-vs-fp64 %s %s %s: members rel_err %.3g elementwise %.3g; mean forward rel_err %.3g elementwise %.3g"
          % (family, dims, name, worst[0], worst[1], worst0[0], worst0[1]))


# --------------------------------------------------------------------------- 4. a level does not see the other levels
@pytest.mark.parametrize("case", tr.CASES[:3], ids=tr.IDS[:3])
def test_a_levels_bits_do_not_depend_on_the_other_levels(bnn, dev, case):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _, _, _ = _setup(bnn, dev, case, "four")
    a, b = ev.threshold_sweep(net, (0.5, 0.9)), ev.threshold_sweep(net, (0.3, 0.9, 0.99))
    for B, S in ((65, 2), (130, 3)):
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        oa = a.ensemble(x, S)
        bnn.manual_seed(SEED, OFF)
        ob = b.ensemble(x, S)
        assert torch.equal(oa[1], ob[1]) and not torch.equal(oa[0], ob[0])
        bnn.manual_seed(SEED, OFF)
        ma = a(x)
        bnn.manual_seed(SEED, OFF)
        mb = b(x)
        assert torch.equal(ma[1], mb[1])


# --------------------------------------------------------------------------- 5. the evaluation pass
def _same(a, b):
    """Integers exactly, doubles bit for bit, through dicts, lists, arrays and the bound ``coverage`` function of a regression
    result (a functools.partial over the PIT histogram: the same function on the same arguments)."""
    if isinstance(a, functools.partial):
        return isinstance(b, functools.partial) and a.func is b.func and _same(a.args, b.args) and _same(a.keywords, b.keywords)
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if isinstance(a, float):
        return type(b) is float and (a == b or (math.isnan(a) and math.isnan(b)))
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("case", [tr.CASES[i] for i in (0, 1, 3, 4)], ids=[tr.IDS[i] for i in (0, 1, 3, 4)])
def test_sweep_batches_is_evaluate_batches_of_every_level(bnn, dev, case):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, masks, sw, fzs = _setup(bnn, dev, case, "four")
    K, B, S, C = len(fzs), 65, 3, dims[-1]
    g = torch.Generator().manual_seed(4)
    if head == "identity":
        ys = [torch.randn(B, C, generator=g) for _ in range(3)]
    elif head == "sigmoid":
        ys = [torch.randint(0, 2, (B,), generator=g).float() for _ in range(3)]            # float 0 / 1 targets
    else:
        ys = [torch.randint(0, C, (B,), generator=g) for _ in range(3)]
    data = [(torch.rand(B, dims[0], generator=g).to(dev), y.to(dev)) for y in ys]
    st = bnn.ops.RngState.get(dev)
    make = (lambda: ev.RegressionAccumulator(C, S, dev, 0.0)) if head == "identity" else None
    bnn.manual_seed(SEED, OFF)
    res = ev.sweep_batches(sw, data, S, accs=[make() for _ in range(K)] if make else None)
    end = int(st.t[1])
    assert end == OFF + 3 * (S + (1 if family == "mnf" else 0))
    assert sorted(res) == ["density", "kept", "results", "thresholds"] and len(res["results"]) == K
    assert res["thresholds"] == sw.thresholds and torch.equal(res["kept"], sw.kept) and torch.equal(res["density"], sw.density)
    for j, fz in enumerate(fzs):
        bnn.manual_seed(SEED, OFF)
        want = ev.evaluate_batches(fz, data, S, acc=make() if make else None)
        assert int(st.t[1]) == end
        assert _same(res["results"][j], want), (j, res["results"][j], want)
    if head != "identity":
        assert all(r["rows"] == 3 * B for r in res["results"])
    # without the posterior-mean forward, into accumulators of the caller
    accs = [make() if make else ev.EvalAccumulator(2 if head == "sigmoid" else C, S, dev) for _ in range(K)]
    bnn.manual_seed(SEED, OFF)
    res2 = ev.sweep_batches(sw, data[:1], S, posterior_mean=False, accs=accs)
    assert int(st.t[1]) == OFF + S
    bnn.manual_seed(SEED, OFF)
    want = ev.evaluate_batches(fzs[1], data[:1], S, acc=make() if make else None, posterior_mean=False)
    assert _same(res2["results"][1], want) and _same(accs[1].result(), want)


# --------------------------------------------------------------------------- 6. the chosen level goes on without a freeze
@pytest.mark.parametrize("case", tr.CASES[:2], ids=tr.IDS[:2])
def test_the_chosen_level_feeds_the_consumers(bnn, dev, case):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, masks, sw, fzs = _setup(bnn, dev, case, "four")
    lvl, one = sw.model(1), fzs[1]
    x = _x(dev, 65, dims[0])
    y = torch.randint(0, dims[-1], (65,), generator=torch.Generator().manual_seed(2)).to(dev)
    bnn.manual_seed(SEED, OFF)
    got = ev.explain_ensemble(lvl, x, 3, targets="pred")
    bnn.manual_seed(SEED, OFF)
    want = ev.explain_ensemble(one, x, 3, targets="pred")
    assert torch.equal(got["mean"], want["mean"]) and torch.equal(got["logits"], want["logits"])
    assert torch.equal(got["targets"], want["targets"])
    bnn.manual_seed(SEED, OFF)
    r = ev.ensemble_eval(lvl, x, y, 3)
    bnn.manual_seed(SEED, OFF)
    w = ev.ensemble_eval(one, x, y, 3)
    assert torch.equal(r["outputs"], w["outputs"]) and r["correct_ensemble"] == w["correct_ensemble"]
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(sw.ensemble(x, 3)[1], w["outputs"])


# --------------------------------------------------------------------------- 7. moved, copied, reloaded
@pytest.mark.parametrize("case", tr.CASES[1:3], ids=tr.IDS[1:3])
def test_a_moved_copied_or_reloaded_sweep_addresses_its_own_buffers(bnn, dev, case):
    ev = bnn.evaluate
    family, dims, T, head = case
    net, _, ref, _ = _setup(bnn, dev, case, "four")
    sw = ev.threshold_sweep(net, ref.thresholds)                            # one of its own: its buffers get scribbled on
    x = _x(dev, 65, dims[0])
    bnn.manual_seed(SEED, OFF)
    want = ref.ensemble(x, 2)
    bnn.manual_seed(SEED, OFF)
    want0 = ref(x)

    def check(s):
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(s.ensemble(x, 2), want)
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(s(x), want0)
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(s.model(2).ensemble(x, 2), want[2])
        assert s.nnz == ref.nnz and torch.equal(s.kept, ref.kept) and torch.equal(s.density, ref.density)

    def scribble(s):
        for _, b in s.named_buffers():
            b.fill_(float("nan")) if b.is_floating_point() else b.zero_()   # (zeros are in range for row_ptr and col)

    check(sw)                                                               # (and its level-0 model now exists)
    state = {k: v.clone() for k, v in sw.state_dict().items()}
    assert sorted(state) == sorted(k for k, _ in sw.named_buffers())
    twin = copy.deepcopy(sw)
    scribble(sw)
    check(twin)
    assert sw.to(dev) is sw
    sw.load_state_dict(state)
    check(sw)
    moved = twin.to(dev, torch.float32)
    check(moved)
    scribble(twin)
    twin.load_state_dict(sw.state_dict())
    check(twin)


# --------------------------------------------------------------------------- 8. refusals that need a device
def test_refusals_on_the_device(bnn, dev):
    ev = bnn.evaluate
    net, _, sw, _ = _setup(bnn, dev, tr.CASES[1], "four")
    x = _x(dev, 5, 64)
    with pytest.raises(ValueError, match=r"thresholds \* samples members in one launch, at most 65535; got 4 \* 16384"):
        sw.ensemble(x, 16384)
    with pytest.raises(ValueError, match="samples must be >= 1"):
        sw.ensemble(x, 0)
    with pytest.raises(RuntimeError, match="evaluates on a HIP device tensor"):
        sw.ensemble(x.cpu(), 2)
    with pytest.raises(RuntimeError, match="evaluates on a HIP device tensor"):
        sw(x.cpu())
    with pytest.raises(ValueError, match="log_probs=True applies"):
        sw.ensemble(x, 2, log_probs=True)
    with pytest.raises(ValueError, match="log_probs=True applies"):
        sw(x, log_probs=True)
    with pytest.raises(ValueError):
        ev.ensemble_forward(sw.model(0), x, 2, gates="mpm")
    with pytest.raises(ValueError, match="a head='log_softmax' sweep takes EvalAccumulators"):
        ev.sweep_batches(sw, [(x, None)], 2, accs=[ev.RegressionAccumulator(2, 2, dev, 0.0) for _ in range(4)])
    with pytest.raises(NotImplementedError, match="a sparse model does not refresh"):
        sw.model(1).refresh()
    _, _, reg, _ = _setup(bnn, dev, tr.CASES[4], "four")
    with pytest.raises(ValueError, match=r"head=\"identity\" \(regression\): accs must be 4 evaluate.RegressionAccumulator, got None"):
        ev.sweep_batches(reg, [(_x(dev, 5, 8), None)], 2)
    with pytest.raises(ValueError, match=r"accs must be 4 evaluate.RegressionAccumulator, got \['EvalAccumulator'\]"):
        ev.sweep_batches(reg, [(_x(dev, 5, 8), None)], 2, accs=[ev.EvalAccumulator(2, 2, dev) for _ in range(4)])
    dense = bnn.mnf.BayesianNetwork((20, 16, 12, 3), 2).to(dev)            # the reference's default: dense coupling z flows
    if dense.l1._check_flows() == "dense":
        with pytest.raises(ValueError, match=r"not built for dense coupling z flows.*dense=True"):
            ev.threshold_sweep(dense)
    with pytest.raises(TypeError, match=r"baseline.*freeze_base\(net, \"mpm\", threshold=t, sparse=True\)"):
        ev.threshold_sweep(bnn.base.BayesianNetwork((20, 16, 3)).to(dev))
    with pytest.raises(TypeError, match="variational-dropout"):
        ev.threshold_sweep(bnn.vd.BNN((20, 16, 3)).to(dev))
    first = net._layers()[0]
    first.noise = {"eps_out": torch.zeros(5, 48, device=dev)}
    try:
        with pytest.raises(ValueError, match="layer 1 has injected noise"):
            ev.threshold_sweep(net)
    finally:
        first.noise = None
