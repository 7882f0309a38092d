"""GPU tier of the baseline family's sparse median-probability model, ``evaluate.freeze_base(net, "mpm", sparse=True)``
(include/lbbnn.h: lbbnn_base_sparse_count / _pack / lbbnn_base_sparse_draw_members, and the member layer on stored values,
lbbnn_sparse_gather_members): the pack and the draws against the dense frozen model bit for bit; every member against an fp64
forward composed from the model's own weights; the bits; NaN-filled buffers; the evaluation stack; ``explain_ensemble`` on the
new model; the refusals that need a device.

Bars (the project's): TIGHT = 5e-6 as max|got - ref| / max|ref| for fp32 outputs and elementwise_violation <= 1 at TOL = 1e-4
(tests/test_frozen_sparse_gpu.py); the explanations' bars are tests/test_sparse_explain_gpu.py's (TIGHT, and |residual| <=
FP32_CEILING = 1e-5 of the sum of the absolute terms).  Inputs: tests/base_sparse_ref.py."""
import copy

import numpy as np
import pytest
import torch

import base_sparse_ref as br
import frozen_sparse_ref as sr
import sparse_explain_ref as xr
from conftest import elementwise_violation, rel_err

pytestmark = pytest.mark.gpu

TIGHT = 5e-6
TOL = 1e-4
FP32_CEILING = 1e-5
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


@pytest.fixture(scope="module")
def models(bnn, dev):
    """(net, sparse model, dense model) of a case and threshold, built once."""
    cache = {}

    def get(case, threshold=0.5):
        key = (case, threshold)
        if key not in cache:
            dims, head = case
            net = br.make_net(bnn, dev, dims, head, threshold)
            cache[key] = (net, br.freeze_sparse(bnn.evaluate, net, head, threshold), br.freeze_dense(bnn.evaluate, net, head, threshold))
        return cache[key]
    return get


def _case(name):
    return br.CASES[br.IDS.index(name)]


def _x(dev, B, I, seed=1):
    return torch.randn(B, I, generator=torch.Generator().manual_seed(seed + B)).to(dev)


def _np(t):
    return t.double().cpu().numpy()


def _offset(bnn, dev):
    return int(bnn.ops.RngState.get(dev).t[1])


def _csrs(fz):
    return [fz.csr(i)[:2] for i in range(fz.n_layers)]


# --------------------------------------------------------------------------- 1. the pack
def _check_pack(ev, net, fz, dense, threshold):
    layers = net._layers()
    masks = ev._base_keep_masks(layers, threshold)
    cut = sr.cut_of(threshold)
    total = 0
    for i, l in enumerate(layers):
        row_ptr, col, mean, sigma = fz.csr(i)
        O, I = l.out_features, l.in_features
        want_ptr, want_col, keep = sr.csr_of(l.lambdal.detach().cpu(), cut)
        assert torch.equal(keep, masks[i].cpu())              # (the inputs are unambiguous: either rule gives the kernel's mask)
        assert row_ptr.dtype == col.dtype == torch.int32
        assert torch.equal(row_ptr.cpu(), want_ptr) and torch.equal(col.cpu(), want_col)
        r, c = masks[i].nonzero(as_tuple=True)                # row-major: the CSR order
        for name, got, plane in (("mean", mean, "w_mu"), ("sigma", sigma, "w_sigma")):
            want = dense._buf(plane, i)[r, c]
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, i)
        assert torch.equal(mean, l.weight_mu.detach()[r, c])
        if r.numel():
            assert rel_err(sigma, torch.log1p(torch.exp(l.weight_rho.detach()[r, c].double()))) < TIGHT
        for name in ("b_mu", "b_sigma"):
            assert torch.equal(fz._buf(name, i).view(torch.int32), dense._buf(name, i).view(torch.int32)), (name, i)
        assert torch.equal(fz.kept_rows[i], dense.kept_rows[i])
        assert tuple(mean.shape) == tuple(sigma.shape) == tuple(col.shape) == (int(masks[i].sum()),)
        total += int(masks[i].sum())
    assert fz.kept == dense.kept and fz.density == dense.density
    assert fz.nnz == total
    assert fz.operand_bytes == sum(4 * (d + 1) + 8 * d for d in fz.dims[1:]) + 12 * total
    assert "sparse" in repr(fz) and "nnz=%d" % total in repr(fz) and "family=base" in repr(fz)
    assert fz.family == "base" and fz.gates == "mpm" and isinstance(fz, ev._FrozenModel)
    assert not any(k.startswith(("w_mu", "w_sigma", "e_w", "alpha")) for k, _ in fz.named_buffers())


@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("case", br.CASES, ids=br.IDS)
def test_pack_is_the_dense_models_planes(bnn, dev, models, case, threshold):
    """1. row_ptr / col / mean / sigma / b_mu / b_sigma: the bits of the dense frozen model's planes at the positions of its own
    keep masks; kept_rows, kept, density its own.  Everything is an equality."""
    net, fz, dense = models(case, threshold)
    _check_pack(bnn.evaluate, net, fz, dense, threshold)


# --------------------------------------------------------------------------- 2. the draws
def _check_draws(bnn, dev, fz, dense, x, S):
    bnn.manual_seed(SEED, OFF)
    got = fz.ensemble(x, S, keep_weights=True)
    assert _offset(bnn, dev) == OFF + S
    bnn.manual_seed(SEED, OFF)
    want = dense.ensemble(x, S, keep_weights=True)
    assert _offset(bnn, dev) == OFF + S
    for i in range(fz.n_layers):
        row_ptr, col, _, _ = fz.csr(i)
        nnz, O = col.numel(), fz.dims[i + 1]
        assert tuple(fz.last_weights[i].shape) == (S, nnz) and tuple(fz.last_biases[i].shape) == (S, O)
        r = br.rows_of(row_ptr)
        assert br.same_bits(fz.last_weights[i], dense.last_weights[i][:, r, col.long()]), i
        assert torch.equal(fz.last_biases[i].view(torch.int32), dense.last_biases[i].view(torch.int32)), i
        if S > 1 and nnz:
            assert bool((fz.last_weights[i][0] != fz.last_weights[i][1]).any())         # the members do differ
    return got, want


@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("case", br.CASES, ids=br.IDS)
def test_draws_are_the_dense_models_members(bnn, dev, models, case, threshold):
    """2. From the same seed and offset every kept weight of every member and every bias has the bits of the dense frozen
    model's member (a zero of either sign equals a zero), and both advance the offset by S; at threshold 0.5 the outputs equal
    base_ensemble(net, x, S, gates="mpm")'s within TIGHT.  Worst seen on the GPU (MI355X): the bits are equalities; against
    base_ensemble 3.7e-07."""
    ev = bnn.evaluate
    dims, head = case
    net, fz, dense = models(case, threshold)
    for B, S in sr.BS:
        x = _x(dev, B, dims[0])
        got, want = _check_draws(bnn, dev, fz, dense, x, S)
        if threshold == 0.5 and head != "identity":
            bnn.manual_seed(SEED, OFF)
            ref = ev.base_ensemble(net, x, S, gates="mpm")["outputs"]
            e = rel_err(got, ref)
            print("base_ensemble", dims, B, S, e)
            assert e < TIGHT


def test_pack_and_draws_of_the_reference_network(bnn, dev):
    """784-400-600-10 at (B, S) = (100, 10): the pack and the draws only."""
    ev = bnn.evaluate
    for threshold in sr.THRESHOLDS:
        net = br.make_net(bnn, dev, br.BIG, "log_softmax", threshold)
        fz, dense = br.freeze_sparse(ev, net, "log_softmax", threshold), br.freeze_dense(ev, net, "log_softmax", threshold)
        _check_pack(ev, net, fz, dense, threshold)
        _check_draws(bnn, dev, fz, dense, _x(dev, 100, 784), 10)


# --------------------------------------------------------------------------- 3. the outputs
@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("case", br.CASES, ids=br.IDS)
def test_outputs(bnn, dev, models, case, threshold):
    """3. Every member against the fp64 forward composed on the CPU from the model's own weights read back, and against the dense
    model's outputs; fz(x) against the dense fz(x) and the fp64 medimean, the offset unchanged.
    Worst seen on the GPU (MI355X), over every case, threshold and batch: against fp64 2.3e-07 (elementwise violation 0.04),
    against the dense model 3.7e-07; the medimean against fp64 2.1e-07, against the dense model 2.7e-07."""
    dims, head = case
    net, fz, dense = models(case, threshold)
    csrs = _csrs(fz)
    worst = dict(fp64=0.0, viol=0.0, dense=0.0, mean64=0.0, mean_dense=0.0)
    for B, S in sr.BS:
        x = _x(dev, B, dims[0])
        bnn.manual_seed(SEED, OFF)
        got = fz.ensemble(x, S, keep_weights=True)
        assert tuple(got.shape) == (S, B, dims[-1]) and got.dtype == torch.float32
        bnn.manual_seed(SEED, OFF)
        want_dense = dense.ensemble(x, S)
        ref = torch.stack([br.forward64(x, csrs, [w[m] for w in fz.last_weights], [b[m] for b in fz.last_biases], dims, head)
                           for m in range(S)])
        worst["fp64"] = max(worst["fp64"], rel_err(got, ref))
        worst["viol"] = max(worst["viol"], elementwise_violation(got, ref, rtol=TOL))
        worst["dense"] = max(worst["dense"], rel_err(got, want_dense))
        # the medimean forward: no draw, no advance
        bnn.manual_seed(SEED, OFF)
        mean = fz(x)
        assert _offset(bnn, dev) == OFF and tuple(mean.shape) == (B, dims[-1])
        ref_mean = br.forward64(x, csrs, [fz.csr(i)[2] for i in range(fz.n_layers)], [fz._buf("b_mu", i) for i in range(fz.n_layers)],
                                dims, head)
        worst["mean64"] = max(worst["mean64"], rel_err(mean, ref_mean))
        worst["mean_dense"] = max(worst["mean_dense"], rel_err(mean, dense(x)))
        assert _offset(bnn, dev) == OFF
    print("outputs", dims, threshold, worst)
    assert worst["fp64"] < TIGHT and worst["dense"] < TIGHT and worst["mean64"] < TIGHT and worst["mean_dense"] < TIGHT
    assert worst["viol"] <= 1.0


def test_sigmoid_head_log_probs(bnn, dev, models):
    """The sigmoid head as two classes: log_probs=True against fp64, for the ensemble and the medimean forward.  Worst seen on
    the GPU: 9.5e-08."""
    case = _case("20-1-sigmoid")
    for threshold in sr.THRESHOLDS:
        net, fz, dense = models(case, threshold)
        x = _x(dev, 65, 20)
        bnn.manual_seed(SEED, OFF)
        got = fz.ensemble(x, 3, log_probs=True, keep_weights=True)
        assert tuple(got.shape) == (3, 65, 2)
        ref = torch.stack([br.forward64(x, _csrs(fz), [w[m] for w in fz.last_weights], [b[m] for b in fz.last_biases], (20, 1),
                                        "sigmoid", True) for m in range(3)])
        e = rel_err(got, ref)
        bnn.manual_seed(SEED, OFF)
        e2 = rel_err(got, dense.ensemble(x, 3, log_probs=True))
        e3 = rel_err(fz(x, log_probs=True), dense(x, log_probs=True))
        print("sigmoid log_probs", threshold, e, e2, e3)
        assert e < TIGHT and e2 < TIGHT and e3 < TIGHT


# --------------------------------------------------------------------------- 4. the bits
@pytest.mark.parametrize("case", br.CASES, ids=br.IDS)
def test_bits(bnn, dev, models, case):
    """4. Two runs from one state; max_members=3 against unchunked; member m against a one-member call at offset + m; x[:64]
    against the first 64 rows of B = 257; fz(x, sample=True) against ensemble(x, 1)[0]; ensemble_forward(max_members=4)."""
    ev = bnn.evaluate
    dims, head = case
    net, fz, _ = models(case, 0.9)
    B, S = 257, 5
    x = _x(dev, B, dims[0])

    def run(xs, s, off=OFF, **kw):
        bnn.manual_seed(SEED, off)
        return fz.ensemble(xs, s, **kw)
    a = run(x, S)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, run(x, S))
    assert torch.equal(a, run(x, S, max_members=3)) and _offset(bnn, dev) == OFF + S
    for m in range(S):
        assert torch.equal(run(x, 1, OFF + m)[0], a[m]), m
    assert torch.equal(run(x[:64], S), a[:, :64])
    bnn.manual_seed(SEED, OFF)
    one = fz(x, sample=True)
    assert _offset(bnn, dev) == OFF + 1 and torch.equal(one, a[0])
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(ev.ensemble_forward(fz, x, S, max_members=4), a)
    with pytest.raises(ValueError, match="fixed by evaluate.freeze"):
        ev.ensemble_forward(fz, x, S, gates="mpm")


def _c_calls(fn):
    from bnn_amd import _lib
    _lib.RECORD = []
    try:
        fn()
        return [r[0].replace("lbbnn_", "") for r in _lib.RECORD]
    finally:
        _lib.RECORD = None


@pytest.mark.parametrize("name,head_call", [("16-16-16-16-16-4", ["log_softmax_rows"]), ("8-12-20-18", ["log_softmax_rows"]),
                                            ("20-1-sigmoid", ["binary_head"]), ("8-32-2-identity", [])])
def test_launch_sequence(bnn, dev, models, name, head_call):
    """The C calls of one call: ceil(n / 4) draws, one layer launch per layer and the offset's advance per chunk, after ONE input
    transpose, then at most one head launch whatever S; the medimean forward makes no draw and advances nothing."""
    case = _case(name)
    dims, head = case
    net, fz, _ = models(case)
    n = len(dims) - 1
    x = _x(dev, 65, dims[0])
    chunk = ["base_sparse_draw_members"] * -(-n // 4) + ["sparse_gather_members"] * n + ["rng_advance"]
    assert _c_calls(lambda: fz.ensemble(x, 7)) == ["transpose_operand"] + chunk + head_call
    assert _c_calls(lambda: fz.ensemble(x, 7, max_members=3)) == ["transpose_operand"] + 3 * chunk + head_call
    bnn.manual_seed(SEED, OFF)
    assert _c_calls(lambda: fz(x)) == ["transpose_operand"] + ["sparse_gather_members"] * n + head_call
    assert _offset(bnn, dev) == OFF


# --------------------------------------------------------------------------- 5. every buffer is written
def _nan_empty(*size, **kw):
    fill = float("nan") if kw.get("dtype", torch.float32).is_floating_point else 255
    return torch.full(*size, fill, **kw) if len(size) == 1 else torch.full(size, fill, **kw)


@pytest.mark.parametrize("case", [_case("13-9-3"), _case("76-12-5"), _case("16-16-16-16-16-4"), _case("20-1-sigmoid")],
                         ids=["13-9-3", "76-12-5", "16-16-16-16-16-4", "20-1-sigmoid"])
def test_nan_filled_buffers(bnn, dev, models, monkeypatch, case):
    """5. Every buffer (the CSR, the members' weights and biases, x^T, the activations, the outputs) handed out full of NaN:
    the results are the clean ones, and every padded tail of w / b is zero."""
    ev, ops = bnn.evaluate, bnn.ops
    dims, head = case
    net, fz0, _ = models(case, 0.9)
    x = _x(dev, 65, dims[0])
    bnn.manual_seed(SEED, OFF)
    clean = fz0.ensemble(x, 3)
    clean_mean = fz0(x)
    monkeypatch.setattr(ev, "_empty", _nan_empty)
    fz = br.freeze_sparse(ev, net, head, 0.9)
    for name, buf in fz.named_buffers():
        assert bool(torch.isfinite(buf.float()).all()), name
        assert torch.equal(buf, dict(fz0.named_buffers())[name]), name
    bnn.manual_seed(SEED, OFF)
    out = fz.ensemble(x, 3)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, clean) and torch.equal(fz(x), clean_mean)
    # the draw's own buffers, tails included
    st = ops.RngState.get(dev)
    for tpos in (None, [ev._transposed_pattern(fz, i)[3] for i in range(fz.n_layers)]):
        wb = fz._draw(3, st.t, torch.cuda.current_stream(dev).cuda_stream, tpos=tpos)
        for i, (w, b, wt) in enumerate(wb):
            nnz, O = fz.csr(i)[1].numel(), dims[i + 1]
            assert tuple(w.shape) == (3, ops.pad4(nnz)) and tuple(b.shape) == (3, ops.pad4(O))
            assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all())
            assert bool((w[:, nnz:] == 0).all()) and bool((b[:, O:] == 0).all())
            if wt is not None:
                assert bool((wt[:, nnz:] == 0).all())
                assert torch.equal(wt[:, tpos[i].long()], w[:, :nnz])          # slot k stands at place tpos[k]


def test_a_layer_that_keeps_nothing(bnn, dev, monkeypatch):
    """(20, 1) with every lambdal below the cut: nnz = 0, the members are sigmoid(b), and nothing launches on a NULL pattern."""
    ev = bnn.evaluate
    net = br.make_net(bnn, dev, (20, 1), "sigmoid", 0.5)
    with torch.no_grad():
        net.l1.lambdal.fill_(-2.0)
    monkeypatch.setattr(ev, "_empty", _nan_empty)
    fz = ev.freeze_base(net, "mpm", sparse=True)
    assert fz.nnz == 0 and fz.kept == [0] and fz.density == 0.0
    assert fz.csr(0)[0].tolist() == [0, 0] and fz.csr(0)[1].numel() == 0
    x = _x(dev, 65, 20)
    bnn.manual_seed(SEED, OFF)
    out = fz.ensemble(x, 4, keep_weights=True)
    assert _offset(bnn, dev) == OFF + 4
    assert tuple(fz.last_weights[0].shape) == (4, 0)
    want = torch.sigmoid(fz.last_biases[0].double())[:, None, :].expand(4, 65, 1)
    assert rel_err(out, want) < TIGHT
    assert rel_err(fz(x), torch.sigmoid(net.l1.bias_mu.detach().double()).expand(65, 1)) < TIGHT
    dense = ev.freeze_base(net, "mpm")
    bnn.manual_seed(SEED, OFF)
    assert rel_err(out, dense.ensemble(x, 4)) < TIGHT


def test_empty_batch(bnn, dev, models):
    net, fz, _ = models(_case("13-9-3"))
    bnn.manual_seed(SEED, OFF)
    out = fz.ensemble(torch.zeros(0, 13, device=dev), 3)
    assert tuple(out.shape) == (3, 0, 3) and _offset(bnn, dev) == OFF + 3
    assert tuple(fz(torch.zeros(0, 13, device=dev)).shape) == (0, 3) and _offset(bnn, dev) == OFF + 3


# --------------------------------------------------------------------------- 6. the stack
def test_ensemble_eval_and_evaluate_batches(bnn, dev, models):
    """6. ensemble_eval and evaluate_batches with both accumulators are the dense model's numbers' keys, computed from this
    model's own outputs."""
    ev = bnn.evaluate
    dims, head = case = _case("50-37-29-3")
    net, fz, dense = models(case)
    B, C, S = 40, 3, 4
    g = torch.Generator().manual_seed(4)
    data = [(torch.randn(B, 50, generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)) for _ in range(3)]
    bnn.manual_seed(SEED, OFF)
    res = ev.ensemble_eval(fz, data[0][0], data[0][1], S)
    bnn.manual_seed(SEED, OFF)
    outputs = fz.ensemble(data[0][0], S)
    assert torch.equal(res["outputs"], outputs)
    assert torch.equal(res["pred_ensemble"], outputs.mean(0).argmax(1))
    assert torch.equal(res["pred_posterior_mean"], fz(data[0][0]).argmax(1))
    assert torch.equal(res["density"], torch.full((S,), fz.density, device=dev))
    assert res["correct_ensemble"] == int(outputs.mean(0).argmax(1).eq(data[0][1]).sum())
    acc, unc = ev.EvalAccumulator(C, S, dev), ev.UncertaintyAccumulator(C, S, dev)
    bnn.manual_seed(SEED, OFF)
    got = ev.evaluate_batches(fz, data, S, acc=acc, uncertainty=unc)
    assert _offset(bnn, dev) == OFF + 3 * S and got["rows"] == 3 * B
    acc2, unc2 = ev.EvalAccumulator(C, S, dev), ev.UncertaintyAccumulator(C, S, dev)
    bnn.manual_seed(SEED, OFF)
    for xb, yb in data:
        o = fz.ensemble(xb, S)
        acc2.update(o, yb, fz(xb))
        unc2.update(o, yb)
    assert torch.equal(acc._totals, acc2._totals) and torch.equal(unc._totals, unc2._totals)


def test_sigmoid_head_through_the_accumulators(bnn, dev, models):
    ev = bnn.evaluate
    net, fz, _ = models(_case("20-1-sigmoid"))
    B, S = 40, 4
    g = torch.Generator().manual_seed(4)
    data = [(torch.randn(B, 20, generator=g).to(dev), torch.randint(0, 2, (B,), generator=g).float().to(dev)) for _ in range(2)]
    acc, unc = ev.EvalAccumulator(2, S, dev), ev.UncertaintyAccumulator(2, S, dev)
    bnn.manual_seed(SEED, OFF)
    got = ev.evaluate_batches(fz, data, S, acc=acc, uncertainty=unc)
    assert got["rows"] == 2 * B
    acc2 = ev.EvalAccumulator(2, S, dev)
    bnn.manual_seed(SEED, OFF)
    for xb, yb in data:
        acc2.update(fz.ensemble(xb, S, log_probs=True), yb.long(), fz(xb, log_probs=True))
    assert torch.equal(acc._totals, acc2._totals)


@pytest.mark.parametrize("case", [_case("50-37-29-3"), _case("8-12-20-18"), _case("20-1-sigmoid")],
                         ids=["50-37-29-3", "8-12-20-18", "20-1-sigmoid"])
def test_graphed_eval_step(bnn, dev, models, case):
    """6. Replays of make_graphed_eval_step give the eager results bitwise from the same offset, and the accumulator's totals are
    those of evaluate_batches over the same batches."""
    ev = bnn.evaluate
    dims, head = case
    net, fz, _ = models(case)
    binary = head == "sigmoid"
    B, C, members = 40, 2 if binary else dims[-1], 4
    g = torch.Generator().manual_seed(4)
    ys = [torch.randint(0, C, (B,), generator=g) for _ in range(3)]
    data = [(torch.randn(B, dims[0], generator=g).to(dev), (y.float() if binary else y).to(dev)) for y in ys]
    acc_g = ev.EvalAccumulator(C, members, dev)
    step = bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], members, acc_g)
    bnn.manual_seed(SEED, OFF)
    got = [{k: v.clone() for k, v in step(xb, yb).items()} for xb, yb in data]
    assert bnn.ops.RngState.get(dev).t[:2].tolist() == [SEED, OFF + 3 * members]
    acc_e = ev.EvalAccumulator(C, members, dev)
    bnn.manual_seed(SEED, OFF)
    for (xb, yb), rows_g in zip(data, got):
        rows_e = acc_e.update(fz.ensemble(xb, members, log_probs=binary), yb.long() if binary else yb,
                              fz(xb, sample=False, log_probs=binary))
        assert sorted(rows_e) == sorted(rows_g)
        for k in rows_e:
            assert torch.equal(rows_e[k], rows_g[k]), k
    assert torch.equal(acc_g._totals, acc_e._totals) and acc_g.updates == 3
    acc_b = ev.EvalAccumulator(C, members, dev)
    bnn.manual_seed(SEED, OFF)
    res = ev.evaluate_batches(fz, data, members, acc=acc_b)
    assert torch.equal(acc_b._totals, acc_g._totals) and res["rows"] == 3 * B


def test_a_copied_or_moved_model_addresses_its_own_buffers(bnn, dev, models):
    ev = bnn.evaluate
    net = br.make_net(bnn, dev, (13, 9, 3), "log_softmax", 0.5)
    x = _x(dev, 5, 13)
    fz = ev.freeze_base(net, "mpm", sparse=True)
    bnn.manual_seed(SEED, OFF)
    want = fz.ensemble(x, 3)
    twin = copy.deepcopy(fz)
    for i in range(2):
        fz.csr(i)[2].fill_(float("nan"))                          # the original's values are no longer usable
        fz._buf("b_mu", i).fill_(float("nan"))
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(twin.ensemble(x, 3), want)
    old = dict(twin.named_buffers())
    moved = twin.double().float()                                # every float buffer replaced (a cast leaves int32 ones in place)
    for k, b in moved.named_buffers():
        if b.is_floating_point():
            assert b.data_ptr() != old[k].data_ptr(), k
            old[k].fill_(float("nan"))                           # still alive: a stale address reads NaN, not freed memory
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(moved.ensemble(x, 3), want)
    moved = moved.to(dev)
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(moved.ensemble(x, 3), want)
    with pytest.raises(RuntimeError, match="data is on"):
        moved.cpu().ensemble(x, 3)


# --------------------------------------------------------------------------- 7. the explanations
def _targets_of(case, B, dev):
    """Every output where C <= 16; "pred" and a target tensor on the 18-class case (by batch size)."""
    C = case[0][-1]
    if C <= 16:
        return None
    return "pred" if B != 65 else (torch.arange(B, device=dev) * 7) % C


@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("B,S", xr.BS)
@pytest.mark.parametrize("case", br.CASES, ids=br.IDS)
def test_explanations(bnn, dev, models, case, B, S, threshold):
    """7. explain_ensemble on the new model: weights / biases are fz.ensemble's from the same offset, bit for bit (an identity
    head: the logits too); every member's logits, contributions and intercept and the statistics against
    tests/sparse_explain_ref.py in fp64 within TIGHT, |residual| within FP32_CEILING of the sum of the absolute terms.
    Worst seen on the GPU (MI355X): logits 3.9e-07, members 2.0e-07, intercept 2.4e-07, mean 1.2e-07, std 2.7e-06 (two members of
    the 20 -> 1 network), residual 1.9e-07 of the terms."""
    ev = bnn.evaluate
    dims, head = case
    net, fz, _ = models(case, threshold)
    x = _x(dev, B, dims[0])
    C, F = dims[-1], dims[0]
    bnn.manual_seed(SEED, OFF)
    outputs = fz.ensemble(x, S, keep_weights=True)
    lw, lb = fz.last_weights, fz.last_biases
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, S, targets=_targets_of(case, B, dev), keep_members=True, keep_weights=True, keep_masks=True)
    assert _offset(bnn, dev) == OFF + S and "z" not in res
    for i in range(fz.n_layers):
        assert torch.equal(res["weights"][i].view(torch.int32), lw[i].view(torch.int32)), i
        assert torch.equal(res["biases"][i].view(torch.int32), lb[i].view(torch.int32)), i
    if head == "identity":
        assert torch.equal(res["logits"].view(torch.int32), outputs.view(torch.int32))
    elif head == "log_softmax":
        assert rel_err(torch.log_softmax(res["logits"].double(), -1), outputs) < TIGHT
    Cp = C if res["targets"] is None else 1
    for k in ("mean", "std", "prob_positive", "prob_negative"):
        assert tuple(res[k].shape) == (B, Cp, F) and res[k].dtype == torch.float32
    assert tuple(res["logits"].shape) == (S, B, C) and tuple(res["members"].shape) == (S, B, Cp, F)
    assert tuple(res["intercept"].shape) == tuple(res["residual"].shape) == (S, B, Cp)
    if C > 16 and B != 65:
        assert torch.equal(res["targets"], res["logits"].mean(0).argmax(1))
    # every member and the statistics against fp64 on the device's own weights, biases and masks
    csrs = _csrs(fz)
    t = None if res["targets"] is None else res["targets"].cpu().numpy()
    refs = []
    for m in range(S):
        Ws, bs = xr.dense_member(csrs, res["weights"], res["biases"], dims, m)
        refs.append(xr.member_ref(Ws, bs, _np(x), [_np(k[m]) > 0 for k in res["masks"]], t))
    want = dict((k, np.stack([r[k] for r in refs])) for k in ("contributions", "intercept", "logits", "terms"))
    mean, std, _, _ = xr.stats_ref(want["contributions"])
    errs = dict(logits=rel_err(res["logits"], want["logits"]), members=rel_err(res["members"], want["contributions"]),
                intercept=rel_err(res["intercept"], want["intercept"]), mean=rel_err(res["mean"], mean))
    if S > 1:
        errs["std"] = rel_err(res["std"], std)
    else:
        assert bool((res["std"] == 0).all())
    errs["residual"] = float((np.abs(_np(res["residual"])) / want["terms"]).max())
    print("explain_ensemble errors", tuple(dims), B, S, threshold, errs)
    for k, v in errs.items():
        assert v <= (FP32_CEILING if k == "residual" else TIGHT), (k, v)
    got = res["members"]
    assert torch.equal(res["prob_positive"], ((got > 0).sum(0).double() / S).float())
    assert torch.equal(res["prob_negative"], ((got < 0).sum(0).double() / S).float())


def test_a_feature_without_a_kept_path(bnn, dev):
    """Column 0 of layer 1 is kept by its row 1 only; with unit 1's consumers pruned in layer 2, feature 0 has no kept path:
    exactly 0.0 in every member and every statistic, while its neighbour is not."""
    ev = bnn.evaluate
    dims = (50, 37, 29, 3)
    net = br.make_net(bnn, dev, dims, "log_softmax", 0.5)
    lams = sr.lambdals(dims, 0.5)[0]
    lams[1][:, 1] = -2.0
    sr.apply(net, lams)
    fz = ev.freeze_base(net, "mpm", sparse=True)
    assert not bool((fz.csr(1)[1] == 1).any())
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, _x(dev, 65, 50), 3, keep_members=True)
    for k in ("members", "mean", "std", "prob_positive", "prob_negative"):
        assert bool((res[k][..., 0] == 0).all()), k
    assert bool((res["members"][..., 1] != 0).any()) and bool((res["std"][..., 1] > 0).any())


@pytest.mark.parametrize("case", br.CASES, ids=br.IDS)
def test_the_medimean_explanation(bnn, dev, models, case):
    """weight_noise=False, samples=1: the explanation of the medimean network, against fp64; nothing is drawn.  Also: two calls
    from one state give the same bits.  Worst seen on the GPU: 3.5e-07."""
    ev = bnn.evaluate
    dims, head = case
    net, fz, _ = models(case)
    B = 65
    x = _x(dev, B, dims[0])
    targets = _targets_of(case, B, dev)
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, 1, weight_noise=False, targets=targets, keep_weights=True, keep_masks=True, keep_members=True)
    assert _offset(bnn, dev) == OFF
    n = fz.n_layers
    for i in range(n):
        assert torch.equal(res["weights"][i][0], fz.csr(i)[2]) and torch.equal(res["biases"][i][0], fz._buf("b_mu", i))
    Ws, bs = xr.dense_member(_csrs(fz), [fz.csr(i)[2][None] for i in range(n)], [fz._buf("b_mu", i)[None] for i in range(n)], dims, 0)
    t = None if res["targets"] is None else res["targets"].cpu().numpy()
    ref = xr.member_ref(Ws, bs, _np(x), [_np(k[0]) > 0 for k in res["masks"]], t)
    errs = (rel_err(res["mean"], ref["contributions"]), rel_err(res["logits"][0], ref["logits"]),
            rel_err(res["intercept"][0], ref["intercept"]))
    print("medimean explanation", dims, errs)
    assert max(errs) <= TIGHT and bool((res["std"] == 0).all())
    if head == "identity":
        assert torch.equal(res["logits"][0], fz(x))
    with pytest.raises(ValueError, match="ONE member"):
        ev.explain_ensemble(fz, x, 2, weight_noise=False, targets=targets)
    # two calls from one state
    bnn.manual_seed(SEED, OFF)
    a = ev.explain_ensemble(fz, x, 3, targets=targets, keep_members=True)
    bnn.manual_seed(SEED, OFF)
    b = ev.explain_ensemble(fz, x, 3, targets=targets, keep_members=True)
    for k in ("mean", "std", "prob_positive", "prob_negative", "logits", "intercept", "residual", "members"):
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k


def test_explanation_of_an_empty_batch(bnn, dev, models):
    ev = bnn.evaluate
    net, fz, _ = models(_case("13-9-3"))
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, torch.zeros(0, 13, device=dev), 3, keep_members=True, keep_weights=True)
    assert _offset(bnn, dev) == OFF + 3
    assert tuple(res["mean"].shape) == (0, 3, 13) and tuple(res["logits"].shape) == (3, 0, 3)
    assert tuple(res["members"].shape) == (3, 0, 3, 13) and tuple(res["weights"][0].shape) == (3, fz.csr(0)[1].numel())


# --------------------------------------------------------------------------- 8. the refusals that need a device
def test_refusals(bnn, dev, models):
    ev = bnn.evaluate
    net, fz, dense = models(_case("13-9-3"))
    x = _x(dev, 4, 13)
    off = _offset(bnn, dev)
    with pytest.raises(ValueError, match=r"explain_ensemble\(fz, data, samples=1, weight_noise=False\)"):
        ev.explain(fz, x)
    with pytest.raises(TypeError, match=r"freeze_base\(net, \"mpm\", sparse=True\)"):
        ev.explain_ensemble(dense, x)
    with pytest.raises(TypeError, match=r"freeze_base\(net, \"mpm\", sparse=True\)"):
        ev.explain_ensemble(net, x)
    with pytest.raises(ValueError, match=r"sparse=True needs gates=\"mpm\""):
        ev.freeze_base(net, "sample", sparse=True)
    with pytest.raises(ValueError, match="sparse=True with compact=True"):
        ev.freeze_base(net, "mpm", sparse=True, compact=True)
    with pytest.raises(NotImplementedError, match="freeze again"):
        fz.refresh()
    net.l1.noise = {"eps_w": torch.zeros(9, 13, device=dev)}
    try:
        with pytest.raises(ValueError, match="injected noise"):
            ev.freeze_base(net, "mpm", sparse=True)
    finally:
        net.l1.noise = None
    with pytest.raises(RuntimeError, match="no CPU path"):
        fz.ensemble(x.cpu(), 2)
    with pytest.raises(ValueError, match="log_probs=True applies"):
        fz.ensemble(x, 2, log_probs=True)
    assert _offset(bnn, dev) == off                           # a refused call draws nothing
