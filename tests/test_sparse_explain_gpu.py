"""GPU tier of evaluate.explain_ensemble (include/lbbnn.h: lbbnn_sparse_draw_members / lbbnn_sparse_gather_members /
lbbnn_explain_seed / lbbnn_explain_member_stats): the drawn weights against the regenerated Philox draws; every member's
logits, contributions and intercept, and the statistics over the members, against the float64 oracle on the device's own
weights, biases and masks; the cross-checks with evaluate.explain and with the mean network; the one-layer network bit for bit;
the values read through tslot against the column-by-column values the sweep uses; a feature that loses every kept path in a
three-layer network; the distribution of the members' logits against the variance the local-reparameterisation epilogue uses;
the bits; the refusals.

Bars: TIGHT = 5e-6 as max|got - ref| / max|ref| (the fp32 bar of tests/test_frozen_sparse_gpu.py); |residual| <= FP32_CEILING =
1e-5 of the sum of the absolute terms (tests/test_explain_gpu.py); a drawn weight within 4 * 2^-24 * (|mean z| + sqrt(var)
|eps|).  Inputs: tests/sparse_explain_ref.py."""
import numpy as np
import pytest
import torch

import frozen_sparse_ref as sr
import sparse_explain_ref as xr
from conftest import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 5e-6
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
    """(net, sparse model) of a case and threshold, built once."""
    cache = {}

    def get(case, threshold=0.5):
        key = (sr.CASES.index(case), threshold)
        if key not in cache:
            family, dims, T, head = case
            torch.manual_seed(11)
            if family == "lrt":
                net = bnn.lrt.BayesianNetwork(dims, head=head)
            else:
                net = bnn.mnf.BayesianNetwork(dims, T, z_flow_type="Planar", r_flow_type="Planar", head=head)
            g = torch.Generator().manual_seed(12)
            with torch.no_grad():
                for l in net._layers():
                    # (as tests/explain_ref.py: the input path must not vanish beside the bias path, and z sits around 1)
                    l.weight_mu.copy_(torch.randn(l.weight_mu.shape, generator=g) * (4.0 / l.in_features) ** 0.5)
                    l.bias_mu.copy_(torch.randn(l.bias_mu.shape, generator=g) * 0.5)
                    if family == "mnf":
                        l.q0_mean.copy_(1.0 + 0.1 * torch.randn(l.q0_mean.shape, generator=g))
            net = net.to(dev).eval()
            sr.apply(net, sr.lambdals(dims, threshold)[0])
            cache[key] = (net, bnn.evaluate.freeze(net, "mpm", threshold=threshold, sparse=True))
        return cache[key]
    return get


def _case(name):
    return sr.CASES[sr.IDS.index(name)]


ONE_LAYER = _case("lrt-20-1")


def _x(dev, B, I, seed=1):
    return torch.randn(B, I, generator=torch.Generator().manual_seed(seed + B)).to(dev)


def _targets_of(case, B, dev):
    """The issue's choice: every output where C <= 16; "pred" and a target tensor on the 20-class cases (by batch size)."""
    C = case[1][-1]
    if C <= 16:
        return None
    return "pred" if B != 65 else (torch.arange(B, device=dev) * 7) % C


def _np(t):
    return t.double().cpu().numpy()


def _offset(bnn, dev):
    return int(bnn.ops.RngState.get(dev).t[1])


# --------------------------------------------------------------------------- 1. the draws
@pytest.mark.parametrize("case", xr.CASES, ids=xr.IDS)
def test_draws(bnn, dev, models, case):
    ev, ops = bnn.evaluate, bnn.ops
    family, dims, _, _ = case
    net, fz = models(case)
    B, S = 65, 3
    x = _x(dev, B, dims[0])
    bnn.manual_seed(SEED, OFF)
    fz.ensemble(x, S, keep_z=True)
    want_z = fz.last_z
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, S, targets=_targets_of(case, B, dev), keep_weights=True)
    assert _offset(bnn, dev) == OFF + S
    if family == "mnf":
        assert all(torch.equal(a, b) for a, b in zip(res["z"], want_z))
        assert all(tuple(z.shape) == (S, dims[i]) for i, z in enumerate(res["z"]))
    else:
        assert "z" not in res
    for i, l in enumerate(net._layers()):
        _, col, mean, var = fz.csr(i)
        nnz, O = col.numel(), dims[i + 1]
        assert tuple(res["weights"][i].shape) == (S, nnz) and tuple(res["biases"][i].shape) == (S, O)
        for m in range(S):
            rng_m = torch.tensor([SEED, OFF + m], dtype=torch.int64, device=dev)
            eps = ops.philox_normal(rng_m, ops.STREAM_EPS_W * 64 + l._layer_id, -(-nnz // 4), 4).flatten()[:nnz]
            zcol = res["z"][i][m][col.long()] if family == "mnf" else None
            want, bound = xr.draw_ref(mean, var, eps, zcol)
            assert bool(((res["weights"][i][m].double() - want).abs() <= bound).all()), (i, m)
            eps = ops.philox_normal(rng_m, ops.STREAM_EPS_B * 64 + l._layer_id, -(-O // 4), 4).flatten()[:O]
            want, bound = xr.draw_ref(fz._buf("bias_mu", i), fz._buf("bias_var", i), eps)
            assert bool(((res["biases"][i][m].double() - want).abs() <= bound).all()), (i, m)
        assert bool((res["weights"][i][0] != res["weights"][i][1]).any())             # the members do differ


# --------------------------------------------------------------------------- 2. members against fp64
def _check_against_oracle(fz, x, res, S):
    """Every member and the statistics against tests/sparse_explain_ref.py on the device's own weights, biases and masks."""
    dims, B = fz.dims, x.shape[0]
    csrs = [fz.csr(i)[:2] for i in range(fz.n_layers)]
    t = None if res["targets"] is None else res["targets"].cpu().numpy()
    xs = _np(x)
    refs = []
    for m in range(S):
        Ws, bs = xr.dense_member(csrs, res["weights"], res["biases"], dims, m)
        refs.append(xr.member_ref(Ws, bs, xs, [_np(k[m]) > 0 for k in res["masks"]], t))
    want = dict((k, np.stack([r[k] for r in refs])) for k in ("contributions", "intercept", "logits", "terms"))
    mean, std, pos, neg = xr.stats_ref(want["contributions"])
    errs = dict(logits=rel_err(res["logits"], want["logits"]), members=rel_err(res["members"], want["contributions"]),
                intercept=rel_err(res["intercept"], want["intercept"]), mean=rel_err(res["mean"], mean))
    if S > 1:
        errs["std"] = rel_err(res["std"], std)
    else:
        assert bool((res["std"] == 0).all())
    errs["residual"] = float((np.abs(_np(res["residual"])) / want["terms"]).max())
    print("explain_ensemble errors", tuple(dims), B, S, errs)
    for k, v in errs.items():
        assert v <= (FP32_CEILING if k == "residual" else TIGHT), (k, v)
    # the sign probabilities: the counts of the device's own members over S, exactly
    got = res["members"]
    assert torch.equal(res["prob_positive"], ((got > 0).sum(0).double() / S).float())
    assert torch.equal(res["prob_negative"], ((got < 0).sum(0).double() / S).float())
    return want


@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("B,S", xr.BS)
@pytest.mark.parametrize("case", xr.CASES, ids=xr.IDS)
def test_members_against_fp64(bnn, dev, models, case, B, S, threshold):
    ev = bnn.evaluate
    family, dims, _, _ = case
    net, fz = models(case, threshold)
    x = _x(dev, B, dims[0])
    C, F = dims[-1], dims[0]
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, S, targets=_targets_of(case, B, dev), keep_members=True, keep_weights=True, keep_masks=True)
    Cp = C if res["targets"] is None else 1
    for k in ("mean", "std", "prob_positive", "prob_negative"):
        assert tuple(res[k].shape) == (B, Cp, F) and res[k].dtype == torch.float32
    assert tuple(res["logits"].shape) == (S, B, C) and tuple(res["members"].shape) == (S, B, Cp, F)
    assert tuple(res["intercept"].shape) == tuple(res["residual"].shape) == (S, B, Cp)
    # "pred": the first largest member-mean logit, the mean an fp32 sum in member order over S (include/lbbnn.h,
    # lbbnn_explain_seed) -- for the S = 2 and 3 of these cases that is torch's own mean, bit for bit
    if C > 16 and B != 65:
        assert torch.equal(res["targets"], res["logits"].mean(0).argmax(1))
    _check_against_oracle(fz, x, res, S)
    # a feature with no kept path is exactly 0.0 everywhere: column 0 of the first layer is kept by its row 1 alone (a layer of
    # one row: by nothing), and row 1 of the next layer's pattern ... -- so decide it from the structure itself
    reach = torch.ones(C, dtype=torch.bool)
    for i in range(fz.n_layers - 1, -1, -1):
        row_ptr, col, _, _ = [t.cpu() for t in fz.csr(i)]
        keep = sr.decode(row_ptr, col, torch.ones(col.numel()), dims[i + 1], dims[i]) > 0
        reach = (keep & reach[:, None]).any(0)
    dead = ~reach
    if len(dims) == 2:
        assert bool(dead[0])                                  # the 20 -> 1 network keeps nothing of column 0
    for k in ("members", "mean", "std", "prob_positive", "prob_negative"):
        assert bool((res[k][..., dead.to(dev)] == 0).all()), k


# --------------------------------------------------------------------------- 3. the cross-checks with tested code
@pytest.mark.parametrize("case", [c for c in xr.CASES if c[0] == "lrt"], ids=[i for i, c in zip(xr.IDS, xr.CASES) if c[0] == "lrt"])
def test_mean_network_equals_explain_of_the_dense_model(bnn, dev, models, case):
    ev = bnn.evaluate
    net, fz = models(case)
    C = case[1][-1]
    x = _x(dev, 65, case[1][0])
    t = None if C <= 16 else (torch.arange(65, device=dev) * 7) % C       # (20 classes: one output per row, which explain takes too)
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, 1, weight_noise=False, targets=t)
    assert _offset(bnn, dev) == OFF                           # nothing was drawn
    want = ev.explain(ev.freeze(net, "mpm"), x, targets=t)
    assert rel_err(res["mean"], want["contributions"]) <= TIGHT
    assert rel_err(res["logits"][0], want["logits"]) <= TIGHT and rel_err(res["intercept"][0], want["intercept"]) <= TIGHT
    assert bool((res["std"] == 0).all())


@pytest.mark.parametrize("case", [c for c in xr.CASES if c[0] == "mnf"], ids=[i for i, c in zip(xr.IDS, xr.CASES) if c[0] == "mnf"])
def test_mnf_mean_network_under_its_own_z(bnn, dev, models, case):
    ev = bnn.evaluate
    _, dims, _, _ = case
    net, fz = models(case)
    B, S = 65, 3
    x = _x(dev, B, dims[0])
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, S, targets=_targets_of(case, B, dev), weight_noise=False, keep_members=True,
                              keep_weights=True, keep_masks=True)
    assert _offset(bnn, dev) == OFF + S
    for i in range(fz.n_layers):                              # the weights are mean * z[col] in fp32, the biases bias_mu
        _, col, mean, _ = fz.csr(i)
        assert torch.equal(res["weights"][i], mean[None, :] * res["z"][i][:, col.long()])
        assert torch.equal(res["biases"][i], fz._buf("bias_mu", i)[None, :].expand(S, -1))
    # ... and every member equals the fp64 mean network under z[m], built from the model's own mean and the returned z
    csrs = [fz.csr(i)[:2] for i in range(fz.n_layers)]
    weights = [fz.csr(i)[2].double()[None, :] * res["z"][i].double()[:, fz.csr(i)[1].long()] for i in range(fz.n_layers)]
    biases = [fz._buf("bias_mu", i).double()[None, :].expand(S, -1) for i in range(fz.n_layers)]
    t = None if res["targets"] is None else res["targets"].cpu().numpy()
    for m in range(S):
        Ws, bs = xr.dense_member(csrs, weights, biases, dims, m)
        ref = xr.member_ref(Ws, bs, _np(x), [_np(k[m]) > 0 for k in res["masks"]], t)
        assert rel_err(res["members"][m], ref["contributions"]) <= TIGHT
        assert rel_err(res["logits"][m], ref["logits"]) <= TIGHT


# --------------------------------------------------------------------------- 4. one layer
def test_one_layer_is_the_product_bit_for_bit(bnn, dev, models):
    ev = bnn.evaluate
    net, fz = models(ONE_LAYER)
    B, S = 65, 3
    x = _x(dev, B, 20)
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, S, keep_members=True, keep_weights=True)
    _, col, _, _ = fz.csr(0)
    w = torch.zeros(S, 20, device=dev)
    w[:, col.long()] = res["weights"][0]                      # one row: slot(i) is the place of i in col
    want = w[:, None, :] * x[None, :, :]
    assert torch.equal(res["members"][:, :, 0, :].view(torch.int32), want.view(torch.int32))
    assert torch.equal(res["intercept"][:, :, 0], res["biases"][0][:, :1].expand(S, B))


def test_values_through_tslot_equal_the_transposed_values(bnn, dev, models):
    """The sweep reads a member's values column by column (stored so by the draw); lbbnn_sparse_gather_members on the CSR-order
    values through ``tslot`` gives the same bits."""
    ev, ops = bnn.evaluate, bnn.ops
    from bnn_amd import _lib
    case = _case("mnf-8-32-2-T2")
    net, fz = models(case)
    B, S = 65, 3
    x = _x(dev, B, 8)
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, S, keep_members=True, keep_weights=True, keep_masks=True)
    ldb = ops.sparse_row_pad(B)
    col_ptr, trow, tslot = (fz._buf(k, 0) for k in ("col_ptr", "trow", "tslot"))
    # G_1 [m, c'][u][b] from the last layer's weights and the masks, then the finish step in the slot form
    w2 = torch.zeros(S, 2, 32, device=dev)
    rows = torch.repeat_interleave(torch.arange(2, device=dev), (fz.csr(1)[0][1:] - fz.csr(1)[0][:-1]).long())
    w2[:, rows, fz.csr(1)[1].long()] = res["weights"][1]
    g = torch.zeros(S * 2, 32, ldb, device=dev)
    g[:, :, :B] = (w2[:, :, :, None] * res["masks"][0].transpose(1, 2)[:, None, :, :]).reshape(S * 2, 32, B)
    xT = torch.zeros(8, ldb, device=dev)
    xT[:, :B] = x.T
    out = torch.full((S * 2, 8 * ldb), float("nan"), device=dev)
    ops.sparse_gather_members(_lib.GATHER_FINISH, col_ptr, trow, tslot, res["weights"][0].contiguous(), g, out, B=B, K=32, N=8,
                              lda=ldb, a_mstride=32 * ldb, ldo=ldb, o_mstride=8 * ldb, blocks=S * 2, per_member=2, h=xT, ldh=ldb)
    got = out.view(S, 2, 8, ldb)[:, :, :, :B].permute(0, 3, 1, 2)
    assert torch.equal(got, res["members"])


def test_a_feature_without_a_kept_path_in_a_deep_network(bnn, dev):
    """Features 5 and 9 of a 20-16-12-3 network lose every first-layer weight: exactly 0.0 in every member, in every statistic,
    while their neighbours are not."""
    ev = bnn.evaluate
    torch.manual_seed(11)
    net = bnn.mnf.BayesianNetwork((20, 16, 12, 3), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).eval()
    lams = sr.lambdals((20, 16, 12, 3), 0.5)[0]
    lams[0][:, [5, 9]] = -2.0
    sr.apply(net, lams)
    fz = ev.freeze(net, "mpm", sparse=True)
    assert not bool(torch.isin(fz.csr(0)[1], torch.tensor([5, 9], device=dev, dtype=torch.int32)).any())
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, _x(dev, 65, 20), 3, keep_members=True)
    for k in ("members", "mean", "std", "prob_positive", "prob_negative"):
        assert bool((res[k][..., [5, 9]] == 0).all()), k
    assert bool((res["members"][..., 6] != 0).any()) and bool((res["std"][..., 6] > 0).any())


# --------------------------------------------------------------------------- 5. the distribution
def test_distribution_of_the_members_logits(bnn, dev, models):
    """The members' logits of the 20 -> 1 network are N(mean-only logit, v_b) with v_b = bias_var + sum_k var[k] x^2, the
    variance the local-reparameterisation epilogue uses: the mean within 5 standard errors, the sample variance within 5 of its
    own (v_b sqrt(2 / (S - 1)) for a normal sample)."""
    ev = bnn.evaluate
    net, fz = models(ONE_LAYER)
    B, S = 4, 4096
    x = _x(dev, B, 20)
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, S)
    _, col, mean, var = [t.double().cpu() for t in fz.csr(0)]
    xs = x.double().cpu()[:, col.long()]
    mu_b = xs @ mean + fz._buf("bias_mu", 0).double().cpu()
    v_b = (xs * xs) @ var + fz._buf("bias_var", 0).double().cpu()
    lg = res["logits"][:, :, 0].double().cpu()
    assert bool(((lg.mean(0) - mu_b).abs() <= 5 * torch.sqrt(v_b / S)).all())
    assert bool(((lg.var(0, unbiased=True) - v_b).abs() <= 5 * v_b * (2.0 / (S - 1)) ** 0.5).all())


# --------------------------------------------------------------------------- 6. the bits
BIT_KEYS = ("mean", "std", "prob_positive", "prob_negative", "logits", "intercept", "residual", "members")


@pytest.mark.parametrize("case", [_case("mnf-64-48-40-20-T2"), _case("lrt-32-24-24-24-24-10"), _case("lrt-50-37-29-3")],
                         ids=["mnf-64-48-40-20-T2", "lrt-32-24-24-24-24-10", "lrt-50-37-29-3"])
def test_bits(bnn, dev, models, monkeypatch, case):
    ev = bnn.evaluate
    _, dims, _, _ = case
    net, fz = models(case)
    B, S = 130, 2
    x = _x(dev, B, dims[0])
    t = (torch.arange(B, device=dev) * 3) % dims[-1]          # fixed targets: a slice of the batch explains the same outputs

    def run(xs, s, ts, off=OFF):
        bnn.manual_seed(SEED, off)
        return ev.explain_ensemble(fz, xs, s, targets=ts, keep_members=True)
    a = run(x, S, t)
    # two calls from one state -- the second on NaN-filled buffers: nothing is read that was not written
    monkeypatch.setattr(ev, "_empty", lambda *size, **kw: torch.full(*size, float("nan"), **kw))
    b = run(x, S, t)
    monkeypatch.undo()
    for k in BIT_KEYS:
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k
    # member m of an S-member call is member 0 of a 1-member call at offset + m
    for m in range(S):
        one = run(x, 1, t, OFF + m)
        for k in ("logits", "intercept", "residual", "members"):
            assert torch.equal(one[k][0], a[k][m]), (k, m)
    # a 64-row slice (the one-row kernel form) equals those rows of the whole batch (the two-row form)
    for lo in (0, 64):
        part = run(x[lo:lo + 64], S, t[lo:lo + 64])
        for k in ("mean", "std", "prob_positive", "prob_negative"):
            assert torch.equal(part[k], a[k][lo:lo + 64]), (k, lo)
        for k in ("logits", "intercept", "residual", "members"):
            assert torch.equal(part[k], a[k][:, lo:lo + 64]), (k, lo)


def test_levels_and_every_output(bnn, dev, models):
    """``levels``: torch.quantile over the members; the bounds bracket the members' median and lie inside their range."""
    ev = bnn.evaluate
    case = _case("mnf-8-32-2-T2")
    net, fz = models(case)
    x = _x(dev, 5, 8)
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, x, 16, levels=(0.5, 0.9))
    mem = res["members"]
    assert len(res["lower"]) == len(res["upper"]) == 2
    for lvl, lo, hi in zip((0.5, 0.9), res["lower"], res["upper"]):
        assert torch.equal(lo, torch.quantile(mem, (1 - lvl) / 2, dim=0)) and torch.equal(hi, torch.quantile(mem, (1 + lvl) / 2, dim=0))
        assert bool((lo <= hi).all()) and bool((lo >= mem.min(0).values).all()) and bool((hi <= mem.max(0).values).all())
    assert bool((res["lower"][1] <= res["lower"][0]).all()) and bool((res["upper"][1] >= res["upper"][0]).all())


# --------------------------------------------------------------------------- 7. the refusals
def test_refusals(bnn, dev, models):
    ev = bnn.evaluate
    net, fz = models(_case("lrt-64-48-40-20"))
    x = _x(dev, 4, 64)
    off = _offset(bnn, dev)
    with pytest.raises(TypeError, match=r"sparse=True.*evaluate\.explain\("):
        ev.explain_ensemble(ev.freeze(net, "mpm"), x)
    with pytest.raises(TypeError, match="not the network itself"):
        ev.explain_ensemble(net, x)
    with pytest.raises(ValueError, match="no CPU path"):
        ev.explain_ensemble(fz, x.cpu())
    with pytest.raises(ValueError, match="samples >= 1"):
        ev.explain_ensemble(fz, x, 0, targets="pred")
    with pytest.raises(ValueError, match="at most 16 outputs"):
        ev.explain_ensemble(fz, x, 2)
    with pytest.raises(ValueError, match="65535"):
        ev.explain_ensemble(fz, x, 65536, targets="pred")
    small_net, small = models(_case("lrt-50-37-29-3"))
    with pytest.raises(ValueError, match="65535"):
        ev.explain_ensemble(small, _x(dev, 4, 50), 21846)     # x 3 outputs
    need = ev.explain_ensemble_work_bytes(fz.dims, 4, 3, 1)
    with pytest.raises(ValueError, match=r"needs %d bytes.*split the batch or lower samples" % need):
        ev.explain_ensemble(fz, x, 3, targets="pred", max_bytes=need - 1)
    with pytest.raises(IndexError, match=r"outside \[0, 20\)"):
        ev.explain_ensemble(fz, x, 3, targets=torch.tensor([0, 1, 20, 2], device=dev))
    with pytest.raises(IndexError):
        ev.explain_ensemble(fz, x, 3, targets=torch.tensor([0, -1, 3, 2], device=dev))
    with pytest.raises(ValueError, match="int64"):
        ev.explain_ensemble(fz, x, 3, targets=torch.tensor([0, 1, 2], device=dev))
    with pytest.raises(ValueError, match="ONE member"):
        ev.explain_ensemble(fz, x, 2, targets="pred", weight_noise=False)
    with pytest.raises(ValueError, match="levels"):
        ev.explain_ensemble(fz, x, 2, targets="pred", levels=(1.5,))
    assert _offset(bnn, dev) == off                           # a refused call draws nothing
    # explain keeps refusing the sparse model
    with pytest.raises(ValueError, match="not built for sparse=True"):
        ev.explain(fz, x)
    # ... and the call at exactly max_bytes goes through
    res = ev.explain_ensemble(fz, x, 3, targets="pred", max_bytes=need)
    assert tuple(res["mean"].shape) == (4, 1, 64)


def test_empty_batch(bnn, dev, models):
    ev = bnn.evaluate
    net, fz = models(_case("mnf-20-16-12-3-T4"))
    bnn.manual_seed(SEED, OFF)
    res = ev.explain_ensemble(fz, torch.zeros(0, 20, device=dev), 3, keep_members=True)
    assert _offset(bnn, dev) == OFF + 3
    assert tuple(res["mean"].shape) == (0, 3, 20) and tuple(res["logits"].shape) == (3, 0, 3)
    assert tuple(res["members"].shape) == (3, 0, 3, 20) and tuple(res["z"][0].shape) == (3, 20)
