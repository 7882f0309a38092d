"""GPU tier of evaluate.explain (include/lbbnn.h: lbbnn_explain_step, lbbnn_explain_totals, lbbnn_explain_operand) against the
numpy float64 restatement (tests/explain_ref.py) under the DEVICE's masks, on the frozen snapshot's own operands.

Every error below is normalised by max|contributions| of its case.  The parity bars are four times the worst error of the
first run on an MI355X, rounded up to one digit (profiles/explain.txt); for fp32 they sit below the ceiling the arithmetic
allows -- chains of at most five products of at most 32 terms at unit round-off 6e-8: about 1e-6, and never above 1e-5."""
import copy

import numpy as np
import pytest
import torch

import explain_ref as er

pytestmark = pytest.mark.gpu

FP32_CEILING = 1e-5
# (case, precision) -> the bar of contributions, intercept, logits and residual; measured x 4, one digit, see above
BARS = {
    ("20-1", "fp32"): 9e-7,             # measured 2.02e-7
    ("12-24-8-3", "fp32"): 1e-6,        # 2.31e-7 (the worst of the mpm, alpha, dead-feature and compact models)
    ("8-32-2", "fp32"): 9e-7,           # 2.03e-7
    ("13-9-5-2", "fp32"): 2e-6,         # 4.48e-7
    ("12-24-3-mnf", "fp32"): 5e-7,      # 1.00e-7 (full and compact)
    ("8-16x4-4", "fp32"): 2e-6,         # 3.74e-7
    ("12-24-8-3", "bf16x3"): 7e-7,      # 1.58e-7: no layer of these widths takes the hi | lo format, the numbers are fp32's
    # 9.79e-6, all of it the FORWARD's: x and the hidden activations enter its products as bf16 hi + lo (16 bits); the sweep
    # is fp32 on hi + lo of the operands, and contributions and intercept stay at 7e-8
    ("16-24-40-3", "bf16x3"): 4e-5,
}
# the sweep alone (contributions, intercept) where the forward is 16-bit: it is fp32 there too; measured 6.93e-8 x 4
SWEEP_BARS = {("16-24-40-3", "bf16x3"): 3e-7}
DEAD = (1, 3, 4, 8, 10)      # features cut off every path in the exact-zero networks (12 inputs: 7 stay needed)
FP32 = [k for k in er.CASES if k != "16-24-40-3"]
ALL = [(k, "fp32") for k in FP32] + [("12-24-8-3", "bf16x3"), ("16-24-40-3", "bf16x3")]
IDS = ["%s-%s" % c for c in ALL]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _np(t):
    return t.detach().cpu().double().numpy()


class Run:
    """One case: the frozen model, one explain call from a fixed Philox state, and the fp64 reference under its masks."""

    def __init__(self, bnn, dev, name, precision="fp32", gates="mpm", compact=False, dead=False):
        net, x = er.build_net(bnn, name)
        if dead:
            with torch.no_grad():
                net._layers()[0].lambdal[:, list(DEAD)] = -9.0
        net = net.to(dev).eval()
        if precision != "fp32":
            net.set_precision(precision)
        self.name, self.family = name, er.CASES[name][2]
        self.fz = bnn.evaluate.freeze(net, gates, compact=compact)
        self.x = x.to(dev)
        self.res = self.call(bnn, keep_masks=True)
        self.Ws, self.bs = er.snapshot_operands(self.fz, self.res.get("z"))
        xin = self.x[:, self.fz.live[0].long()] if compact else self.x
        self.xin = _np(xin)
        self.ref = er.explain_ref(self.Ws, self.bs, self.xin, [m.cpu().numpy() for m in self.res["masks"]])
        self.scale = float(np.abs(self.ref["contributions"]).max())

    def call(self, bnn, **kw):
        bnn.manual_seed(7, 3)                                 # the same Philox state for every call of a case
        return bnn.evaluate.explain(self.fz, self.x, **kw)

    def full(self, contributions):
        """Reference contributions (B, C, compact width) at the network's own feature index."""
        if not self.fz.compact:
            return contributions
        out = np.zeros(contributions.shape[:2] + (self.fz.full_dims[0],))
        out[:, :, self.fz.live[0].cpu().numpy()] = contributions
        return out


@pytest.fixture(scope="module")
def runs(bnn, dev):
    cache = {}

    def get(name, precision="fp32", **kw):
        key = (name, precision, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = Run(bnn, dev, name, precision, **kw)
        return cache[key]
    return get


def _errors(r):
    res, ref = r.res, r.ref
    e = {k: float(np.abs(_np(res[k]) - (r.full(ref[k]) if k == "contributions" else ref[k])).max()) / r.scale
         for k in ("contributions", "intercept", "logits")}
    e["residual"] = float(np.abs(_np(res["residual"])).max()) / r.scale
    return e


# ------------------------------------------------------------------------------------------------ 1. parity, 3. completeness
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_parity_and_completeness(runs, case):
    r = runs(*case)
    dims, B = er.CASES[case[0]][0], er.CASES[case[0]][3]
    C = dims[-1]
    assert r.res["logits"].shape == (B, C) and r.res["contributions"].shape == (B, C, dims[0])
    assert r.res["intercept"].shape == r.res["residual"].shape == (B, C)
    assert r.res["contributions"].dtype == torch.float32 and r.res["active"].dtype == torch.int32
    assert r.res["active"].shape == (B, len(dims) - 2) and r.res["targets"] is None
    e = _errors(r)
    print("explain parity %s %s: " % case + "  ".join("%s %.3e" % kv for kv in sorted(e.items())))
    bar = BARS[case]
    if case[1] == "fp32":
        assert bar <= FP32_CEILING
    if case[0] == "16-24-40-3":
        assert r.fz._split[0] and r.fz._split[1] and not r.fz._split[2]       # the hi | lo operands really are in play
    for k, v in e.items():
        assert v <= bar, (k, v, bar)
    if case in SWEEP_BARS:
        assert max(e["contributions"], e["intercept"]) <= SWEEP_BARS[case], e
    if len(dims) == 2:                                       # one layer: w * x and b, exactly
        w32, x32 = r.Ws[0].astype(np.float32), r.xin.astype(np.float32)       # (exact: they are fp32 values)
        assert np.array_equal(r.res["contributions"].cpu().numpy(), w32[None, :, :] * x32[:, None, :])
        assert np.array_equal(_np(r.res["intercept"]), np.broadcast_to(r.bs[0][None, :], (B, C)))


def test_gates_alpha(runs):
    r = runs("12-24-8-3", gates="alpha")
    e = _errors(r)
    print("explain parity 12-24-8-3 alpha: " + "  ".join("%s %.3e" % kv for kv in sorted(e.items())))
    assert max(e.values()) <= BARS[("12-24-8-3", "fp32")]


# ------------------------------------------------------------------------------------------------ 2. masks
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_masks_are_the_forwards_own(runs, case):
    r = runs(*case)
    masks = r.res["masks"]
    n = len(r.Ws)
    assert len(masks) == n - 1
    if n == 1:
        assert r.res["active"].shape[1] == 0
        return
    _, pre = er.relu_masks(r.Ws, r.bs, r.xin)
    left_out = total = 0
    for l, (m, a) in enumerate(zip(masks, pre)):
        assert m.dtype == torch.bool and tuple(m.shape) == a.shape
        decided = np.abs(a) >= er.NEAR_ZERO * np.abs(a).max()
        left_out += int((~decided).sum())
        total += a.size
        assert np.array_equal(m.cpu().numpy()[decided], (a > 0)[decided]), l
        assert torch.equal(r.res["active"][:, l], m.sum(1).to(torch.int32)), l
    assert left_out <= er.NEAR_ZERO_CAP * total, (left_out, total)


# ------------------------------------------------------------------------------------------------ 4. exact zeros
@pytest.mark.parametrize("name", ["12-24-8-3", "12-24-3-mnf"])
def test_exact_zeros_and_the_compact_model(bnn, runs, name):
    full, comp = runs(name, dead=True), runs(name, dead=True, compact=True)
    need, _ = bnn.evaluate.live_structure([l.lambdal.detach() > 0 for l in full.fz._src[0]._layers()])
    needed = need[0].cpu().numpy()
    assert not needed[list(DEAD)].any() and needed.sum() == 12 - len(DEAD)
    assert comp.fz.compact and not comp.fz._input_identity and comp.fz.dims[0] == 8    # the scatter path is in play
    cf, cc = _np(full.res["contributions"]), _np(comp.res["contributions"])
    assert (cf[:, :, ~needed] == 0.0).all() and (cc[:, :, ~needed] == 0.0).all()
    assert (cf[:, :, needed] != 0.0).any()
    bar = BARS[(name, "fp32")]
    for r in (full, comp):
        e = _errors(r)
        print("explain parity %s dead features, compact=%s: " % (name, r.fz.compact) + "  ".join("%s %.3e" % kv for kv in sorted(e.items())))
        assert max(e.values()) <= bar, e
    assert np.abs(cf - cc).max() <= bar * full.scale
    assert np.abs(_np(full.res["intercept"]) - _np(comp.res["intercept"])).max() <= bar * full.scale
    if full.family == "mnf":                                  # the same Philox state: the same z, bit for bit
        for zf, zc in zip(full.res["z"], comp.res["z"]):
            assert torch.equal(zf, zc)


# ------------------------------------------------------------------------------------------------ 5. forward identity
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_logits_are_the_forwards_pre_head_output(bnn, dev, runs, case):
    r = runs(*case)
    fz = r.fz
    raw = copy.deepcopy(fz)
    raw.head = "identity"                                     # the same chain, returned before the head
    st = bnn.ops.RngState.get(dev)
    bnn.manual_seed(7, 3)
    assert torch.equal(raw(r.x, sample=False), r.res["logits"])
    bnn.manual_seed(7, 3)
    out = fz(r.x, sample=False)
    if fz.head == "identity":
        assert torch.equal(out, r.res["logits"])
    elif fz.head == "sigmoid":
        assert torch.equal(out, bnn.ops.binary_head(r.res["logits"].clone()))
    else:
        assert torch.allclose(out, torch.log_softmax(r.res["logits"], 1), rtol=1e-5, atol=1e-6)
    bnn.manual_seed(7, 3)
    before = int(st.t[1])
    bnn.evaluate.explain(fz, r.x)
    assert int(st.t[1]) - before == (1 if r.family == "mnf" else 0)
    if r.family == "mnf":
        assert len(r.res["z"]) == fz.n_layers and all(z.shape == (d,) for z, d in zip(r.res["z"], fz.full_dims))
    else:
        assert "z" not in r.res


# ------------------------------------------------------------------------------------------------ 6. targets
@pytest.mark.parametrize("name", ["12-24-8-3", "8-32-2", "12-24-3-mnf", "20-1"])
def test_targets(bnn, runs, name):
    r = runs(name)
    bar, B = BARS[(name, "fp32")] * r.scale, r.x.shape[0]
    C = r.fz.dims[-1]
    pred = torch.argmax(r.res["logits"], 1)
    idx = pred[:, None, None].expand(B, 1, r.fz.full_dims[0])
    for t in ("pred", pred):
        one = r.call(bnn, targets=t)
        assert one["contributions"].shape == (B, 1, r.fz.full_dims[0]) and one["intercept"].shape == one["residual"].shape == (B, 1)
        assert torch.equal(one["targets"], pred) and torch.equal(one["logits"], r.res["logits"])
        assert float((one["contributions"] - r.res["contributions"].gather(1, idx)).abs().max()) <= bar
        assert float((one["intercept"] - r.res["intercept"].gather(1, pred[:, None])).abs().max()) <= bar
        assert float(one["residual"].abs().max()) <= bar
    for bad in (C, -1):
        t = pred.clone()
        t[B // 2] = bad
        with pytest.raises(IndexError):
            r.call(bnn, targets=t)
    with pytest.raises(ValueError):
        r.call(bnn, targets=pred[:-1])
    with pytest.raises(ValueError):
        r.call(bnn, targets=pred.cpu())


def test_more_than_16_outputs_need_targets(bnn, dev):
    torch.manual_seed(0)
    net = bnn.lrt.BayesianNetwork((8, 12, 20)).to(dev).eval()
    fz = bnn.evaluate.freeze(net, "mpm")
    x = torch.randn(6, 8, device=dev)
    with pytest.raises(ValueError, match="targets="):
        bnn.evaluate.explain(fz, x)
    res = bnn.evaluate.explain(fz, x, targets="pred", keep_masks=True)
    Ws, bs = er.snapshot_operands(fz)
    ref = er.explain_ref(Ws, bs, _np(x), [m.cpu().numpy() for m in res["masks"]])
    t = res["targets"].cpu().numpy()
    scale = np.abs(ref["contributions"]).max()
    assert np.abs(_np(res["contributions"])[:, 0] - ref["contributions"][np.arange(6), t]).max() <= FP32_CEILING * scale
    assert np.abs(_np(res["residual"])).max() <= FP32_CEILING * scale


# ------------------------------------------------------------------------------------------------ 7. determinism
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_two_calls_give_the_same_bits(bnn, runs, case):
    r = runs(*case)
    again = r.call(bnn, keep_masks=True)
    for k in ("logits", "contributions", "intercept", "residual", "active"):
        assert torch.equal(again[k], r.res[k]), k
    for a, b in zip(again["masks"], r.res["masks"]):
        assert torch.equal(a, b)
    for a, b in zip(again.get("z", []), r.res.get("z", [])):
        assert torch.equal(a, b)
    plain = r.call(bnn)
    assert "masks" not in plain and torch.equal(plain["active"], r.res["active"]) and torch.equal(plain["intercept"], r.res["intercept"])


# ------------------------------------------------------------------------------------------------ 8. the accumulator
@pytest.mark.parametrize("mode", ["all", "pred"])
def test_accumulator(bnn, dev, runs, mode):
    ev = bnn.evaluate
    r = runs("12-24-8-3")
    fz, C, F = r.fz, 3, 12
    g = torch.Generator().manual_seed(5)
    batches = [torch.randn(b, F, generator=g).to(dev) for b in (5, 64, 1)]
    tg = None if mode == "all" else "pred"
    acc = ev.ExplanationAccumulator(C, F, dev)
    total, abs_total, rows = np.zeros((C, F)), np.zeros((C, F)), np.zeros(C, dtype=np.int64)
    for x in batches:
        res = ev.explain(fz, x, targets=tg, acc=acc)
        c = _np(res["contributions"])
        for cls in range(C):
            sel = c[:, cls] if mode == "all" else c[res["targets"].cpu().numpy() == cls, 0]
            total[cls] += sel.sum(0)
            abs_total[cls] += np.abs(sel).sum(0)
            rows[cls] += sel.shape[0]
    out = acc.result()
    assert acc.updates == 3 and np.array_equal(out["rows"], rows) and rows.sum() == 70 * (C if mode == "all" else 1)
    tol = 1e-12 * np.abs(abs_total).max()
    assert np.abs(out["sum_contribution"] - total).max() <= tol and np.abs(out["sum_abs_contribution"] - abs_total).max() <= tol
    den = np.where(rows > 0, rows, 1)[:, None]
    ok = rows > 0
    assert np.abs(out["mean_abs_contribution"][ok] - (abs_total / den)[ok]).max() <= tol
    assert np.abs(out["mean_contribution"][ok] - (total / den)[ok]).max() <= tol
    # the pass form, and a second run: the same bits
    first = ev.explain_batches(fz, batches, targets=mode).result()
    second = ev.explain_batches(fz, [(x, None) for x in batches], targets=mode).result()
    for k in ("rows", "sum_contribution", "sum_abs_contribution"):
        assert np.array_equal(first[k], out[k]) and np.array_equal(second[k], out[k]), k
    acc.reset()
    z = acc.result()
    assert acc.updates == 0 and not z["rows"].any() and not z["sum_contribution"].any() and not z["sum_abs_contribution"].any()
    # one batch of more rows than one block of the totals holds
    big = torch.randn(200, F, generator=g).to(dev)
    res = ev.explain(fz, big, targets=tg, acc=acc)
    c = _np(res["contributions"])
    want = np.stack([np.abs(c[:, cls] if mode == "all" else c[res["targets"].cpu().numpy() == cls, 0]).sum(0) for cls in range(C)])
    assert np.abs(acc.result()["sum_abs_contribution"] - want).max() <= 1e-12 * want.max()


@pytest.mark.parametrize("mode", ["all", "pred"])
def test_accumulator_past_256_row_blocks(bnn, dev, runs, mode):
    """64 * 256 + 1 rows: the totals then take 65 rows per block (253 blocks) instead of 64, and the last block is short."""
    ev = bnn.evaluate
    fz, B = runs("12-24-8-3").fz, 64 * 256 + 1
    x = torch.randn(B, 12, generator=torch.Generator().manual_seed(9)).to(dev)
    acc = ev.ExplanationAccumulator(3, 12, dev)
    res = ev.explain(fz, x, targets=None if mode == "all" else "pred", acc=acc)
    assert float(res["residual"].abs().max()) <= BARS[("12-24-8-3", "fp32")] * float(res["contributions"].abs().max())
    c = res["contributions"].double()
    out = acc.result()
    for cls in range(3):
        sel = c[:, cls] if mode == "all" else c[res["targets"] == cls, 0]
        assert out["rows"][cls] == sel.shape[0]
        want, want_abs = sel.sum(0).cpu().numpy(), sel.abs().sum(0).cpu().numpy()
        assert np.abs(out["sum_contribution"][cls] - want).max() <= 1e-12 * want_abs.max()
        assert np.abs(out["sum_abs_contribution"][cls] - want_abs).max() <= 1e-12 * want_abs.max()
    assert out["rows"].sum() == B * (3 if mode == "all" else 1)


@pytest.mark.parametrize("name", ["12-24-8-3", "12-24-3-mnf"])
def test_empty_batch(bnn, dev, runs, name):
    r = runs(name)
    st = bnn.ops.RngState.get(dev)
    bnn.manual_seed(7, 3)
    acc = bnn.evaluate.ExplanationAccumulator(3, 12, dev)
    res = bnn.evaluate.explain(r.fz, r.x[:0], keep_masks=True, acc=acc)
    assert int(st.t[1]) - 3 == (1 if r.family == "mnf" else 0)
    assert res["logits"].shape == (0, 3) and res["contributions"].shape == (0, 3, 12) and res["active"].shape == (0, len(r.Ws) - 1)
    assert res["intercept"].shape == res["residual"].shape == (0, 3) and [m.shape for m in res["masks"]] == [(0, 24)] * (len(r.Ws) - 2) + [(0, r.fz.dims[-2])]
    assert bnn.evaluate.explain(r.fz, r.x[:0], targets="pred")["contributions"].shape == (0, 1, 12)
    assert acc.updates == 1 and not acc.result()["rows"].any()
    if r.family == "mnf":
        assert all(torch.equal(a, b) for a, b in zip(res["z"], r.res["z"]))      # the draw an explained batch makes


def test_refresh_drops_the_cached_operands(bnn, dev):
    net, x = er.build_net(bnn, "12-24-8-3")
    net = net.to(dev).eval()
    fz = bnn.evaluate.freeze(net, "mpm")
    x = x.to(dev)
    a = bnn.evaluate.explain(fz, x)
    assert fz._xops is not None
    with torch.no_grad():
        net._layers()[0].weight_mu.mul_(2.0)
    fz.refresh()
    assert fz._xops is None
    b = bnn.evaluate.explain(fz, x, keep_masks=True)
    Ws, bs = er.snapshot_operands(fz)
    ref = er.explain_ref(Ws, bs, _np(x), [m.cpu().numpy() for m in b["masks"]])
    scale = np.abs(ref["contributions"]).max()
    assert np.abs(_np(b["contributions"]) - ref["contributions"]).max() <= BARS[("12-24-8-3", "fp32")] * scale
    assert not torch.equal(a["contributions"], b["contributions"])
