"""GPU tier of the uncertainty metrics (include/lbbnn.h lbbnn_eval_uncertainty; evaluate.ensemble_uncertainty /
UncertaintyAccumulator / ood_auroc / evaluate_batches; graphs.make_graphed_eval_step) against tests/eval_uncertainty_ref.py.

EXACT, no row left out, derived from the kernel's own returned per-row values: ``confidence == bma_probs.max(1)`` bit for bit,
``pred_bma`` = numpy's argmax of the returned ``bma_probs``, ``mutual_information == max(0, total - expected)`` in fp32, and
every count, reliability bin and histogram = the restatement's binning of the returned fp32 values -- over S in {1, 2, 3, 4, 5,
10, 17} x B in {0, 1, 15, 16, 17, 63, 64, 65, 100, 257} x C in {1, 2, 3, 10, 16, 17, 33, 64} (the member loop loads 4 members at
a time and has no other chunking; S = 100 at B = 3, C = 10 is 25 such groups), inputs of scale 1, 3 and 20.

DOUBLE SUMS (the six sums and the per-bin confidence sums): against the float64 sum of the returned per-row values within
DBL * sum|term|, DBL = 1e-12: the terms are exact fp32 values, so only the error of adding n <= 257 doubles in another order
remains (<= n * 2^-53 * sum|term| = 2.9e-14 * sum|term|).

PER-ROW VALUES against float64 from the inputs (``rows64``), absolute, the three entropies divided by ln C: the bar per
quantity is FACTOR = 4 x the largest error of the same expression written in torch fp32 on the same device and inputs
(``_torch_rows``), with a floor of 8 * 2^-24 = 4.8e-7 for a torch error of zero.  Both are fp32 exp / log chains with different
device intrinsics and summation orders; a wrong formula shows at 1e-2 or more.  Both errors are measured and printed on every
run (test_per_row_values_within_four_times_the_torch_error); profiles/eval_uncertainty.txt keeps a run's table.
"""
import math

import numpy as np
import pytest
import torch

import eval_uncertainty_ref as ref

pytestmark = pytest.mark.gpu

SS = (1, 2, 3, 4, 5, 10, 17)
BS = (0, 1, 15, 16, 17, 63, 64, 65, 100, 257)
CS = (1, 2, 3, 10, 16, 17, 33, 64)
LONG = (100, 3, 10)
DBL = 1e-12
FACTOR = 4.0
FLOOR = 8 * 2.0 ** -24
M, K = 20, 1024
QUANTITIES = ("total_entropy", "expected_entropy", "mutual_information", "confidence", "brier", "log_score")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _logp(S, B, C, seed, scale=None):
    g = torch.Generator().manual_seed(seed)
    scale = (1.0, 3.0, 20.0)[seed % 3] if scale is None else scale
    return torch.log_softmax(scale * torch.randn(S, B, C, generator=g), -1)


def _targets(B, C, seed):
    return torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed))


def _np(t):
    return t.detach().cpu().numpy()


def _same_f32(a, b):
    """Bit for bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))


def _close_sum(got, terms, what):
    terms = np.asarray(terms, dtype=np.float64)
    want = float(terms.sum()) if terms.size else 0.0
    assert np.isfinite(want) and abs(got - want) <= DBL * float(np.abs(terms).sum()), (what, got, want, abs(got - want))


def _run(bnn, dev, o, t=None, conf_bins=M, hist_bins=K):
    """One update of a fresh accumulator: (per-row numpy dict, result with strict=False, the accumulator)."""
    S, B, C = o.shape
    u = bnn.evaluate.UncertaintyAccumulator(C, S, dev, conf_bins=conf_bins, hist_bins=hist_bins)
    rows = u.update(o.to(dev) if o.device != dev else o, None if t is None else t.to(dev))
    return {k: _np(v) for k, v in rows.items()}, u.result(strict=False), u


def _check_exact(rows, tot, t, C, what, conf_bins=M, hist_bins=K, parts=None):
    """Everything that must be exact given the kernel's own per-row values, and the double sums.  ``parts``: the restatement's
    totals when ``tot`` accumulated several calls (default: one call, from ``rows``)."""
    B = rows["confidence"].shape[0]
    if B:
        with np.errstate(all="ignore"):
            assert _same_f32(rows["confidence"], rows["bma_probs"].max(1)), what
    else:
        assert rows["bma_probs"].shape == (0, C)
    assert np.array_equal(rows["pred_bma"], ref.argmax_rows(rows["bma_probs"])), what
    want_mi = ref.mutual_information(rows["total_entropy"], rows["expected_entropy"])
    got_mi = rows["mutual_information"]
    assert np.array_equal(np.isnan(got_mi), np.isnan(want_mi)) and np.array_equal(got_mi[~np.isnan(got_mi)], want_mi[~np.isnan(want_mi)]), what
    r = parts if parts is not None else ref.totals(rows, None if t is None else _np(t), C, conf_bins, hist_bins)
    for k in ref.COUNT_NAMES:
        assert tot[k] == r[k], (what, k, tot[k], r[k])
    for k in ("bin_rows", "bin_rows_with_target", "bin_correct"):
        assert np.array_equal(tot[k], r[k]), (what, k)
    for i, k in enumerate(ref.SCORES):
        assert np.array_equal(tot["histograms"][k]["counts"], r["hist"][i]), (what, k)
    finite = tot["rows"] - tot["nonfinite_rows"]
    assert int(tot["bin_rows"].sum()) == finite and [int(h.sum()) for h in r["hist"]] == [finite] * 3, what
    for k in ref.SUM_NAMES:
        _close_sum(tot[k + "_sum"], r["terms"][k], what + " " + k)
    for m in range(conf_bins):
        _close_sum(float(tot["bin_conf_sum"][m]), r["bin_conf_terms"][m], what + " bin_conf_sum[%d]" % m)
    c = ref.calibration(r["bin_rows_with_target"], r["bin_correct"], tot["bin_conf_sum"])
    if int(r["bin_rows_with_target"].sum()):
        assert abs(tot["ece"] - c["ece"]) < 1e-12 and abs(tot["mce"] - c["mce"]) < 1e-12, what
        assert np.allclose(tot["selective"]["coverage"], c["coverage"], equal_nan=True), what
        assert np.allclose(tot["selective"]["accuracy"], c["accuracy"], equal_nan=True), what
    return r


def _torch_rows(o, t):
    """The same per-row numbers as plain torch fp32 expressions on the device (the comparator of the error bar)."""
    S, B, C = o.shape
    p = o.exp()
    pb = p.mean(0)
    zero = torch.zeros((), device=o.device)
    total = -torch.where(pb == 0, zero, pb * pb.log()).sum(-1)
    expected = (-torch.where(p == 0, zero, p * o).sum(-1)).mean(0)
    idx = torch.arange(B, device=o.device)
    return {"total_entropy": total, "expected_entropy": expected, "mutual_information": (total - expected).clamp_min(0.0),
            "confidence": pb.max(-1).values if B else pb.new_zeros(0),
            "brier": ((pb - torch.nn.functional.one_hot(t, C)) ** 2).sum(-1),
            "log_score": -(torch.logsumexp(o[:, idx, t], 0) - math.log(S))}


def _errors(rows, r64, C):
    """max |x - float64| per quantity, the entropies over ln C; the log score wherever the float64 value is finite."""
    out = {}
    for k in QUANTITIES:
        want = np.asarray(r64[k], dtype=np.float64)
        ok = np.isfinite(want)
        d = np.abs(np.asarray(rows[k], dtype=np.float64)[ok] - want[ok])
        assert np.isfinite(d).all(), k
        scale = math.log(max(C, 2)) if k in QUANTITIES[:3] else 1.0
        out[k] = float(d.max() / scale) if d.size else 0.0
    return out


@pytest.fixture(scope="module")
def sweep(bnn, dev):
    """case(S, B, C) -> the kernel's results, and both errors against float64, on the random inputs of that shape (once)."""
    cache = {}

    def case(S, B, C):
        if (S, B, C) not in cache:
            o, t = _logp(S, B, C, 1000 * S + B + C), _targets(B, C, B + C)
            rows, tot, _ = _run(bnn, dev, o, t)
            r64 = ref.rows64(_np(o), _np(t))
            assert all(np.isfinite(r64[k]).all() for k in QUANTITIES), (S, B, C)
            e_torch = _errors({k: _np(v) for k, v in _torch_rows(o.to(dev), t.to(dev)).items()}, r64, C)
            cache[(S, B, C)] = dict(rows=rows, tot=tot, t=t, err_kernel=_errors(rows, r64, C), err_torch=e_torch)
        return cache[(S, B, C)]
    return case


# ----------------------------------------------------------------------------------- 1. random inputs, every shape
@pytest.mark.parametrize("C", CS)
def test_random_inputs_totals_equal_the_binning_of_the_returned_rows(sweep, C):
    for S, B in [(S, B) for S in SS for B in BS] + ([LONG[:2]] if C == LONG[2] else []):
        k = sweep(S, B, C)
        tot = k["tot"]
        assert tot["rows"] == B == tot["rows_with_target"] and tot["bad_targets"] == 0 and tot["nonfinite_rows"] == 0
        assert tot["log_score_nonfinite"] == 0
        _check_exact(k["rows"], tot, k["t"], C, "S=%d B=%d C=%d" % (S, B, C))
        if S == 1:
            assert not k["rows"]["mutual_information"].any(), (B, C)          # one member: exactly 0


def test_per_row_values_within_four_times_the_torch_error(sweep):
    """The bar of the module docstring, per quantity, over the whole sweep."""
    shapes = [(S, B, C) for S in SS for B in BS for C in CS] + [LONG]
    e_t, e_k = dict.fromkeys(QUANTITIES, 0.0), dict.fromkeys(QUANTITIES, 0.0)
    for sh in shapes:
        k = sweep(*sh)
        for q in QUANTITIES:
            e_t[q], e_k[q] = max(e_t[q], k["err_torch"][q]), max(e_k[q], k["err_kernel"][q])
    bars = {q: max(FACTOR * e_t[q], FLOOR) for q in QUANTITIES}
    for q in QUANTITIES:
        print("per-row %-18s against float64%s: torch %.3e, kernel %.3e, bar %.3e"
              % (q, " (/ ln C)" if q in QUANTITIES[:3] else "", e_t[q], e_k[q], bars[q]))
    for q in QUANTITIES:
        assert e_k[q] <= bars[q], (q, e_k[q], e_t[q], bars[q])


def _bar(sweep, q, C):
    """The bar of quantity q as an absolute number for C classes, from the shapes of the sweep with that C."""
    e = max(sweep(S, B, C)["err_torch"][q] for S in SS for B in BS)
    return max(FACTOR * e, FLOOR) * (math.log(max(C, 2)) if q in QUANTITIES[:3] else 1.0)


# ----------------------------------------------------------------------------------- 2. constructed inputs
@pytest.mark.parametrize("C", (3, 10, 17, 64))
@pytest.mark.parametrize("S", (1, 2, 5))
def test_constructed_inputs(bnn, dev, S, C):
    """Exact ties (duplicated class columns), a -inf entry, an all-NaN row, targets -1 and C."""
    B = 65
    z, t = 3.0 * torch.randn(S, B, C, generator=torch.Generator().manual_seed(31 * S + C)), _targets(B, C, C)
    z[..., C - 1] = z[..., 1]
    even = np.arange(B) % 2 == 0
    z[:, torch.from_numpy(even), 1] += 20.0
    z[:, torch.from_numpy(even), C - 1] += 20.0                # the tied maximum on even rows: the lowest index must win
    o = torch.log_softmax(z, -1)
    assert torch.equal(o[..., 1], o[..., C - 1])
    o[S - 1, 3, 0] = float("-inf")
    t[3] = 2
    o[:, 7, :] = float("nan")
    o[0, 9, 2] = float("nan")                                  # one NaN class in one member poisons the row as well
    t[5], t[11] = -1, C
    rows, tot, _ = _run(bnn, dev, o, t)
    what = "S=%d C=%d" % (S, C)
    _check_exact(rows, tot, t, C, what)
    assert (rows["pred_bma"][even & (np.arange(B) > 9)] == 1).all(), what
    for k in QUANTITIES[:4]:
        assert np.isfinite(rows[k][3]), (what, k)              # -inf: a zero term, not a NaN
    r64 = ref.rows64(_np(o), _np(t))
    assert abs(rows["total_entropy"][3] - r64["total_entropy"][3]) < 1e-5 and abs(rows["expected_entropy"][3] - r64["expected_entropy"][3]) < 1e-5
    assert tot["nonfinite_rows"] == 2 and np.isnan(rows["confidence"][7]) and np.isnan(rows["mutual_information"][9])
    assert rows["pred_bma"][7] == 0 and rows["pred_bma"][9] == 2          # a NaN is the maximum
    assert tot["bad_targets"] == 2 and tot["rows_with_target"] == B - 2 and tot["rows"] == B
    assert np.isnan(rows["brier"][5]) and np.isnan(rows["log_score"][11]) and np.isfinite(rows["brier"][4])
    assert int(tot["bin_rows"].sum()) == B - 2 and int(tot["bin_rows_with_target"].sum()) == B - 4
    assert all(np.isfinite(tot[k + "_sum"]) for k in ref.SUM_NAMES), what
    with pytest.raises(IndexError):
        u = bnn.evaluate.UncertaintyAccumulator(C, S, dev)
        u.update(o.to(dev), t.to(dev))
        u.result()
    # without a target: no score, no target-dependent total
    rows0, tot0, _ = _run(bnn, dev, o, None)
    _check_exact(rows0, tot0, None, C, what + " target=None")
    assert np.isnan(rows0["brier"]).all() and np.isnan(rows0["log_score"]).all()
    assert tot0["rows_with_target"] == tot0["bad_targets"] == tot0["correct_bma"] == 0 and tot0["brier_sum"] == 0.0
    assert int(tot0["bin_rows_with_target"].sum()) == 0 and np.isnan(tot0["ece"]) and tot0["rows"] == B
    for k in ("bma_probs", "confidence", "total_entropy", "expected_entropy", "mutual_information"):
        assert _same_f32(rows0[k], rows[k]), (what, k)
    # ensemble_uncertainty alone (no totals: one launch) returns the same rows
    alone = bnn.evaluate.ensemble_uncertainty(o.to(dev), t.to(dev))
    for k in rows:
        assert _same_f32(_np(alone[k]), rows[k]) if rows[k].dtype == np.float32 else np.array_equal(_np(alone[k]), rows[k]), k


def test_log_score_where_the_probability_underflows(bnn, dev):
    """Every member gives the target a log-probability below expf's range: pbar_target is 0, the log score is finite."""
    S, B, C = 4, 16, 10
    o = _logp(S, B, C, 5, scale=1.0)
    t = _targets(B, C, 6)
    o[:, torch.arange(B), t] = -120.0 - torch.arange(S, dtype=torch.float32)[:, None]
    rows, tot, _ = _run(bnn, dev, o, t)
    assert (rows["bma_probs"][np.arange(B), _np(t)] == 0).all()
    want = ref.rows64(_np(o), _np(t))["log_score"]
    assert np.isfinite(rows["log_score"]).all() and np.abs(rows["log_score"] - want).max() < 1e-4 and want.min() > 120
    assert tot["log_score_nonfinite"] == 0
    o[:, 2, t[2]] = float("-inf")                              # no member gives it any probability: +inf, counted, not summed
    rows, tot, _ = _run(bnn, dev, o, t)
    assert rows["log_score"][2] == np.inf and tot["log_score_nonfinite"] == 1 and np.isfinite(tot["log_score_sum"])
    _check_exact(rows, tot, t, C, "underflow")


@pytest.mark.parametrize("C", (2, 10, 33))
def test_mutual_information_of_agreeing_and_disagreeing_members(bnn, dev, sweep, C):
    bar = _bar(sweep, "mutual_information", C)
    one = _logp(1, 100, C, 77, scale=3.0)
    rows, _, _ = _run(bnn, dev, one.expand(5, 100, C).contiguous())
    print("identical members, C=%d: largest MI %.3e, bar %.3e" % (C, rows["mutual_information"].max(), bar))
    assert rows["mutual_information"].max() <= bar and rows["mutual_information"].min() >= 0.0
    for S, classes in ((4, (0, 1, 0, 1)), (3, (0, 1, 2)), (10, (0, C - 1) * 5)):
        if max(classes) >= C:
            continue
        o = torch.full((S, 17, C), float("-inf"))
        for s, k in enumerate(classes):
            o[s, :, k] = 0.0                                   # exactly one-hot members
        rows, tot, _ = _run(bnn, dev, o)
        want = math.log(len(set(classes)))
        assert np.abs(rows["mutual_information"] - want).max() <= bar, (C, S, rows["mutual_information"][0], want)
        assert not rows["expected_entropy"].any() and tot["nonfinite_rows"] == 0
        assert np.allclose(rows["confidence"], classes.count(0) / S)


# ----------------------------------------------------------------------------------- 3. strided views, read in place
def test_strided_views_are_read_in_place(bnn, dev):
    from bnn_amd import _lib
    S, B, C = 10, 100, 10
    o, t = _logp(S, B, C, 3), _targets(B, C, 4)
    rows_c, _, u_c = _run(bnn, dev, o, t)
    nan = float("nan")
    pad_m = torch.full((S, B * C + 12), nan, device=dev)                   # a padded member stride (the head buffer's shape)
    v_m = pad_m[:, :B * C].view(S, B, C)
    v_m.copy_(o)
    pad_r = torch.full((S, B, C + 3), nan, device=dev)                     # padded rows
    v_r = pad_r[:, :, :C]
    v_r.copy_(o)
    for v in (v_m, v_r):
        assert not v.is_contiguous()
        u = bnn.evaluate.UncertaintyAccumulator(C, S, dev)
        _lib.RECORD = calls = []
        try:
            rows = u.update(v, t.to(dev))
        finally:
            _lib.RECORD = None
        (name, _, args), = [c for c in calls if c[0] == "lbbnn_eval_uncertainty"]
        a = args[0]._obj
        assert a.logp == v.data_ptr() and a.m_stride == v.stride(0) and a.ldp == v.stride(1)       # no copy was made
        for k in rows_c:
            got = _np(rows[k])
            assert _same_f32(got, rows_c[k]) if got.dtype == np.float32 else np.array_equal(got, rows_c[k]), k
        assert torch.equal(u._totals, u_c._totals)
    # a layout the kernel does not take is copied, not refused
    rows = bnn.evaluate.ensemble_uncertainty(o.to(dev).permute(0, 2, 1).contiguous().permute(0, 2, 1), t.to(dev))
    assert _same_f32(_np(rows["bma_probs"]), rows_c["bma_probs"]) and _same_f32(_np(rows["log_score"]), rows_c["log_score"])


# ----------------------------------------------------------------------------------- 4. accumulation
def test_updates_accumulate_and_totals_are_bitwise_reproducible(bnn, dev):
    ev = bnn.evaluate
    S, C = 10, 10
    parts = [(_logp(S, B, C, 50 + B), _targets(B, C, 60 + B)) for B in (100, 37, 257)]
    parts[1][1][3] = C                                                     # one bad target on the way
    parts[2][0][:, 5, :] = float("nan")                                    # and one row that is not finite
    on = [tuple(x.to(dev) for x in p) for p in parts]

    def three(u):
        return [{k: _np(v) for k, v in u.update(o, t).items()} for o, t in on]

    a = ev.UncertaintyAccumulator(C, S, dev)
    rows = three(a)
    b = ev.UncertaintyAccumulator(C, S, dev)
    three(b)
    assert torch.equal(a._totals, b._totals)                               # the same bits in the whole totals buffer
    rr = ref.add_totals([ref.totals(r, _np(t), C, M, K) for r, (_, t) in zip(rows, parts)])
    tot = a.result(strict=False)
    _check_exact({k: np.concatenate([r[k] for r in rows]) for k in rows[0]}, tot, None, C, "three updates", parts=rr)
    assert tot["rows"] == 394 and tot["bad_targets"] == 1 and tot["nonfinite_rows"] == 1 and a.updates == 3
    a.reset()
    assert int(a._totals.abs().sum()) == 0 and a.updates == 0 and a.result()["rows"] == 0
    three(a)
    assert torch.equal(a._totals, b._totals)                               # and a reset accumulator starts over exactly
    # other bin counts: the edges of the ranges the C entry point takes
    for conf_bins, hist_bins in ((1, 1), (100, 4096), (7, 33)):
        o, t = parts[0]
        r, tt, _ = _run(bnn, dev, o, t, conf_bins=conf_bins, hist_bins=hist_bins)
        _check_exact(r, tt, t, C, "M=%d K=%d" % (conf_bins, hist_bins), conf_bins=conf_bins, hist_bins=hist_bins)


# ----------------------------------------------------------------------------------- 5. a pass, graphed and eager
DIMS = (20, 16, 16, 10)
SEED = 13


def _frozen(bnn, dev):
    torch.manual_seed(11)
    return bnn.evaluate.freeze(bnn.lrt.BayesianNetwork(DIMS).to(dev).eval())


def _data(dev, n, B, seed, noise=False):
    g = torch.Generator().manual_seed(seed)
    xs = [(5.0 * torch.randn(B, DIMS[0], generator=g) if noise else torch.rand(B, DIMS[0], generator=g)) for _ in range(n)]
    return [(x.to(dev), torch.randint(0, DIMS[-1], (B,), generator=g).to(dev)) for x in xs]


def test_graphed_eval_step_equals_eager_updates_bitwise(bnn, dev):
    ev = bnn.evaluate
    S, C, B = 10, DIMS[-1], 100
    fz = _frozen(bnn, dev)
    data = _data(dev, 3, B, 4)
    mk = lambda: (ev.EvalAccumulator(C, S, dev), ev.UncertaintyAccumulator(C, S, dev))
    acc_g, u_g = mk()
    bnn.manual_seed(SEED)
    o = fz.ensemble(data[0][0], S)
    acc_g.update(o, data[0][1])
    u_g.update(o, data[0][1])                                             # totals that must survive the build
    before, st = (acc_g._totals.clone(), u_g._totals.clone()), bnn.ops.RngState.get(dev)
    rng_before = st.t.clone()
    step = bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], S, acc_g, uncertainty=u_g)
    assert torch.equal(acc_g._totals, before[0]) and torch.equal(u_g._totals, before[1]) and torch.equal(st.t, rng_before)
    assert acc_g.updates == 1 and u_g.updates == 1
    acc_g.reset()
    u_g.reset()
    bnn.manual_seed(SEED)
    got = []
    for x, y in data:
        got.append({k: v.clone() for k, v in step(x, y).items()})
    acc_e, u_e = mk()
    acc_p = ev.EvalAccumulator(C, S, dev)                                  # the pass as it is without the keyword
    bnn.manual_seed(SEED)
    for (x, y), rows_g in zip(data, got):
        o = fz.ensemble(x, S)
        rows_e = acc_e.update(o, y, fz(x, sample=False))
        rows_e.update(u_e.update(o, y))
        assert sorted(rows_e) == sorted(rows_g) and "mutual_information" in rows_g and "pred_posterior_mean" in rows_g
        for k in rows_e:
            assert torch.equal(rows_e[k], rows_g[k]), k
    assert torch.equal(acc_g._totals, acc_e._totals) and torch.equal(u_g._totals, u_e._totals)
    assert acc_g.updates == 3 == u_g.updates and u_g.result()["rows"] == 3 * B
    plain = bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], S, acc_p)
    bnn.manual_seed(SEED)
    for x, y in data:
        assert "mutual_information" not in plain(x, y)
    assert torch.equal(acc_p._totals, acc_g._totals)


def test_evaluate_batches_merges_the_uncertainty_and_ood_auroc_holds_the_pairwise_auroc(bnn, dev):
    ev = bnn.evaluate
    S, C, B = 10, DIMS[-1], 100
    fz = _frozen(bnn, dev)
    results, scores = [], []
    for noise in (False, True):
        data = _data(dev, 2, B, 21 + noise, noise=noise)
        u = ev.UncertaintyAccumulator(C, S, dev, hist_bins=64)
        rec, inner = [], u.update

        def update(o, t, rec=rec, inner=inner):
            rows = inner(o, t)
            rec.append({k: _np(v) for k, v in rows.items()})
            return rows

        u.update = update
        bnn.manual_seed(SEED)
        res = ev.evaluate_batches(fz, data, S, uncertainty=u)
        bnn.manual_seed(SEED)
        alone = ev.evaluate_batches(fz, data, S)
        assert all(np.array_equal(res[k], alone[k]) for k in alone), "the keyword changes none of today's numbers"
        assert "ece" not in alone and res["rows"] == 2 * B == int(res["bin_rows"].sum()) and 0.0 <= res["ece"] <= 1.0
        assert res["correct_bma"] == sum(int((r["pred_bma"] == _np(t)).sum()) for r, (_, t) in zip(rec, data))
        results.append(res)
        scores.append({"total_entropy": np.concatenate([r["total_entropy"] for r in rec]),
                       "mutual_information": np.concatenate([r["mutual_information"] for r in rec]),
                       "max_prob": np.concatenate([np.float32(1) - r["confidence"] for r in rec])})
    for k in ev.OOD_SCORES:
        auroc, hw = ev.ood_auroc(results[0], results[1], k)
        exact = ref.auroc_pairs(scores[0][k], scores[1][k])
        print("ood_auroc %-18s %.4f +- %.4f, pairwise %.4f" % (k, auroc, hw, exact))
        assert auroc - hw - 1e-12 <= exact <= auroc + hw + 1e-12, (k, auroc, hw, exact)
