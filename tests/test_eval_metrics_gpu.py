"""GPU tier of the evaluation metrics (include/lbbnn.h lbbnn_eval_metrics; evaluate.ensemble_metrics / EvalAccumulator /
evaluate_batches; graphs.make_graphed_eval_step) against the numpy restatement tests/eval_metrics_ref.py.

EXACT, no tolerance, no row left out: ``mean_log_probs`` (bit for bit: the header fixes the fp32 order), ``pred_ensemble``,
``pred_posterior_mean``, every integer total, ``correct_member`` and the confusion matrix -- on random log-softmax inputs over
S in {1, 2, 10, 100} x B in {0, 1, 63, 64, 65, 100, 1000, 4096} x C in {1, 2, 10, 16, 17, 64}, on constructed inputs (exact ties
from duplicated class columns, NaN rows, -inf entries, targets -1 and C) and on strided (S,B,C) views read in place.

DOUBLE SUMS: ``nll_sum`` against the float64 sum of the exact ``mean_log_probs`` entries and ``entropy_sum`` against the float64
sum of the returned finite per-row entropies, both within DBL * sum|term| with DBL = 1e-12: the terms are exact fp32 values, so
only the error of adding n <= 4096 doubles in another order remains (<= n * 2^-53 * sum|term| = 4.6e-13 * sum|term|).

PER-ROW ENTROPY against the float64 restatement: the bar is 4 x the largest error of the existing torch expression
``evaluate.predictive_entropy`` against float64 over the same inputs (both are fp32 exp / log / divide chains with different
device intrinsics; a wrong formula shows at 1e-2 or more).  Measured on an MI355X over the 192 random shapes above:
torch 7.21e-07, the kernel 8.97e-07 (absolute, entropies up to log 64 = 4.16), so the bar stood at 2.88e-06
(profiles/eval_metrics.txt).  The test measures both again on every run and prints them.
"""
import numpy as np
import pytest
import torch

import eval_metrics_ref as ref

pytestmark = pytest.mark.gpu

SS = (1, 2, 10, 100)
BS = (0, 1, 63, 64, 65, 100, 1000, 4096)
CS = (1, 2, 10, 16, 17, 64)
DBL = 1e-12
ENTROPY_FACTOR = 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _logp(S, B, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(3.0 * torch.randn(S, B, C, generator=g), -1)


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
    """|got - sum(terms)| <= DBL * sum|terms|; a sum that is not finite must come out as the same inf / NaN."""
    terms = np.asarray(terms, dtype=np.float64)
    with np.errstate(all="ignore"):
        want = float(terms.sum()) if terms.size else 0.0
    if not np.isfinite(want):
        assert (np.isnan(want) and np.isnan(got)) or want == got, (what, got, want)
        return
    assert abs(got - want) <= DBL * float(np.abs(terms).sum()), (what, got, want, abs(got - want))


def _run(bnn, dev, o, t=None, mo=None):
    """One update of a fresh accumulator: (per-row numpy dict, totals with strict=False, the raw totals buffer)."""
    S, B, C = o.shape
    acc = bnn.evaluate.EvalAccumulator(C, S, dev)
    rows = acc.update(o.to(dev), None if t is None else t.to(dev), None if mo is None else mo.to(dev))
    tot = acc.result(strict=False)
    return {k: _np(v) for k, v in rows.items()}, tot, acc._totals.clone()


def _compare(rows, tot, r, what):
    """Everything that must be exact, and the two double sums."""
    assert _same_f32(rows["mean_log_probs"], r["mean_log_probs"]), what
    assert np.array_equal(rows["pred_ensemble"], r["pred_ensemble"]), what
    if "pred_posterior_mean" in r:
        assert np.array_equal(rows["pred_posterior_mean"], r["pred_posterior_mean"]), what
    for k in ref.COUNT_NAMES:
        assert tot[k] == r[k], (what, k, tot[k], r[k])
    assert np.array_equal(tot["correct_member"], r["correct_member"]), what
    assert np.array_equal(tot["confusion"], r["confusion"]), what
    assert int(tot["confusion"].sum()) == r["rows_with_target"], what
    _close_sum(tot["nll_sum"], r["nll_terms"], what + " nll_sum")
    e = rows["entropy"].astype(np.float64)
    assert int((~np.isfinite(e)).sum()) == tot["entropy_nonfinite"], what
    _close_sum(tot["entropy_sum"], e[np.isfinite(e)], what + " entropy_sum")


@pytest.fixture(scope="module")
def sweep(bnn, dev):
    """case(S, B, C) -> the kernel's and the restatement's results on the random inputs of that shape (computed once)."""
    cache = {}

    def case(S, B, C):
        if (S, B, C) not in cache:
            o, t, mo = _logp(S, B, C, 1000 * S + B + C), _targets(B, C, B + C), _logp(1, B, C, 7 * B + C)[0]
            rows, tot, _ = _run(bnn, dev, o, t, mo)
            r = ref.metrics(_np(o), _np(t), _np(mo))
            e_torch = _np(bnn.evaluate.predictive_entropy(o.to(dev))).astype(np.float64)
            e64 = r["entropy"]
            err = lambda e: float(np.abs(e.astype(np.float64) - e64).max()) if B else 0.0
            cache[(S, B, C)] = dict(rows=rows, tot=tot, ref=r, err_torch=err(e_torch), err_kernel=err(rows["entropy"]),
                                    finite=bool(np.isfinite(e64).all()))
        return cache[(S, B, C)]
    return case


# ----------------------------------------------------------------------------------- 1. random inputs, every shape
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("S", SS)
def test_random_inputs_equal_the_restatement_exactly(sweep, S, C):
    for B in BS:
        k = sweep(S, B, C)
        assert k["tot"]["rows"] == B and k["tot"]["bad_targets"] == 0 and k["tot"]["rows_with_target"] == B
        _compare(k["rows"], k["tot"], k["ref"], "S=%d B=%d C=%d" % (S, B, C))


def test_per_row_entropy_within_four_times_the_torch_error(sweep):
    """The bar of the module docstring: 4 x the error of evaluate.predictive_entropy against float64 on the same inputs."""
    e_torch = e_kernel = 0.0
    for S in SS:
        for B in BS:
            for C in CS:
                k = sweep(S, B, C)
                assert k["finite"], (S, B, C)
                e_torch, e_kernel = max(e_torch, k["err_torch"]), max(e_kernel, k["err_kernel"])
    bar = ENTROPY_FACTOR * e_torch
    print("per-row entropy against float64: torch %.3e, kernel %.3e, bar %.3e" % (e_torch, e_kernel, bar))
    assert e_torch > 0.0
    assert e_kernel <= bar, (e_kernel, e_torch, bar)


# ----------------------------------------------------------------------------------- 2. constructed inputs
def _constructed(S, B, C, variant):
    """Duplicated class columns (the tied maximum on even rows: the lowest index must win), -inf entries, targets -1 and C;
    variant 1 adds a row that is NaN in one member, a single NaN class and a row of -inf in every member; variant 2 the same with
    the NaN row's target out of range (so that nll_sum is +inf, not NaN)."""
    o, t, mo = _logp(S, B, C, 31 * S + C), _targets(B, C, C), _logp(1, B, C, 17 + C)[0]
    k0, k1 = (1, C - 1) if C >= 3 else (0, C - 1)
    rows = torch.arange(B)
    for x in (o, mo):
        x[..., k1] = x[..., k0]
        x[..., rows % 2 == 0, k0] += 50.0
        x[..., rows % 2 == 0, k1] += 50.0
    if C >= 2:
        hit = rows[rows % 7 == 3]
        o[S - 1, hit, hit % C] = float("-inf")
        t[hit] = (hit % C + 1) % C                           # the target is another class: nll stays finite
    t[5], t[6], t[7], t[8] = -1, C, -(2 ** 40), 2 ** 40
    mo[9, min(2, C - 1)] = float("nan")
    mo[10, :] = float("-inf")
    if variant:
        o[1 % S, 11, :] = float("nan")
        o[0, 12, min(3, C - 1)] = float("nan")
        o[:, 13, :] = float("-inf")
        t[12] = C                                             # (its NaN would otherwise decide nll_sum alone)
        if variant == 2:
            t[11] = -1
    return o, t, mo


@pytest.mark.parametrize("variant", (0, 1, 2))
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("S", (1, 2, 10))
def test_constructed_inputs_equal_the_restatement_exactly(bnn, dev, S, C, variant):
    for B in (65, 100):
        o, t, mo = _constructed(S, B, C, variant)
        rows, tot, _ = _run(bnn, dev, o, t, mo)
        r = ref.metrics(_np(o), _np(t), _np(mo))
        what = "S=%d B=%d C=%d variant=%d" % (S, B, C, variant)
        _compare(rows, tot, r, what)
        assert tot["bad_targets"] >= 4 and tot["rows_with_target"] + tot["bad_targets"] == B == tot["rows"], what
        if C >= 3:                                            # the tie between columns 1 and C - 1 goes to column 1
            even = np.arange(B) % 2 == 0
            plain = even & (np.arange(B) > 13) & (np.arange(B) % 7 != 3)       # (rows without a NaN / -inf of their own)
            assert (rows["pred_ensemble"][plain] == 1).all() and (rows["pred_posterior_mean"][plain] == 1).all(), what
        if variant:
            assert rows["pred_ensemble"][11] == 0 and rows["pred_ensemble"][12] == min(3, C - 1) and rows["pred_ensemble"][13] == 0
            assert np.isnan(rows["entropy"][11]) and np.isnan(rows["entropy"][13]) and tot["entropy_nonfinite"] >= 2
            assert np.isnan(tot["nll_sum"]) if variant == 1 else tot["nll_sum"] == float("inf"), what
        assert rows["pred_posterior_mean"][9] == min(2, C - 1) and rows["pred_posterior_mean"][10] == 0
        with pytest.raises(IndexError):
            acc = bnn.evaluate.EvalAccumulator(C, S, dev)
            acc.update(o.to(dev), t.to(dev))
            acc.result()


# ----------------------------------------------------------------------------------- 3. strided views, read in place
def test_strided_views_are_read_in_place(bnn, dev):
    from bnn_amd import _lib
    ev = bnn.evaluate
    S, B, C = 10, 100, 10
    o, t, mo = _logp(S, B, C, 3), _targets(B, C, 4), _logp(1, B, C, 5)[0]
    r = ref.metrics(_np(o), _np(t), _np(mo))
    nan = float("nan")
    pad_m = torch.full((S, B * C + 12), nan, device=dev)                   # a padded member stride (the head buffer's shape)
    v_m = pad_m[:, :B * C].view(S, B, C)
    v_m.copy_(o)
    pad_r = torch.full((S, B, C + 3), nan, device=dev)                     # padded rows
    v_r = pad_r[:, :, :C]
    v_r.copy_(o)
    pad_mo = torch.full((B, C + 5), nan, device=dev)
    v_mo = pad_mo[:, :C]
    v_mo.copy_(mo)
    for v in (v_m, v_r):
        assert not v.is_contiguous()
        acc = ev.EvalAccumulator(C, S, dev)
        _lib.RECORD = calls = []
        try:
            rows = acc.update(v, t.to(dev), v_mo)
        finally:
            _lib.RECORD = None
        (name, _, args), = [c for c in calls if c[0] == "lbbnn_eval_metrics"]
        a = args[0]._obj
        assert a.logp == v.data_ptr() and a.m_stride == v.stride(0) and a.ldp == v.stride(1)       # no copy was made
        assert a.mean_logp == v_mo.data_ptr() and a.ldm == C + 5
        _compare({k: _np(x) for k, x in rows.items()}, acc.result(), r, "strided")
    # layouts the kernel does not take are copied, not refused: a transposed last dimension, a broadcast member dimension
    rows = ev.ensemble_metrics(o.to(dev).permute(0, 2, 1).contiguous().permute(0, 2, 1), mean_outputs=mo.to(dev))
    assert _same_f32(_np(rows["mean_log_probs"]), r["mean_log_probs"])
    assert np.array_equal(_np(rows["pred_ensemble"]), r["pred_ensemble"])
    assert np.array_equal(_np(rows["pred_posterior_mean"]), r["pred_posterior_mean"])
    one = ev.ensemble_metrics(o[:1].to(dev).expand(S, B, C))
    assert np.array_equal(_np(one["pred_ensemble"]), ref.argmax_rows(ref.ensemble_mean(np.broadcast_to(_np(o[:1]), (S, B, C)))))
    assert "pred_posterior_mean" not in one
    assert float(np.abs(_np(rows["entropy"]).astype(np.float64) - r["entropy"]).max()) < 1e-4


# ----------------------------------------------------------------------------------- 4. accumulation
def test_updates_accumulate_and_totals_are_bitwise_reproducible(bnn, dev):
    ev = bnn.evaluate
    S, C = 10, 10
    parts = [(_logp(S, B, C, 50 + B), _targets(B, C, 60 + B), _logp(1, B, C, 70 + B)[0]) for B in (100, 37, 1000)]
    parts[1][1][3] = C                                                     # one bad target on the way
    on = [tuple(x.to(dev) for x in p) for p in parts]

    def three(acc):
        for o, t, mo in on:
            acc.update(o, t, mo)
        return acc

    a3 = three(ev.EvalAccumulator(C, S, dev))
    a1 = ev.EvalAccumulator(C, S, dev)
    a1.update(*(torch.cat([p[i] for p in on], dim=1 if i == 0 else 0) for i in range(3)))
    r3, r1 = a3.result(strict=False), a1.result(strict=False)
    rr = ref.add_totals([ref.metrics(_np(o), _np(t), _np(mo)) for o, t, mo in parts])
    for k in ref.COUNT_NAMES:
        assert r3[k] == r1[k] == rr[k], k
    assert r3["bad_targets"] == 1 and r3["rows"] == 1137
    assert np.array_equal(r3["correct_member"], r1["correct_member"]) and np.array_equal(r3["correct_member"], rr["correct_member"])
    assert np.array_equal(r3["confusion"], r1["confusion"]) and np.array_equal(r3["confusion"], rr["confusion"])
    scale = float(np.abs(rr["nll_terms"]).sum())
    assert abs(r3["nll_sum"] - r1["nll_sum"]) <= DBL * scale and abs(r3["nll_sum"] - rr["nll_sum"]) <= DBL * scale
    assert abs(r3["entropy_sum"] - r1["entropy_sum"]) <= DBL * abs(r1["entropy_sum"])
    assert a3.updates == 3 and a3.posterior_mean_updates == 3
    # two identical passes: the same bits in every total, the double sums included
    b3 = three(ev.EvalAccumulator(C, S, dev))
    assert torch.equal(a3._totals, b3._totals)
    big = (_logp(S, 4096, C, 9).to(dev), _targets(4096, C, 10).to(dev))
    x1, x2 = ev.EvalAccumulator(C, S, dev), ev.EvalAccumulator(C, S, dev)
    x1.update(*big)
    x2.update(*big)
    assert torch.equal(x1._totals, x2._totals) and x1.result()["rows"] == 4096
    a3.reset()
    assert int(a3._totals.abs().sum()) == 0 and a3.updates == 0
    z = a3.result()
    assert z["rows"] == 0 and z["nll_sum"] == 0.0 and z["entropy_sum"] == 0.0 and int(z["confusion"].sum()) == 0
    three(a3)
    assert torch.equal(a3._totals, b3._totals)                             # and a reset accumulator starts over exactly


# ----------------------------------------------------------------------------------- 5. every family through evaluate_batches
DIMS = (64, 48, 40, 10)
FAMILIES = ("frozen-lrt", "frozen-mnf-planar", "frozen-rnvp-dense", "base-sample", "base-mpm", "vd", "mnf")
SEED = 13


def _model(bnn, dev, family):
    torch.manual_seed(11)
    ev = bnn.evaluate
    if family == "frozen-lrt":
        return ev.freeze(bnn.lrt.BayesianNetwork(DIMS).to(dev).eval())
    if family == "frozen-mnf-planar":
        return ev.freeze(bnn.mnf.BayesianNetwork(DIMS, 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).eval())
    if family == "frozen-rnvp-dense":
        return ev.freeze(bnn.mnf.BayesianNetwork(DIMS, 2, z_flow_type="RNVP", r_flow_type="RNVP").to(dev).eval(), dense=True)
    if family.startswith("base"):
        net = bnn.base.BayesianNetwork(DIMS).to(dev)
        with torch.no_grad():
            for l in (net.l1, net.l2, net.l3):
                l.lambdal.uniform_(-2.5, 2.5)
        return net
    if family == "vd":
        return bnn.vd.BNN(DIMS).to(dev)
    return bnn.mnf.BayesianNetwork(DIMS, 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).eval()


@pytest.mark.parametrize("family", FAMILIES)
def test_evaluate_batches_consumes_the_outputs_of_ensemble_eval(bnn, dev, family):
    """Per batch, after manual_seed: the outputs evaluate_batches hands to the accumulator are bitwise those of ensemble_eval
    (base-mpm: of ensemble_forward(gates="mpm")) from the same seed, and its numbers are the restatement's on those outputs."""
    ev = bnn.evaluate
    S, C = 10, DIMS[-1]
    net = _model(bnn, dev, family)
    g = torch.Generator().manual_seed(2)
    data = [(torch.rand(B, DIMS[0], generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)) for B in (100, 37)]
    mpm = family == "base-mpm"
    want = []
    for i, (x, y) in enumerate(data):
        bnn.manual_seed(SEED + i)
        if mpm:
            want.append({"outputs": ev.ensemble_forward(net, x, S, gates="mpm").clone()})
        else:
            r = ev.ensemble_eval(net, x, y, S)
            want.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()})

    def batches():
        for i, b in enumerate(data):
            bnn.manual_seed(SEED + i)
            yield b

    acc = ev.EvalAccumulator(C, S, dev)
    rec, inner = [], acc.update

    def update(o, t, mo=None):
        rec.append((o.clone(), t.clone(), None if mo is None else mo.clone()))
        return inner(o, t, mo)

    acc.update = update
    res = ev.evaluate_batches(net, batches(), S, acc=acc, gates="mpm" if mpm else "sample", posterior_mean=not mpm)
    assert len(rec) == 2
    parts = []
    for w, (o, t, mo) in zip(want, rec):
        assert torch.equal(o, w["outputs"]), family
        has_mean = family not in ("vd", "base-mpm")
        assert (mo is not None) == has_mean
        r = ref.metrics(_np(o), _np(t), None if mo is None else _np(mo))
        if has_mean:
            assert np.array_equal(r["pred_posterior_mean"], _np(w["pred_posterior_mean"]))      # the same forward: no ties here
        parts.append(r)
    rr = ref.add_totals(parts)
    for k in ref.COUNT_NAMES:
        assert res[k] == rr[k], (family, k)
    assert res["rows"] == 137 == res["rows_with_target"]
    assert np.array_equal(res["correct_member"], rr["correct_member"]) and np.array_equal(res["confusion"], rr["confusion"])
    _close_sum(res["nll_sum"], rr["nll_terms"], family)
    assert res["accuracy_ensemble"] == rr["correct_ensemble"] / 137
    assert (res["accuracy_posterior_mean"] is None) == (not has_mean)
    if not mpm and "correct_ensemble" in want[0]:
        # ensemble_eval's own count comes from torch's mean (another summation order): equal unless two classes of a row tie
        # to the last bit, which these inputs do not have -- reported, not required
        print(family, "correct_ensemble", res["correct_ensemble"], "ensemble_eval", sum(w["correct_ensemble"] for w in want))
    # without an accumulator of its own evaluate_batches builds one
    bnn.manual_seed(SEED)
    again = ev.evaluate_batches(net, [data[0]], S, gates="mpm" if mpm else "sample", posterior_mean=not mpm)
    for k in ref.COUNT_NAMES:
        assert again[k] == parts[0][k], (family, k)


# ----------------------------------------------------------------------------------- 6. the graphed step
@pytest.mark.parametrize("family", ("frozen-lrt", "frozen-mnf-planar"))
def test_graphed_eval_step_equals_eager_updates_bitwise(bnn, dev, family):
    ev = bnn.evaluate
    S, C, B = 10, DIMS[-1], 100
    fz = _model(bnn, dev, family)
    g = torch.Generator().manual_seed(4)
    data = [(torch.rand(B, DIMS[0], generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)) for _ in range(3)]
    bnn.manual_seed(SEED)
    acc_g = ev.EvalAccumulator(C, S, dev)
    acc_g.update(fz.ensemble(data[0][0], S), data[0][1])                  # totals that must survive the build
    before = acc_g._totals.clone()
    st = bnn.ops.RngState.get(dev)
    rng_before = st.t.clone()
    step = bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], S, acc_g)
    assert torch.equal(acc_g._totals, before) and torch.equal(st.t, rng_before) and acc_g.updates == 1
    acc_g.reset()
    bnn.manual_seed(SEED)
    got = []
    for x, y in data:
        rows = step(x, y)
        got.append({k: v.clone() for k, v in rows.items()})
    acc_e = ev.EvalAccumulator(C, S, dev)
    bnn.manual_seed(SEED)
    for (x, y), rows_g in zip(data, got):
        o = fz.ensemble(x, S)
        rows_e = acc_e.update(o, y, fz(x, sample=False))
        assert sorted(rows_e) == sorted(rows_g) and "pred_posterior_mean" in rows_g
        for k in rows_e:
            assert torch.equal(rows_e[k], rows_g[k]), (family, k)
    assert torch.equal(acc_g._totals, acc_e._totals)
    assert acc_g.updates == 3 and acc_g.result()["rows"] == 3 * B
    assert not torch.equal(got[0]["mean_log_probs"], got[1]["mean_log_probs"])                # fresh members, fresh batches
