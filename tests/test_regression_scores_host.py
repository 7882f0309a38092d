"""CPU tier of the regression scores (include/lbbnn.h: lbbnn_eval_regression_scores; evaluate.ensemble_scores /
RegressionScoreAccumulator / predict_regression): the float64 reference against quadrature, the single-normal closed form and
gaussian_ref; every early return of the two entry points in the order the code takes it (nothing is launched); the ctypes struct
against gcc; ``RegressionScoreAccumulator.result`` from hand-filled totals; the refusals, those reached before the library is
among them."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy import integrate, special

import gaussian_ref as gref
import regression_scores_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------- the reference
def _mixture(S, seed):
    r = np.random.default_rng(seed)
    return r.normal(0.0, 1.0, S), np.exp(r.normal(-0.5, 0.8, S)), float(r.normal(0.3, 1.5))


@pytest.mark.parametrize("S", (1, 2, 5))
def test_reference_crps_is_the_integral_of_the_squared_cdf_difference(S):
    for seed in range(4):
        m, v, y = _mixture(S, 10 * S + seed)
        sd = np.sqrt(v)
        F = lambda x: float(special.ndtr((x - m) / sd).mean())
        lo, hi = float((m - 12 * sd).min()), float((m + 12 * sd).max())
        pts = sorted(set(m.tolist()))
        left = integrate.quad(lambda x: F(x) ** 2, min(lo, y - 1.0), y, points=[p for p in pts if min(lo, y - 1.0) < p < y] or None,
                              epsabs=1e-13, epsrel=1e-13, limit=400)[0]
        right = integrate.quad(lambda x: (F(x) - 1.0) ** 2, y, max(hi, y + 1.0), points=[p for p in pts if y < p < max(hi, y + 1.0)] or None,
                               epsabs=1e-13, epsrel=1e-13, limit=400)[0]
        c, mag = ref.crps_mixture(m.reshape(S, 1, 1), v.reshape(S, 1, 1), np.full((1, 1), y))
        assert abs(float(c[0, 0]) - (left + right)) <= 1e-10 * float(mag[0, 0]), (S, seed, float(c[0, 0]), left + right)
        assert 0.0 < float(c[0, 0]) <= float(mag[0, 0])


def test_reference_crps_of_one_member_is_the_normal_closed_form():
    r = np.random.default_rng(0)
    m, lv, y = r.normal(0, 2, (1, 7, 3)), r.normal(-0.5, 1.0, (1, 7, 3)), r.normal(0, 3, (7, 3))
    c, mag = ref.crps_mixture(m, np.exp(lv), y)
    want = ref.crps_normal(m[0], np.exp(0.5 * lv[0]), y)
    assert float(np.abs(c - want).max()) <= 1e-13 * float(mag.max())
    # and through metrics(), from float32 inputs
    got = ref.metrics(m.astype(np.float32), y.astype(np.float32), lv.astype(np.float32), (0.9,))
    m32, lv32, y32 = (np.asarray(a, np.float32).astype(np.float64) for a in (m, lv, y))
    assert float(np.abs(got["crps"] - ref.crps_normal(m32[0], np.exp(0.5 * lv32[0]), y32)).max()) <= 1e-13 * float(got["crps_mag"].max())
    # one normal: the quantiles are mean +- 1.6449 sd
    z = special.ndtri(0.5 * (1.0 + ref.level_f32(0.9)))
    assert float(np.abs(got["upper"][0] - (m32[0] + z * np.exp(0.5 * lv32[0]))).max()) <= 1e-12 * 20
    assert float(np.abs(got["lower"][0] - (m32[0] - z * np.exp(0.5 * lv32[0]))).max()) <= 1e-12 * 20


def test_reference_equals_gaussian_ref_for_a_noise_level_per_unit():
    r = np.random.default_rng(1)
    S, B, O = 5, 11, 3
    out = r.normal(0, 1, (S, B, O)).astype(np.float32)
    y = r.normal(0, 1.5, (B, O)).astype(np.float32)
    y[2, 1], y[7, 0] = np.nan, np.inf
    lv = r.normal(-0.5, 0.6, O).astype(np.float32)
    a, b = ref.metrics(out, y, lv, (0.5,)), gref.metrics(out, y, lv)
    for k in ("pred_mean", "epistemic_var"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    for k in ("aleatoric_var", "total_std", "sq_err", "log_density", "pit", "log_density_mag"):
        assert np.allclose(a[k], b[k], rtol=1e-13, atol=0, equal_nan=True), k
    assert np.array_equal(a["valid"], b["valid"]) and a["finite"].all()
    # the same block as a per-element and a per-member operand gives the same numbers
    for form in (np.broadcast_to(lv, (B, O)), np.broadcast_to(lv, (S, B, O))):
        c = ref.metrics(out, y, np.ascontiguousarray(form), (0.5,))
        for k in ("crps", "lower", "upper", "interval_score", "pit"):
            assert np.array_equal(c[k], a[k], equal_nan=True), k
    # non-finite elements: an infinite member, a log-variance of 81, a NaN one
    out2, lv3 = out.copy(), np.ascontiguousarray(np.broadcast_to(lv, (S, B, O))).copy()
    out2[1, 0, 0], lv3[2, 3, 1], lv3[0, 4, 2] = np.inf, 81.0, np.nan
    d = ref.metrics(out2, y, lv3, (0.5,))
    bad = np.zeros((B, O), bool)
    bad[0, 0] = bad[3, 1] = bad[4, 2] = True
    assert np.array_equal(d["finite"], ~bad)
    for k in ("pred_mean", "epistemic_var", "aleatoric_var", "total_std", "sq_err", "crps", "pit"):
        assert np.isnan(d[k][bad]).all() and (np.isfinite(d[k][~bad & d["valid"]])).all(), k
    assert np.isnan(d["lower"][0][bad]).all() and np.isfinite(d["lower"][0][~bad]).all()


# ------------------------------------------------------------------------------------------- the C entry points
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


def _args(**kw):
    from bnn_amd import _lib
    a = _lib.EvalScoresArgs()
    base = dict(out=4096, m_stride=16, ldp=3, log_var=4096, lv_mstride=0, lv_ld=0, S=2, B=4, O=3, pit_bins=20, n_levels=1,
                levels=(0.9,))
    base.update(kw)
    for i, p in enumerate(base.pop("levels")):
        a.levels[i] = p
    for k, v in base.items():
        setattr(a, k, v)
    return a


def test_scores_early_return_codes_in_order(lib):
    """Each row of a code is also invalid at a LATER check (an odd ``out``, or B == 0), so it pins the precedence."""
    call = lambda **kw: lib.lbbnn_eval_regression_scores(ctypes.byref(_args(**kw)), None)
    tot = dict(counts=4096, sums=4096, pit_hist=4096, work=4096)
    assert lib.lbbnn_eval_regression_scores(None, None) == E_NULL
    assert call(out=None, S=0) == E_NULL and call(log_var=None, S=0) == E_NULL
    for k in tot:                                                                      # some but not all of the totals
        assert call(**dict(tot, **{k: None}), S=0) == E_NULL, k
    assert call(counts=4096, n_levels=5) == E_NULL
    odd = dict(out=4098)
    assert call(S=0, **odd) == E_SHAPE and call(S=65, m_stride=16, **odd) == E_SHAPE and call(S=64, **odd) == E_ALIGN
    assert call(O=0, ldp=0, **odd) == E_SHAPE and call(O=17, ldp=17, m_stride=80, **odd) == E_SHAPE
    assert call(B=-1, **odd) == E_SHAPE
    assert call(ldp=2, **odd) == E_SHAPE
    assert call(mean_out=4096, ldm=2, **odd) == E_SHAPE and call(target=4096, ldt=2, **odd) == E_SHAPE
    assert call(m_stride=11, **odd) == E_SHAPE                                         # (B - 1) * ldp + O = 12
    assert call(B=1 << 30, m_stride=1 << 40, **odd) == E_SHAPE
    # the log-variance operand
    assert call(lv_ld=2, **odd) == E_SHAPE and call(lv_ld=-3, **odd) == E_SHAPE
    assert call(lv_mstride=-16, lv_ld=3, **odd) == E_SHAPE
    assert call(lv_mstride=16, lv_ld=0, **odd) == E_SHAPE                              # a member stride needs a row stride
    assert call(lv_mstride=11, lv_ld=3, **odd) == E_SHAPE                              # (B - 1) * lv_ld + O = 12
    assert call(lv_mstride=12, lv_ld=3, **odd) == E_ALIGN and call(lv_ld=3, **odd) == E_ALIGN
    assert call(lv_mstride=11, lv_ld=3, S=1, **odd) == E_ALIGN                         # one member: its stride is not read
    # the levels
    assert call(n_levels=5, **odd) == E_SHAPE and call(n_levels=-1, **odd) == E_SHAPE
    for bad in (0.009, 0.9995, 0.0, 1.0, float("nan"), -0.5):
        assert call(levels=(bad,), **odd) == E_SHAPE, bad
        assert call(n_levels=2, levels=(0.5, bad), **odd) == E_SHAPE, bad
    assert call(n_levels=0, levels=(7.0,), **odd) == E_ALIGN                           # levels beyond n_levels are not read
    assert call(n_levels=4, levels=(0.01, 0.5, 0.9, 0.999), **odd) == E_ALIGN          # the ends of the range are inside it
    assert call(**tot, pit_bins=0, **odd) == E_SHAPE and call(**tot, pit_bins=1025, **odd) == E_SHAPE
    assert call(pit_bins=0, B=0) == 0                                                  # pit_bins matters with totals only
    # alignment, ahead of the empty batch
    for k in ("out", "mean_out", "target", "log_var", "pred_mean", "epistemic_var", "aleatoric_var", "total_std", "sq_err",
              "log_density", "pit", "crps", "lower", "upper", "interval_score"):
        extra = dict(ldm=3) if k == "mean_out" else dict(ldt=3) if k == "target" else {}
        assert call(**{k: 4098}, B=0, **extra) == E_ALIGN, k
    for k in tot:
        assert call(**dict(tot, **{k: 4100}), B=0) == E_ALIGN, k
    # an empty batch: a successful no-op
    assert call(B=0, m_stride=0) == 0 and call(**tot, B=0) == 0 and call(B=0, n_levels=4, levels=(0.01, 0.5, 0.9, 0.999)) == 0
    assert call(B=0, lv_mstride=3, lv_ld=3) == 0


def test_scores_work_bytes(lib):
    from bnn_amd import _lib
    wb = lib.lbbnn_eval_regression_scores_work_bytes
    n = _lib.SCORE_SUMS
    assert n == 18 and _lib.SCORE_COUNTS == 9
    # one set of partial sums per workgroup of 64 elements
    assert wb(10, 0, 1, 2) == 8 * n and wb(10, 64, 1, 2) == 8 * n and wb(10, 65, 1, 2) == 2 * 8 * n and wb(3, 257, 5, 0) == 21 * 8 * n
    assert wb(64, 9, 2, 4) == 8 * n and wb(1, 4096, 16, 1) == 1024 * 8 * n
    for bad in ((0, 4, 1, 1), (65, 4, 1, 1), (10, 4, 0, 1), (10, 4, 17, 1), (10, -1, 1, 1), (10, 4, 1, -1), (10, 4, 1, 5)):
        assert wb(*bad) == 0, bad


def test_scores_struct_layout_matches_the_header(tmp_path, lib):
    from bnn_amd import _lib
    names = ("lv_mstride", "crps", "interval_score", "counts", "pit_bins", "n_levels", "levels")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                   'printf("%%zu %%d %%d %%d %%d", sizeof(lbbnn_eval_scores_args_t), LBBNN_SCORE_COUNTS, LBBNN_SCORE_SUMS, '
                   'LBBNN_SCORE_MAX_LEVELS, LBBNN_SCORE_MAX_MEMBERS);\n%s\nprintf("\\n");\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "lbbnn.h"),
                      "\n".join('printf(" %%zu", offsetof(lbbnn_eval_scores_args_t, %s));' % n for n in names)))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    cls = _lib.EvalScoresArgs
    assert got[0] == ctypes.sizeof(cls)
    assert got[1:5] == [_lib.SCORE_COUNTS, _lib.SCORE_SUMS, _lib.SCORE_MAX_LEVELS, _lib.SCORE_MAX_MEMBERS]
    assert got[5:] == [getattr(cls, n).offset for n in names]
    assert _lib.SCORE_SUM_NAMES[:_lib.REG_SUMS] == _lib.REG_SUM_NAMES and len(_lib.SCORE_SUM_NAMES) == _lib.REG_SUMS + 2
    assert lib.lbbnn_abi_version() == 1                          # two new symbols, the same ABI


# ------------------------------------------------------------------------------------------- host arithmetic
def test_score_accumulator_result_from_hand_filled_totals(bnn):
    from bnn_amd import _lib
    ev = bnn.evaluate
    acc = ev.RegressionScoreAccumulator(2, 5, "cpu", -1.0, pit_bins=20, levels=(0.5, 0.9))
    assert isinstance(acc, ev.RegressionAccumulator) and acc._log_var.tolist() == [-1.0, -1.0] and acc.levels == (0.5, 0.9)
    nc, ns = _lib.SCORE_COUNTS, _lib.SCORE_SUMS
    assert acc._totals.numel() == nc + ns + 20
    hist = np.arange(20, dtype=np.int64)                         # 190 scored elements
    h = np.zeros(nc + ns + 20, np.int64)
    h[:nc] = [200, 194, 2, 6, 190, 101, 170, 0, 0]
    sums = np.array([47.5, 76.0, -133.0, 9.7, 58.2, 19.0, 401.9, 95.0, 48.5, 57.0, 133.0, 323.0, 0, 0, 171.0, 380.0, 0, 0])
    h[nc:nc + ns] = sums.view(np.int64)
    h[nc + ns:] = hist
    acc._totals.copy_(torch.from_numpy(h))
    with pytest.raises(IndexError, match="2 target"):
        acc.result()
    r = acc.result(strict=False)
    # everything RegressionAccumulator.result returns, under the same keys, from the same numbers
    old = ev.RegressionAccumulator(2, 5, "cpu", -1.0, pit_bins=20)
    old._totals.copy_(torch.from_numpy(np.concatenate([h[:5], h[nc:nc + 8], h[nc + ns:]])))
    want = old.result(strict=False)
    for k, v in want.items():
        if k == "coverage":
            assert r[k](0.9) == v(0.9) == hist[1:19].sum() / 190
        elif k == "pit_hist":
            assert np.array_equal(r[k], v)
        else:
            assert r[k] == v or (v != v and r[k] != r[k]), k
    assert r["rmse"] == math.sqrt(47.5 / 190) and r["mean_total_var"] == 58.2 / 194 and r["rmse_posterior_mean"] is None
    assert r["mean_aleatoric_var"] == 48.5 / 194 and r["crps"] == 57.0 / 190 and r["crps_sum"] == 57.0
    assert r["levels"] == (0.5, 0.9) and [d["level"] for d in r["intervals"]] == [0.5, 0.9]
    i50, i90 = r["intervals"]
    assert (i50["inside"], i50["coverage"], i50["mean_width"], i50["mean_interval_score"]) == (101, 101 / 190, 133.0 / 190, 171.0 / 190)
    assert (i90["inside"], i90["coverage"], i90["mean_width"], i90["mean_interval_score"]) == (170, 170 / 190, 323.0 / 190, 380.0 / 190)
    acc.posterior_mean_updates = 1
    assert acc.result(strict=False)["rmse_posterior_mean"] == math.sqrt(95.0 / 190)
    acc.reset()
    assert int(acc._totals.abs().sum()) == 0 and (acc.updates, acc.posterior_mean_updates) == (0, 0)
    empty = ev.RegressionScoreAccumulator(1, 1, "cpu", "output", levels=()).result()
    assert math.isnan(empty["crps"]) and math.isnan(empty["mean_aleatoric_var"]) and empty["intervals"] == []


# ------------------------------------------------------------------------------------------- refusals
def test_score_accumulator_constructor_refusals(bnn):
    ev = bnn.evaluate
    mk = lambda **kw: ev.RegressionScoreAccumulator(**dict(dict(units=1, samples=2, device="cpu", log_var=0.0), **kw))
    for kw, what in ((dict(units=0), "units"), (dict(units=17), "units"), (dict(samples=0), "members"), (dict(samples=65), "1 to 64 members"),
                     (dict(pit_bins=0), "PIT"), (dict(pit_bins=1025), "PIT"), (dict(levels=(0.1, 0.2, 0.3, 0.4, 0.5)), "at most 4"),
                     (dict(levels=(0.5, 0.9995)), "level"), (dict(levels=(0.005,)), "level"), (dict(levels=(float("nan"),)), "level"),
                     (dict(levels=0.9), "sequence"), (dict(log_var="outputs"), "log_var")):
        with pytest.raises(ValueError, match=what):
            mk(**kw)
    for lv in (None, True, torch.zeros(2), torch.zeros(1, dtype=torch.float64), torch.zeros(1, device="meta")):
        with pytest.raises(ValueError, match="log_var"):
            mk(log_var=lv)
    assert mk(samples=64, levels=(0.01, 0.5, 0.9, 0.999)).levels == (0.01, 0.5, 0.9, 0.999) and mk(levels=()).levels == ()
    assert mk(log_var="output").in_output and not mk().in_output


def test_refusals_that_are_reached_before_the_library_is(bnn, monkeypatch):
    from bnn_amd import _lib
    ev = bnn.evaluate

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    acc = ev.RegressionScoreAccumulator(1, 2, "cpu", "output")
    with pytest.raises(ValueError, match=r"2 \* units = 2 columns.*got 3"):          # names both numbers
        acc.update(torch.zeros(2, 4, 3), torch.zeros(4, 1))
    with pytest.raises(ValueError, match="reads log_var from the outputs"):
        acc.update(torch.zeros(2, 4, 2), torch.zeros(4, 1), log_var=torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="HIP"):                                     # there is no CPU path
        acc.update(torch.zeros(2, 4, 2), torch.zeros(4, 1))
    plain = ev.RegressionScoreAccumulator(3, 2, "cpu", 0.0)
    with pytest.raises(ValueError, match="update takes log_var"):
        plain.update(torch.zeros(2, 4, 3), None, log_var=0.5)
    with pytest.raises(RuntimeError, match="HIP"):
        plain.update(torch.zeros(2, 4, 3), torch.zeros(4, 3))
    x = torch.zeros(2, 4, 3)
    with pytest.raises(ValueError, match="at most 4"):
        ev.ensemble_scores(x, None, 0.0, levels=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match="level"):
        ev.ensemble_scores(x, None, 0.0, levels=(1.0,))
    with pytest.raises(ValueError, match="\"output\""):
        ev.ensemble_scores(x, None, "column")
    with pytest.raises(ValueError, match="RegressionScoreAccumulator"):
        ev.ensemble_scores(x, None, 0.0, acc=ev.RegressionAccumulator(3, 2, "cpu", 0.0))
    with pytest.raises(RuntimeError, match="HIP"):
        ev.ensemble_scores(x, None, 0.0)
    # predict_regression: the model, the member cap, the levels
    fz = ev.FrozenNetwork((20, 2), "lrt", head="identity")
    with pytest.raises(ValueError, match="1 to 64 members, got 65"):
        ev.predict_regression(fz, torch.zeros(4, 20), 65, "output")
    with pytest.raises(ValueError, match="at most 4"):
        ev.predict_regression(fz, torch.zeros(4, 20), 4, "output", levels=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match="identity"):
        ev.predict_regression(bnn.lrt.BayesianNetwork((20, 2)), torch.zeros(4, 20), 4, 0.0)
    with pytest.raises(ValueError, match="identity"):
        ev.predict_regression(ev.FrozenNetwork((20, 2), "lrt"), torch.zeros(4, 20), 4, 0.0)


def test_the_existing_pairing_refusals_hold_for_the_new_accumulator(bnn):
    ev = bnn.evaluate
    acc = ev.RegressionScoreAccumulator(3, 2, "cpu", 0.0)
    with pytest.raises(ValueError, match="a RegressionAccumulator takes a model with head=\"identity\", this one has head='log_softmax'"):
        ev.evaluate_batches(bnn.lrt.BayesianNetwork((20, 3)), [], 2, acc=acc)
    net = bnn.lrt.BayesianNetwork((20, 2), head="identity")
    with pytest.raises(ValueError, match="uncertainty"):
        ev.evaluate_batches(net, [], 2, acc=ev.RegressionScoreAccumulator(1, 2, "cpu", "output"),
                            uncertainty=ev.UncertaintyAccumulator(2, 2, "cpu"))
    with pytest.raises(ValueError, match="gates"):
        ev.evaluate_batches(net, [], 2, acc=ev.RegressionScoreAccumulator(1, 2, "cpu", "output"), gates="mpm")
    # no batches: the (empty) totals of the accumulator, with the new keys
    res = ev.evaluate_batches(net, [], 2, acc=ev.RegressionScoreAccumulator(1, 2, "cpu", "output"))
    assert res["elements"] == 0 and math.isnan(res["crps"]) and len(res["intervals"]) == 2
    # the unchanged names keep their refusals
    with pytest.raises(ValueError, match="log_var"):
        ev.RegressionAccumulator(1, 2, "cpu", "output")
    with pytest.raises(ValueError, match="log_var"):
        ev.RegressionAccumulator(1, 2, "cpu", torch.zeros(4, 1))
