"""CPU tier of the regression column: the identity head's construction and refusals, ``elbo_gaussian_loss`` on CPU tensors and
its guards, the early return codes of the four new entry points (nothing is launched), the ctypes struct against gcc, and the
host arithmetic of ``TrainMonitor.result`` / ``RegressionAccumulator.result`` / ``pit_coverage`` from hand-filled buffers."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gaussian_ref as ref

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


# ------------------------------------------------------------------------------------------- the head
def _nets(bnn, seed, dims=(20, 8, 1), **kw):
    torch.manual_seed(seed)
    a = bnn.lrt.BayesianNetwork(dims, **kw)
    torch.manual_seed(seed)
    b = bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar", **kw)
    return a, b


def test_identity_head_has_the_state_dict_of_its_log_softmax_twin(bnn):
    from bnn_amd import layers
    assert layers.HEADS == ("log_softmax", "sigmoid", "identity")
    for dims in ((20, 8, 1), (12, 8, 3)):
        for plain, ident in zip(_nets(bnn, 3, dims), _nets(bnn, 3, dims, head="identity")):
            assert plain.head == "log_softmax" and ident.head == "identity"
            a, b = plain.state_dict(), ident.state_dict()
            assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_identity_head_refusals(bnn):
    ev = bnn.evaluate
    with pytest.raises(ValueError, match="at most 16"):
        bnn.lrt.BayesianNetwork((20, 17), head="identity")
    with pytest.raises(ValueError, match="at most 16"):
        bnn.mnf.BayesianNetwork((20, 17), 2, head="identity")
    assert bnn.lrt.BayesianNetwork((20, 16), head="identity").dims[-1] == 16
    with pytest.raises(ValueError, match="at most 16"):
        ev.FrozenNetwork((20, 17), "lrt", head="identity")
    assert ev.FrozenNetwork((20, 3), "lrt", head="identity").head == "identity"
    assert "head=identity" in repr(ev.FrozenNetwork((20, 3), "lrt", head="identity"))
    net = bnn.lrt.BayesianNetwork((20, 1), head="identity")
    with pytest.raises(NotImplementedError, match="identity"):
        bnn.parallel.DataParallelELBO(net)
    # out of scope: the other families keep refusing the keyword value
    with pytest.raises(ValueError):
        bnn.base.BayesianNetwork((20, 1), head="identity")
    x = torch.zeros(4, 20)
    for call in (lambda: ev.ensemble_forward(net, x, 2, log_probs=True),
                 lambda: ev.ensemble_forward(net, x, 2, batched=True, log_probs=True),
                 lambda: ev.FrozenNetwork((20, 1), "lrt", head="identity").ensemble(x, 2, log_probs=True),
                 lambda: ev.FrozenNetwork((20, 1), "lrt", head="identity")(x, log_probs=True)):
        with pytest.raises(ValueError, match="log_probs"):
            call()
    fz = ev.FrozenNetwork((20, 1), "lrt", head="identity")
    for model in (net, fz):
        with pytest.raises(ValueError, match="RegressionAccumulator"):
            ev.ensemble_eval(model, x, None, 2)
        with pytest.raises(ValueError, match="RegressionAccumulator"):
            ev.predictive_entropy(model)
        with pytest.raises(ValueError, match="RegressionAccumulator"):
            ev.evaluate_batches(model, [], 2)                                          # a missing acc
        with pytest.raises(ValueError, match="RegressionAccumulator"):
            ev.evaluate_batches(model, [], 2, acc=ev.EvalAccumulator(2, 2, "cpu"))
        with pytest.raises(ValueError, match="uncertainty"):
            ev.evaluate_batches(model, [], 2, acc=ev.RegressionAccumulator(1, 2, "cpu", 0.0),
                                uncertainty=ev.UncertaintyAccumulator(2, 2, "cpu"))
    with pytest.raises(ValueError, match="identity"):                                  # a regression accumulator, a classifier
        ev.evaluate_batches(bnn.lrt.BayesianNetwork((20, 3)), [], 2, acc=ev.RegressionAccumulator(3, 2, "cpu", 0.0))
    # no batches: the (empty) totals of the accumulator
    assert ev.evaluate_batches(net, [], 2, acc=ev.RegressionAccumulator(1, 2, "cpu", 0.0))["elements"] == 0


# ------------------------------------------------------------------------------------------- elbo_gaussian_loss on CPU tensors
@pytest.mark.parametrize("per_element", (False, True))
@pytest.mark.parametrize("with_kl", (False, True))
@pytest.mark.parametrize("shape", ((15, 1), (5, 3)))
def test_elbo_gaussian_loss_on_cpu_tensors_is_gaussian_nll_loss(bnn, shape, with_kl, per_element):
    g = torch.Generator().manual_seed(1)
    m = torch.randn(shape, generator=g, dtype=torch.float64) * 2
    y = torch.randn(shape, generator=g, dtype=torch.float64) * 2
    lv = torch.randn(shape if per_element else shape[1:], generator=g, dtype=torch.float64)
    got = []
    for fn in ("ours", "torch"):
        mv, lvv = m.clone().requires_grad_(True), lv.clone().requires_grad_(True)
        kl = torch.tensor(3.5, dtype=torch.float64, requires_grad=True) if with_kl else None
        if fn == "ours":
            loss = bnn.elbo_gaussian_loss(mv.float(), y.float(), lvv.float(), kl.float() if with_kl else None, 5)
        else:
            loss = F.gaussian_nll_loss(mv, y, lvv.exp().expand(shape), full=True, reduction="sum", eps=0.0)
            loss = loss + kl / 5 if with_kl else loss
        loss.backward()
        got.append((loss.detach().double(), mv.grad, lvv.grad, kl.grad if with_kl else None))
    tol = lambda a: 1e-5 * float(a.abs().max()) + 1e-6                                 # the CPU form runs in fp32
    assert abs(float(got[0][0] - got[1][0])) <= 2e-6 * float(ref.magnitude(m, y, lv).sum() + 1)
    assert float((got[0][1] - got[1][1]).abs().max()) <= tol(got[1][1])
    assert float((got[0][2] - got[1][2]).abs().max()) <= tol(got[1][2])
    if with_kl:
        assert abs(float(got[0][3]) - 0.2) <= 1e-7
    # the numpy restatement the GPU tests use is the same expression
    assert abs(ref.loss(m, y, lv, 3.5 if with_kl else None, 0.2) - float(got[1][0])) <= 1e-12 * float(ref.magnitude(m, y, lv).sum() + 1)
    gm, glv, _ = ref.grads(1.0, m, y, lv, 0.2)
    assert float(np.abs(gm - got[1][1].numpy()).max()) <= 1e-12 * float(np.abs(gm).max())
    assert float(np.abs(glv - got[1][2].numpy()).max()) <= 1e-12 * float(ref.grad_lv_magnitude(1.0, m, y, lv).max())
    if shape[1] == 1:                                                                  # (B,) targets against (B, 1) means
        a = bnn.elbo_gaussian_loss(m.float(), y.float().reshape(-1), lv.float())
        assert torch.equal(a, bnn.elbo_gaussian_loss(m.float(), y.float(), lv.float()))


def test_elbo_gaussian_loss_on_cpu_skips_bad_targets_and_fills_stats(bnn):
    g = torch.Generator().manual_seed(2)
    m, y, lv = torch.randn(6, 2, generator=g), torch.randn(6, 2, generator=g), torch.randn(2, generator=g)
    y[1, 0], y[4, 1], y[5, 0] = float("nan"), float("inf"), float("-inf")
    mv = m.clone().requires_grad_(True)
    st = torch.zeros(4, dtype=torch.float64)
    loss = bnn.elbo_gaussian_loss(mv, y, lv, stats=st)
    loss.backward()
    assert abs(float(loss.detach()) - ref.loss(m, y, lv)) <= 2e-6 * float(ref.magnitude(m, y, lv).sum())
    assert bool(torch.isfinite(mv.grad).all()) and float(mv.grad[1, 0]) == 0.0 and float(mv.grad[4, 1]) == 0.0
    bnn.elbo_gaussian_loss(m, y, lv, stats=st)
    want = ref.stats(m, y)
    assert st[2:].tolist() == [18.0, 6.0] and want[2:] == [9.0, 3.0]
    assert abs(float(st[0]) - 2 * want[0]) <= 1e-5 * want[0] and abs(float(st[1]) - 2 * want[1]) <= 1e-5 * want[1]


def test_elbo_gaussian_loss_guards_raise_before_the_library_is_reached(bnn, monkeypatch):
    from bnn_amd import _lib

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    m, y, lv = torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(2)
    loss = bnn.elbo_gaussian_loss
    with pytest.raises(ValueError, match=r"\(B, O\)"):
        loss(torch.zeros(4), torch.zeros(4), torch.zeros(1))
    with pytest.raises(ValueError, match="mean must be float32"):
        loss(m.double(), y, lv)
    with pytest.raises(ValueError, match="target must be a tensor"):
        loss(m, 0.0, lv)
    with pytest.raises(ValueError, match="target must be float32"):
        loss(m, y.long(), lv)
    with pytest.raises(ValueError, match="meta"):
        loss(m, torch.zeros(4, 2, device="meta"), lv)
    with pytest.raises(ValueError, match="target has shape"):
        loss(m, torch.zeros(3, 2), lv)
    with pytest.raises(ValueError, match="target has shape"):
        loss(m, torch.zeros(4), lv)                                                    # (B,) stands for (B, 1) only
    with pytest.raises(ValueError, match="contiguous"):
        loss(m, torch.zeros(4, 3)[:, :2], lv)
    with pytest.raises(ValueError, match="log_var must be a tensor"):
        loss(m, y, 0.0)
    with pytest.raises(ValueError, match="log_var must be float32"):
        loss(m, y, lv.double())
    with pytest.raises(ValueError, match="log_var is on meta"):
        loss(m, y, torch.zeros(2, device="meta"))
    for bad in (torch.zeros(3), torch.zeros(4, 1), torch.zeros(()), torch.zeros(2, 4)):
        with pytest.raises(ValueError, match="log_var has shape"):
            loss(m, y, bad)
    with pytest.raises(ValueError, match="stats"):
        loss(m, y, lv, stats=torch.zeros(4))                                           # float32, not float64
    with pytest.raises(ValueError, match="stats"):
        loss(m, y, lv, stats=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="TrainMonitor"):
        loss(m, y, lv, monitor=object())
    with pytest.raises(ValueError, match="built for 3"):
        loss(m, y, lv, monitor=bnn.TrainMonitor(3, "cpu"))
    with pytest.raises(ValueError, match="empty batch"):
        loss(torch.zeros(0, 2), torch.zeros(0, 2), lv, monitor=bnn.TrainMonitor(2, "cpu"))
    with pytest.raises(ValueError, match="kl must be"):
        loss(m, y, lv, 3.0, monitor=bnn.TrainMonitor(2, "cpu"))
    with pytest.raises(ValueError, match="fused HIP loss"):
        loss(m, y, lv, monitor=bnn.TrainMonitor(2, "cpu"))


# ------------------------------------------------------------------------------------------- the C entry points
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
_F, _ODD4, _ODD8 = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(4100)
_K = ctypes.c_float(0.2)

# name -> (a call that would launch, [(changes, code)]): every early return in the order the code takes it; each row but the
# first of a code is also invalid at a LATER check, so it pins the precedence
_LOSS = dict(mean=_F, ldm=3, target=_F, ldt=3, log_var=_F, ldv=0, B=4, O=3, kl=None, kl_scale=_K, loss=_F, stats=None, lv_cols=None)
_LOSS_ROWS = [
    (dict(mean=None, O=0), E_NULL), (dict(target=None, B=-1), E_NULL), (dict(log_var=None, ldm=2), E_NULL),
    (dict(loss=None, stats=_ODD8), E_NULL),
    (dict(B=-1, mean=_ODD4), E_SHAPE), (dict(O=0, ldm=0, ldt=0, mean=_ODD4), E_SHAPE), (dict(O=17, ldm=17, ldt=17, kl=_ODD4), E_SHAPE),
    (dict(B=1 << 30, loss=_ODD4), E_SHAPE), (dict(ldm=2, loss=_ODD4), E_SHAPE), (dict(ldt=2, stats=_ODD8), E_SHAPE),
    (dict(ldv=2, stats=_ODD8), E_SHAPE), (dict(ldv=-3, stats=_ODD8), E_SHAPE),
    (dict(ldv=3, lv_cols=_F, stats=_ODD8), E_SHAPE),                                   # column sums of a per-element log_var
    (dict(mean=_ODD4), E_ALIGN), (dict(target=_ODD4), E_ALIGN), (dict(log_var=_ODD4), E_ALIGN), (dict(kl=_ODD4), E_ALIGN),
    (dict(loss=_ODD4), E_ALIGN), (dict(lv_cols=_ODD4), E_ALIGN), (dict(stats=_ODD8), E_ALIGN),
]
_MON = dict(_LOSS, totals=_F, guard=None)
_MON_ROWS = _LOSS_ROWS + [
    (dict(totals=None, B=0), E_NULL), (dict(B=0, totals=_ODD8), E_SHAPE), (dict(totals=_ODD8), E_ALIGN), (dict(guard=_ODD4), E_ALIGN)]
_BWD = dict(g=_F, mean=_F, ldm=3, target=_F, ldt=3, log_var=_F, ldv=0, B=4, O=3, kl_scale=_K, lv_cols=_F, g_mean=_F, g_lv=_F, g_kl=None)
_BWD_ROWS = [
    (dict(g=None, O=0), E_NULL), (dict(mean=None, O=0), E_NULL), (dict(target=None, O=0), E_NULL), (dict(log_var=None, O=0), E_NULL),
    (dict(g_mean=None, O=0), E_NULL),
    (dict(lv_cols=None, O=0), E_NULL),                                                 # a shared g_lv without the forward's sums
    (dict(B=-1, g=_ODD4), E_SHAPE), (dict(O=0, ldm=0, ldt=0, g=_ODD4), E_SHAPE), (dict(O=17, ldm=17, ldt=17, g=_ODD4), E_SHAPE),
    (dict(ldm=2, g=_ODD4), E_SHAPE), (dict(ldt=2, g=_ODD4), E_SHAPE), (dict(ldv=2, g=_ODD4), E_SHAPE),
    (dict(g=_ODD4), E_ALIGN), (dict(mean=_ODD4), E_ALIGN), (dict(target=_ODD4), E_ALIGN), (dict(log_var=_ODD4), E_ALIGN),
    (dict(lv_cols=_ODD4), E_ALIGN), (dict(g_mean=_ODD4), E_ALIGN), (dict(g_lv=_ODD4), E_ALIGN), (dict(g_kl=_ODD4), E_ALIGN),
]
_RETURN_CODES = {"lbbnn_elbo_gaussian_loss": (_LOSS, _LOSS_ROWS), "lbbnn_elbo_gaussian_loss_monitor": (_MON, _MON_ROWS),
                 "lbbnn_elbo_gaussian_loss_backward": (_BWD, _BWD_ROWS)}


@pytest.mark.parametrize("name", sorted(_RETURN_CODES))
def test_loss_entry_points_early_return_codes(lib, name):
    base, rows = _RETURN_CODES[name]
    for change, code in rows:
        assert not set(change) - set(base), change
        args = dict(base, **change)
        assert getattr(lib, name)(*args.values(), None) == code, (name, change)


def _reg_args(**kw):
    from bnn_amd import _lib
    a = _lib.EvalRegressionArgs()
    base = dict(out=4096, m_stride=16, ldp=3, log_var=4096, S=2, B=4, O=3, pit_bins=20)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return a


def test_eval_regression_early_return_codes(lib):
    call = lambda **kw: lib.lbbnn_eval_regression(ctypes.byref(_reg_args(**kw)), None)
    tot = dict(counts=4096, sums=4096, pit_hist=4096, work=4096)
    assert lib.lbbnn_eval_regression(None, None) == E_NULL
    assert call(out=None, S=0) == E_NULL and call(log_var=None, S=0) == E_NULL
    for k in tot:                                                                      # some but not all of the totals
        assert call(**dict(tot, **{k: None}), S=0) == E_NULL, k
    assert call(counts=4096, S=0) == E_NULL
    assert call(S=0, out=4098) == E_SHAPE and call(S=65536, out=4098) == E_SHAPE
    assert call(O=0, ldp=0, out=4098) == E_SHAPE and call(O=17, ldp=17, m_stride=80, out=4098) == E_SHAPE
    assert call(B=-1, out=4098) == E_SHAPE
    assert call(ldp=2, out=4098) == E_SHAPE
    assert call(mean_out=4096, ldm=2, out=4098) == E_SHAPE and call(target=4096, ldt=2, out=4098) == E_SHAPE
    assert call(m_stride=11, out=4098) == E_SHAPE                                      # (B - 1) * ldp + O = 12
    assert call(B=1 << 30, m_stride=1 << 40, out=4098) == E_SHAPE
    assert call(**tot, pit_bins=0, out=4098) == E_SHAPE and call(**tot, pit_bins=1025, out=4098) == E_SHAPE
    assert call(pit_bins=0, B=0) == 0                                                  # pit_bins matters with totals only
    for k in ("out", "mean_out", "target", "log_var", "pred_mean", "epistemic_var", "aleatoric_var", "total_std", "sq_err",
              "log_density", "pit"):
        extra = dict(ldm=3) if k == "mean_out" else dict(ldt=3) if k == "target" else {}
        assert call(**{k: 4098}, **extra) == E_ALIGN, k
    for k in tot:
        assert call(**dict(tot, **{k: 4100})) == E_ALIGN, k
    assert call(B=0, m_stride=0) == 0 and call(**tot, B=0) == 0                        # an empty batch: a successful no-op
    wb = lib.lbbnn_eval_regression_work_bytes
    assert wb(10, 0, 1) == 8 * 8 and wb(10, 256, 1) == 8 * 8 and wb(10, 257, 1) == 2 * 8 * 8 and wb(3, 257, 5) == 6 * 8 * 8
    assert wb(10, 4, 0) == 0 and wb(10, 4, 17) == 0 and wb(10, -1, 1) == 0


def test_ctypes_struct_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                   'printf("%%zu %%zu %%zu\\n", sizeof(lbbnn_eval_regression_args_t), offsetof(lbbnn_eval_regression_args_t, pit_bins),'
                   ' offsetof(lbbnn_eval_regression_args_t, counts));\nreturn 0; }\n' % os.path.join(ROOT, "include", "lbbnn.h"))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, last, counts = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    cls = _lib.EvalRegressionArgs
    assert (ctypes.sizeof(cls), cls.pit_bins.offset, cls.counts.offset) == (size, last, counts)
    assert _lib.REG_COUNTS == len(_lib.REG_COUNT_NAMES) == 5 and _lib.REG_SUMS == len(_lib.REG_SUM_NAMES) == 8


# ------------------------------------------------------------------------------------------- host arithmetic
def test_train_monitor_result_reads_as_one_sigma_coverage(bnn):
    from bnn_amd import _lib
    mon = bnn.TrainMonitor(2, "cpu")
    h = np.zeros(_lib.MONITOR_WORDS, np.int64)
    h[:_lib.MONITOR_COUNTS] = [3, 60, 40, 2, 1, 1, 1, 38]      # steps rows correct bad nonfinite_rows nonfinite_steps skipped nll_rows
    h[_lib.MONITOR_COUNTS:] = np.array([57.0, 1.5, 58.5, 20.0, float("inf")]).view(np.int64)
    mon._totals.copy_(torch.from_numpy(h))
    with pytest.raises(IndexError):
        mon.result()
    r = mon.result(strict=False)
    assert r["accuracy"] == 40 / 58 and r["nll_mean"] == 57.0 / 38 and r["loss_mean"] == 58.5 / 2 and r["last_loss"] == float("inf")


def test_regression_accumulator_result_and_coverage_from_hand_filled_totals(bnn):
    from bnn_amd import _lib
    ev = bnn.evaluate
    acc = ev.RegressionAccumulator(2, 5, "cpu", -1.0, pit_bins=20)
    assert acc._log_var.tolist() == [-1.0, -1.0]
    hist = np.arange(20, dtype=np.int64)                         # 190 scored elements
    h = np.zeros(_lib.REG_COUNTS + _lib.REG_SUMS + 20, np.int64)
    h[:5] = [200, 194, 2, 6, 190]
    sums = np.array([47.5, 76.0, -133.0, 9.7, 58.2, 19.0, 401.9, 95.0])
    h[5:13] = sums.view(np.int64)
    h[13:] = hist
    acc._totals.copy_(torch.from_numpy(h))
    with pytest.raises(IndexError, match="2 target"):
        acc.result()
    r = acc.result(strict=False)
    assert (r["elements"], r["elements_with_target"], r["bad_targets"], r["nonfinite_elements"], r["scored_elements"]) == \
        (200, 194, 2, 6, 190)
    assert r["rmse"] == math.sqrt(47.5 / 190) and r["mae"] == 76.0 / 190 and r["mean_log_density"] == -133.0 / 190
    assert r["r2"] == 1.0 - 47.5 / (401.9 - 19.0 ** 2 / 190)
    assert r["mean_epistemic_var"] == 9.7 / 194 and r["mean_total_var"] == 58.2 / 194
    assert r["rmse_posterior_mean"] is None                      # no update carried posterior-mean outputs
    acc.posterior_mean_updates = 1
    assert acc.result(strict=False)["rmse_posterior_mean"] == math.sqrt(95.0 / 190)
    assert np.array_equal(r["pit_hist"], hist)
    cov = r["coverage"]
    assert cov(0.5) == hist[5:15].sum() / 190 and cov(0.8) == hist[2:18].sum() / 190 and cov(0.9) == hist[1:19].sum() / 190
    assert cov(1.0) == 1.0
    for level in (0.77, 0.95 + 1e-6, 0.25):
        with pytest.raises(ValueError, match="bin edges"):
            cov(level)
    with pytest.raises(ValueError, match="level"):
        cov(0.0)
    assert math.isnan(ev.pit_coverage(np.zeros(20, np.int64), 0.5))
    empty = ev.RegressionAccumulator(1, 1, "cpu", torch.zeros(1)).result()
    assert math.isnan(empty["rmse"]) and math.isnan(empty["r2"]) and math.isnan(empty["mean_total_var"])


def test_regression_accumulator_constructor_refusals(bnn):
    ev = bnn.evaluate
    for kw, what in ((dict(units=0), "units"), (dict(units=17), "units"), (dict(samples=0), "members"),
                     (dict(pit_bins=0), "PIT"), (dict(pit_bins=1025), "PIT")):
        args = dict(dict(units=1, samples=2, device="cpu", log_var=0.0), **kw)
        with pytest.raises(ValueError, match=what):
            ev.RegressionAccumulator(**args)
    for lv in ("0", None, True, torch.zeros(2), torch.zeros(1, dtype=torch.float64), torch.zeros(1, device="meta")):
        with pytest.raises(ValueError, match="log_var"):
            ev.RegressionAccumulator(1, 2, "cpu", lv)
    acc = ev.RegressionAccumulator(3, 2, "cpu", 0.0)
    with pytest.raises(RuntimeError, match="HIP"):
        acc.update(torch.zeros(2, 4, 3), torch.zeros(4, 3))                            # there is no CPU path
    with pytest.raises(RuntimeError, match="HIP"):
        ev.ensemble_regression(torch.zeros(2, 4, 3), None, 0.0)
