"""CPU tier of the evaluation metrics (include/lbbnn.h lbbnn_eval_metrics; evaluate.ensemble_metrics / EvalAccumulator):
argument checks that return before any launch, the ctypes mirror of the argument struct against gcc, the work-memory helper,
the no-CPU-path rule and ``EvalAccumulator.result`` on a stubbed totals buffer; plus the numpy restatement against a
hand-worked case."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import eval_metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def _args(**kw):
    from bnn_amd import _lib
    a = _lib.EvalMetricsArgs()
    base = dict(logp=4096, m_stride=1000, ldp=10, S=10, B=100, C=10)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return a


TOTALS = dict(counts=4096, correct_member=4096, confusion=4096, sums=4096, work=4096)


def test_argument_checks_return_codes_without_launching(lib):
    call = lambda **kw: lib.lbbnn_eval_metrics(ctypes.byref(_args(**kw)), None)
    assert lib.lbbnn_eval_metrics(None, None) == -1
    assert call(logp=None) == -1
    for k in ("counts", "correct_member", "confusion", "sums"):           # all or none
        assert call(**{**TOTALS, k: None}) == -1, k
        assert call(**{k: 4096}) == -1, k
    assert call(**{**TOTALS, "work": None}) == -1                          # totals without work memory
    assert call(pred_mean=4096) == -1                                      # no mean_logp to take the argmax of
    for kw in (dict(S=0), dict(S=65536), dict(C=0), dict(C=65), dict(B=-1), dict(ldp=9), dict(m_stride=999),
               dict(mean_logp=4096, ldm=9)):
        assert call(**kw) == -2, kw
    assert call(m_stride=0, S=1, B=0) == 0                                 # B == 0: a successful no-op
    assert call(B=0) == 0 and call(B=0, **TOTALS) == 0
    for k in ("logp", "mean_logp", "ens_logp", "entropy"):
        assert call(**{"ldm": 10, k: 4098}) == -3, k
    for k in ("target", "pred_ensemble"):
        assert call(**{k: 4100}) == -3, k
    assert call(mean_logp=4096, ldm=10, pred_mean=4100) == -3
    for k in TOTALS:
        assert call(**{**TOTALS, k: 4100}) == -3, k


def test_struct_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                   'printf("%%zu %%zu %%zu %%d\\n", sizeof(lbbnn_eval_metrics_args_t), offsetof(lbbnn_eval_metrics_args_t, C), '
                   'offsetof(lbbnn_eval_metrics_args_t, work), LBBNN_EVAL_COUNTS);\nreturn 0; }\n'
                   % os.path.join(ROOT, "include", "lbbnn.h"))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, off_c, off_work, counts = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(_lib.EvalMetricsArgs) == size
    assert _lib.EvalMetricsArgs.C.offset == off_c and _lib.EvalMetricsArgs.work.offset == off_work
    assert _lib.EVAL_COUNTS == counts == len(_lib.EVAL_COUNT_NAMES) == len(ref.COUNT_NAMES)
    assert tuple(_lib.EVAL_COUNT_NAMES) == tuple(ref.COUNT_NAMES)


def test_work_bytes_is_monotone_and_non_zero(lib):
    for C in (1, 2, 10, 16, 17, 64):
        prev = 0
        for B in (0, 1, 63, 64, 65, 100, 1000, 4096, 1 << 20):
            w = lib.lbbnn_eval_metrics_work_bytes(10, B, C)
            assert w > 0 and w % 8 == 0 and w >= prev, (B, C, w)
            prev = w
        assert lib.lbbnn_eval_metrics_work_bytes(100, 4096, C) == lib.lbbnn_eval_metrics_work_bytes(1, 4096, C)
    assert lib.lbbnn_eval_metrics_work_bytes(10, 4096, 64) >= lib.lbbnn_eval_metrics_work_bytes(10, 4096, 10)
    assert lib.lbbnn_eval_metrics_work_bytes(10, 100, 65) == 0 and lib.lbbnn_eval_metrics_work_bytes(10, -1, 10) == 0


def test_cpu_tensors_raise():
    import bnn_amd
    ev = bnn_amd.evaluate
    out = torch.log_softmax(torch.randn(3, 5, 4), -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.ensemble_metrics(out)
    acc = ev.EvalAccumulator(4, 3, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        acc.update(out, torch.zeros(5, dtype=torch.long))
    with pytest.raises(ValueError):
        ev.ensemble_metrics(out[0])
    with pytest.raises(ValueError):
        ev.EvalAccumulator(65, 3, "cpu")
    with pytest.raises(ValueError):
        ev.EvalAccumulator(4, 0, "cpu")


def test_result_reads_the_totals_and_is_strict_about_bad_targets():
    import bnn_amd
    from bnn_amd import _lib
    ev = bnn_amd.evaluate
    C, S = 3, 2
    acc = ev.EvalAccumulator(C, S, "cpu")
    n = _lib.EVAL_COUNTS
    h = np.zeros(n + S + C * C + 2, dtype=np.int64)
    h[:n] = (12, 10, 2, 7, 5, 1)
    h[n:n + S] = (6, 4)
    h[n + S:n + S + C * C] = np.arange(9)
    h[n + S + C * C:] = np.array([20.5, 5.5]).view(np.int64)
    acc._read = lambda: h                                     # the stubbed totals buffer: no device
    with pytest.raises(IndexError, match="2 target"):
        acc.result()
    with pytest.raises(IndexError):
        acc.result(strict=True)
    r = acc.result(strict=False)
    assert [r[k] for k in _lib.EVAL_COUNT_NAMES] == [12, 10, 2, 7, 5, 1]
    assert all(type(r[k]) is int for k in _lib.EVAL_COUNT_NAMES)
    assert r["correct_member"].tolist() == [6, 4] and r["confusion"].tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert r["nll_sum"] == 20.5 and r["entropy_sum"] == 5.5
    assert r["accuracy_ensemble"] == 0.7 and r["nll_mean"] == 2.05 and r["entropy_mean"] == 0.5
    assert r["accuracy_posterior_mean"] is None              # no update carried posterior-mean outputs
    acc.posterior_mean_updates = 1
    assert acc.result(strict=False)["accuracy_posterior_mean"] == 0.5
    h[2] = 0
    assert acc.result()["bad_targets"] == 0                   # strict, and nothing to object to
    # an untouched accumulator: zeros, NaN means, no division error
    z = ev.EvalAccumulator(C, S, "cpu").result()
    assert z["rows"] == 0 and np.isnan(z["accuracy_ensemble"]) and np.isnan(z["entropy_mean"]) and z["nll_sum"] == 0.0
    assert int(z["confusion"].sum()) == 0


def test_restatement_on_a_hand_worked_case():
    """Ties go to the lowest index, a NaN is the maximum, bad targets are left out; the fp32 mean in the stated order."""
    o = np.log(np.array([[[0.5, 0.25, 0.25], [0.2, 0.4, 0.4], [0.1, 0.1, 0.8]],
                         [[0.5, 0.25, 0.25], [0.2, 0.4, 0.4], [0.1, 0.1, 0.8]]], dtype=np.float32))
    o[1, 2, 1] = np.nan
    r = ref.metrics(o, np.array([0, 2, 5]), mean_outputs=o[0])
    assert r["pred_ensemble"].tolist() == [0, 1, 1] and r["pred_posterior_mean"].tolist() == [0, 1, 2]
    assert (r["rows"], r["rows_with_target"], r["bad_targets"], r["correct_ensemble"], r["correct_posterior_mean"]) == (3, 2, 1, 1, 1)
    assert r["entropy_nonfinite"] == 1 and r["correct_member"].tolist() == [1, 1]
    assert r["confusion"].tolist() == [[1, 0, 0], [0, 0, 0], [0, 1, 0]]
    assert np.array_equal(r["mean_log_probs"][:2], o[0, :2])                # (a + a) / 2 == a exactly
    assert abs(r["nll_sum"] - (-np.log(0.5) - np.log(0.4))) < 1e-6
    e = ref.entropy64(o[:, :1])
    s = 1 / (1 + np.exp(-np.log([0.5, 0.25, 0.25])))
    p = s / s.sum()
    assert abs(e[0] + (p * np.log(p)).sum()) < 1e-7
