"""CPU tier of the uncertainty metrics (include/lbbnn.h lbbnn_eval_uncertainty; evaluate.ensemble_uncertainty /
UncertaintyAccumulator / ood_auroc): the numpy restatement tests/eval_uncertainty_ref.py against independent torch-float64
expressions, the AUROC interval against a brute-force pairwise AUROC, ``UncertaintyAccumulator.result`` on a hand-filled totals
buffer, the argument checks that return before any launch, and the ctypes mirror of the argument struct against gcc."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import eval_uncertainty_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


# ----------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("S,B,C,scale", [(1, 5, 3, 1.0), (4, 33, 10, 3.0), (10, 17, 64, 20.0), (3, 8, 2, 0.1)])
def test_restatement_equals_torch_float64_expressions(S, B, C, scale):
    g = torch.Generator().manual_seed(S * 100 + C)
    l = torch.log_softmax(scale * torch.randn(S, B, C, generator=g, dtype=torch.float64), -1)
    t = torch.randint(0, C, (B,), generator=g)
    r = ref.rows64(l.numpy(), t.numpy())
    p = l.exp()
    pb = p.mean(0)
    total = torch.special.entr(pb).sum(-1)
    expected = torch.special.entr(p).sum(-1).mean(0)
    idx = torch.arange(B)
    want = {"bma_probs": pb, "total_entropy": total, "expected_entropy": expected,
            "mutual_information": (total - expected).clamp_min(0.0), "confidence": pb.max(-1).values,
            "brier": ((pb - torch.nn.functional.one_hot(t, C)) ** 2).sum(-1),
            "log_score": -(torch.logsumexp(l[:, idx, t], 0) - math.log(S))}
    for k, w in want.items():
        assert np.allclose(r[k], w.numpy(), rtol=1e-12, atol=1e-13), k
    # the log score is that of the model average, and it survives where -log(pbar) would not
    assert np.allclose(r["log_score"], -np.log(pb[idx, t].numpy()), rtol=1e-9)
    low = np.full((2, 1, 3), -800.0)
    low[:, 0, 1] = -1e-300
    assert np.isfinite(ref.rows64(low, np.array([0]))["log_score"][0]) and np.exp(-800.0) == 0.0
    # a -inf entry is a zero term, rows without a valid target carry NaN scores
    l2 = l.numpy().copy()
    l2[0, 0, 0] = -np.inf
    r2 = ref.rows64(l2, np.array([-1] + [0] * (B - 1)))
    assert np.isfinite(r2["total_entropy"][0]) and np.isfinite(r2["expected_entropy"][0])
    assert np.isnan(r2["brier"][0]) and np.isnan(r2["log_score"][0]) and np.isfinite(r2["brier"][1:]).all()


def test_bin_index_and_totals_on_a_hand_worked_case():
    f = np.float32
    assert ref.bin_index(f([0.0, 0.049, 0.05, 0.5, 0.999, 1.0, 1.0000001, -0.1]), 20, 20).tolist() == [0, 0, 1, 10, 19, 19, 19, 0]
    assert ref.bin_index(f([3.0e38]), 100, 100).tolist() == [99]               # the product overflows: the last bin
    assert ref.mutual_information(f([1.0, 0.5, np.nan]), f([0.25, 0.75, 0.0])).tolist()[:2] == [0.75, 0.0]
    assert np.isnan(ref.mutual_information(f([np.nan]), f([0.0]))[0])
    rows = {"confidence": f([0.9, 0.6, np.nan, 0.3, 0.6]), "total_entropy": f([0.2, 0.6, np.nan, 1.0, 0.6]),
            "expected_entropy": f([0.1, 0.6, np.nan, 0.5, 0.5]), "mutual_information": f([0.1, 0.0, np.nan, 0.5, 0.1]),
            "brier": f([0.1, 0.7, np.nan, 1.2, np.nan]), "log_score": f([0.1, np.inf, np.nan, 1.5, np.nan]),
            "pred_bma": np.array([1, 0, 0, 2, 1])}
    r = ref.totals(rows, np.array([1, 2, 0, 2, 7]), C=3, M=4, K=8)
    assert [r[k] for k in ref.COUNT_NAMES] == [5, 4, 1, 3, 1, 1]
    assert r["bin_rows"].tolist() == [0, 1, 2, 1] and r["bin_rows_with_target"].tolist() == [0, 1, 1, 1]
    assert r["bin_correct"].tolist() == [0, 1, 0, 1]
    assert r["hist"].sum(1).tolist() == [4, 4, 4] and r["hist"][2].tolist() == [1, 0, 0, 2, 0, 1, 0, 0]
    assert r["terms"]["brier"].size == 3 and r["terms"]["log_score"].size == 2 and r["terms"]["confidence"].size == 4
    assert [x.size for x in r["bin_conf_terms"]] == [0, 1, 1, 1]
    c = ref.calibration(r["bin_rows_with_target"], r["bin_correct"], [0.0, f(0.3), f(0.6), f(0.9)])
    want = (abs(1 - float(f(0.3))) + abs(0 - float(f(0.6))) + abs(1 - float(f(0.9)))) / 3
    assert abs(c["ece"] - want) < 1e-15 and abs(c["mce"] - abs(1 - float(f(0.3)))) < 1e-15
    assert c["coverage"].tolist() == [1.0, 1.0, 2 / 3, 1 / 3] and c["accuracy"].tolist() == [2 / 3, 2 / 3, 0.5, 1.0]


# ----------------------------------------------------------------------------------- 2. the AUROC interval
def _fake_result(scores, C, K):
    """A result dict carrying nothing but what ood_auroc reads: the histogram of fp32 scores, binned as the kernel bins them."""
    h = {k: {"counts": np.bincount(ref.bin_index(scores, ref.ent_scale(C, K) if k != "max_prob" else K, K), minlength=K)}
         for k in ref.SCORES}
    return {"classes": C, "hist_bins": K, "histograms": h}


@pytest.mark.parametrize("K", (1, 7, 64, 1024))
@pytest.mark.parametrize("score", ref.SCORES)
def test_ood_auroc_interval_holds_the_pairwise_auroc(score, K):
    import bnn_amd
    ev = bnn_amd.evaluate
    rng = np.random.default_rng(K)
    C = 10
    top = math.log(C) if score != "max_prob" else 1.0
    for n_in, n_out, shift in ((200, 150, 0.3), (50, 400, 0.0), (300, 300, -0.2), (40, 40, 1.5)):
        s_in = np.clip(rng.beta(2, 5, n_in) * top, 0, top).astype(np.float32)
        s_out = np.clip((rng.beta(2, 5, n_out) + shift) * top, 0, top).astype(np.float32)
        s_out[:5] = s_in[:5]                                   # exact ties across the two passes
        auroc, hw = ev.ood_auroc(_fake_result(s_in, C, K), _fake_result(s_out, C, K), score)
        a_ref, hw_ref = ref.auroc_hist(_fake_result(s_in, C, K)["histograms"][score]["counts"],
                                       _fake_result(s_out, C, K)["histograms"][score]["counts"])
        assert abs(auroc - a_ref) < 1e-15 and abs(hw - hw_ref) < 1e-15
        exact = ref.auroc_pairs(s_in, s_out)
        assert auroc - hw - 1e-12 <= exact <= auroc + hw + 1e-12, (score, K, exact, auroc, hw)
        assert 0.0 <= hw <= 0.5
        if K == 1:
            assert auroc == 0.5 and hw == 0.5                 # one bin says nothing, and says so
    with pytest.raises(ValueError):
        ev.ood_auroc(_fake_result(s_in, C, K), _fake_result(s_out, C, K + 1), score)
    with pytest.raises(ValueError):
        ev.ood_auroc(_fake_result(s_in, C, K), _fake_result(s_out, C + 1, K), score)
    with pytest.raises(ValueError):
        ev.ood_auroc(_fake_result(s_in, C, K), _fake_result(s_out, C, K), "entropy")


# ----------------------------------------------------------------------------------- 3. the accumulator
def test_result_reads_a_hand_filled_totals_buffer():
    import bnn_amd
    from bnn_amd import _lib
    ev = bnn_amd.evaluate
    C, S, M, K = 3, 2, 4, 8
    u = ev.UncertaintyAccumulator(C, S, "cpu", conf_bins=M, hist_bins=K)
    off = u._offsets()
    assert [off[k] for k in ("counts", "sums", "bin_rows", "bin_rows_with_target", "bin_correct", "bin_conf_sum", "hist", "end")] \
        == [0, 6, 12, 16, 20, 24, 28, 52]
    assert u._totals.numel() == 52 and u._totals.dtype == torch.int64 and float(u.ent_scale) == float(np.float32(K / math.log(C)))
    assert tuple(_lib.UNC_COUNT_NAMES) == ref.COUNT_NAMES and tuple(_lib.UNC_SUM_NAMES) == ref.SUM_NAMES
    assert tuple(ev.OOD_SCORES) == ref.SCORES
    h = np.zeros(52, dtype=np.int64)
    h[0:6] = (12, 10, 1, 7, 2, 1)                              # 10 finite rows, 8 of them with a target
    h[6:12] = np.array([5.0, 3.0, 2.0, 7.5, 4.0, 14.0]).view(np.int64)
    h[12:16] = (0, 3, 2, 5)
    h[16:20] = (0, 2, 2, 4)
    h[20:24] = (0, 1, 1, 4)
    h[24:28] = np.array([0.0, 0.75, 1.25, 3.5]).view(np.int64)
    h[28:52] = np.arange(24)
    u._read = lambda: h                                       # the stubbed totals buffer: no device
    with pytest.raises(IndexError, match="1 target"):
        u.result()
    r = u.result(strict=False)
    assert [r[k] for k in _lib.UNC_COUNT_NAMES] == [12, 10, 1, 7, 2, 1] and all(type(r[k]) is int for k in _lib.UNC_COUNT_NAMES)
    assert [r[k + "_sum"] for k in _lib.UNC_SUM_NAMES] == [5.0, 3.0, 2.0, 7.5, 4.0, 14.0]
    assert [r[k + "_mean"] for k in _lib.UNC_SUM_NAMES] == [0.5, 0.3, 0.2, 0.75, 0.5, 2.0]       # / 10, / 8, / (8 - 1)
    assert r["accuracy_bma"] == 0.7
    c = ref.calibration(h[16:20], h[20:24], [0.0, 0.75, 1.25, 3.5])
    assert r["ece"] == pytest.approx(c["ece"], abs=1e-15) and r["mce"] == pytest.approx(c["mce"], abs=1e-15)
    assert r["ece"] == pytest.approx((2 * abs(0.5 - 0.375) + 2 * abs(0.5 - 0.625) + 4 * abs(1.0 - 0.875)) / 8)
    assert r["mce"] == pytest.approx(0.125)
    rel = r["reliability"]
    assert rel["edges"].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0] and rel["rows"].tolist() == [0, 3, 2, 5]
    assert np.isnan(rel["accuracy"][0]) and rel["accuracy"][1:].tolist() == [0.5, 0.5, 1.0]
    assert rel["confidence"][1:].tolist() == [0.375, 0.625, 0.875]
    sel = r["selective"]
    assert sel["threshold"].tolist() == [0.0, 0.25, 0.5, 0.75]
    assert np.allclose(sel["coverage"], c["coverage"]) and sel["coverage"].tolist() == [1.0, 1.0, 0.75, 0.5]
    assert np.allclose(sel["accuracy"], c["accuracy"]) and sel["accuracy"].tolist() == [0.75, 0.75, 5 / 6, 1.0]
    hs = r["histograms"]
    assert hs["total_entropy"]["counts"].tolist() == list(range(8)) and hs["max_prob"]["counts"].tolist() == list(range(16, 24))
    assert hs["mutual_information"]["edges"][-1] == pytest.approx(math.log(3)) and hs["max_prob"]["edges"].tolist()[1] == 0.125
    assert (r["classes"], r["samples"], r["conf_bins"], r["hist_bins"]) == (3, 2, 4, 8)
    # an untouched accumulator: zeros and NaN means, no division error
    z = ev.UncertaintyAccumulator(C, S, "cpu").result()
    assert z["rows"] == 0 and np.isnan(z["ece"]) and np.isnan(z["mce"]) and np.isnan(z["brier_mean"]) and np.isnan(z["accuracy_bma"])
    assert z["bin_rows"].shape == (20,) and z["histograms"]["max_prob"]["counts"].shape == (1024,)
    assert ev.UncertaintyAccumulator(1, 1, "cpu").ent_scale == 0.0
    for bad in (dict(classes=65), dict(classes=0), dict(samples=0), dict(conf_bins=0), dict(conf_bins=101), dict(hist_bins=0),
                dict(hist_bins=4097)):
        with pytest.raises(ValueError):
            ev.UncertaintyAccumulator(**{**dict(classes=4, samples=3, device="cpu"), **bad})


def test_cpu_tensors_raise():
    import bnn_amd
    ev = bnn_amd.evaluate
    out = torch.log_softmax(torch.randn(3, 5, 4), -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.ensemble_uncertainty(out)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.UncertaintyAccumulator(4, 3, "cpu").update(out, torch.zeros(5, dtype=torch.long))
    with pytest.raises(ValueError):
        ev.ensemble_uncertainty(out[0])


# ----------------------------------------------------------------------------------- 4. the C ABI
def _args(**kw):
    from bnn_amd import _lib
    a = _lib.EvalUncertaintyArgs()
    base = dict(logp=4096, m_stride=1000, ldp=10, S=10, B=100, C=10, conf_bins=20, hist_bins=1024, ent_scale=444.0)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return a


TOTALS = dict(counts=4096, sums=4096, bin_rows=4096, bin_rows_with_target=4096, bin_correct=4096, bin_conf_sum=4096, hist=4096,
              work=4096)
ROWS_F32 = ("bma_probs", "confidence", "total_entropy", "expected_entropy", "mutual_information", "brier", "log_score")


def test_argument_checks_return_codes_without_launching(lib):
    call = lambda **kw: lib.lbbnn_eval_uncertainty(ctypes.byref(_args(**kw)), None)
    assert lib.lbbnn_eval_uncertainty(None, None) == -1
    assert call(logp=None) == -1
    for k in TOTALS:
        assert call(**{**TOTALS, k: None}) == -1, k                       # all or none, and never without work memory
        if k != "work":
            assert call(**{k: 4096}) == -1, k
    for kw in (dict(S=0), dict(S=65536), dict(C=0), dict(C=65), dict(B=-1), dict(ldp=9), dict(m_stride=999)):
        assert call(**kw) == -2, kw
        assert call(**TOTALS, **kw) == -2, kw
    for kw in (dict(conf_bins=0), dict(conf_bins=101), dict(hist_bins=0), dict(hist_bins=4097), dict(ent_scale=-1.0),
               dict(ent_scale=float("nan")), dict(ent_scale=float("inf"))):
        assert call(**TOTALS, **kw) == -2, kw
    assert call(m_stride=0, S=1, B=0) == 0                                 # B == 0: a successful no-op
    assert call(B=0) == 0 and call(B=0, **TOTALS) == 0
    for k in ("logp",) + ROWS_F32:
        assert call(**{k: 4098}) == -3, k
    for k in ("target", "pred_bma"):
        assert call(**{k: 4100}) == -3, k
    for k in TOTALS:
        assert call(**{**TOTALS, k: 4100}) == -3, k


def test_work_bytes_is_monotone_and_non_zero(lib):
    for C in (1, 2, 10, 16, 17, 64):
        prev = 0
        for B in (0, 1, 63, 64, 65, 100, 1000, 4096, 1 << 20):
            w = lib.lbbnn_eval_uncertainty_work_bytes(10, B, C, 20)
            assert w > 0 and w % 8 == 0 and w >= prev, (B, C, w)
            prev = w
        assert lib.lbbnn_eval_uncertainty_work_bytes(10, 4096, C, 100) > lib.lbbnn_eval_uncertainty_work_bytes(10, 4096, C, 1)
    for bad in ((10, 100, 65, 20), (10, -1, 10, 20), (10, 100, 10, 0), (10, 100, 10, 101)):
        assert lib.lbbnn_eval_uncertainty_work_bytes(*bad) == 0, bad


def test_struct_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    fields = [n for n, _ in _lib.EvalUncertaintyArgs._fields_]
    src = tmp_path / "sizes.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"),
             "int main(void) {", 'printf("%zu %d %d\\n", sizeof(lbbnn_eval_uncertainty_args_t), LBBNN_UNC_COUNTS, LBBNN_UNC_SUMS);']
    lines += ['printf("%%zu\\n", offsetof(lbbnn_eval_uncertainty_args_t, %s));' % n for n in fields]
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    size, counts, sums = map(int, out[:3])
    assert ctypes.sizeof(_lib.EvalUncertaintyArgs) == size
    assert [getattr(_lib.EvalUncertaintyArgs, n).offset for n in fields] == list(map(int, out[3:]))
    assert _lib.UNC_COUNTS == counts == len(_lib.UNC_COUNT_NAMES) and _lib.UNC_SUMS == sums == len(_lib.UNC_SUM_NAMES)
    for n in ("lbbnn_eval_uncertainty", "lbbnn_eval_uncertainty_work_bytes"):
        assert n in _lib.SIGNATURES, n
