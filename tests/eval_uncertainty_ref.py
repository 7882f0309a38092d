"""numpy restatement of lbbnn_eval_uncertainty (include/lbbnn.h) with two faces.

1. ``rows64``: the per-row numbers in float64 from the input log-probabilities -- the standard definitions: the Bayesian model
   average p = mean_s exp(l_s), H[p], mean_s H[p_s], their difference, max p, the Brier score, and the log score as a
   logsumexp with the maximum subtracted.
2. The exact integer logic applied to GIVEN fp32 per-row values (the kernel's own returned values, in the tests): ``bin_index``
   (one np.float32 multiplication, clamped to [0, bins] as a float, truncated, clamped to [0, bins - 1]), ``totals`` (counts,
   reliability bins, histograms, and the terms of every double sum), ``calibration`` (ECE / MCE / suffix sums from bins) and the
   two AUROCs (from histograms with in-bin ties counted 1/2; brute force over all pairs)."""
import math

import numpy as np

COUNT_NAMES = ("rows", "rows_with_target", "bad_targets", "correct_bma", "nonfinite_rows", "log_score_nonfinite")
SUM_NAMES = ("total_entropy", "expected_entropy", "mutual_information", "confidence", "brier", "log_score")
SCORES = ("total_entropy", "mutual_information", "max_prob")


# ------------------------------------------------------------------------------------------------ 1. float64 from the inputs
def rows64(outputs, target=None) -> dict:
    l = np.asarray(outputs, dtype=np.float64)
    S, B, C = l.shape
    with np.errstate(all="ignore"):
        p = np.exp(l)
        pb = p.sum(0) / S
        total = -np.where(pb == 0, 0.0, pb * np.log(pb)).sum(-1)
        expected = (-np.where(p == 0, 0.0, p * l).sum(-1)).sum(0) / S
        mi = np.maximum(total - expected, 0.0)
        mi = np.where(np.isnan(total - expected), np.nan, mi)
    res = {"bma_probs": pb, "total_entropy": total, "expected_entropy": expected, "mutual_information": mi,
           "confidence": pb.max(-1) if B else np.zeros(0), "brier": np.full(B, np.nan), "log_score": np.full(B, np.nan)}
    if target is not None and B:
        t = np.asarray(target, dtype=np.int64)
        ok = (t >= 0) & (t < C)
        tv = np.where(ok, t, 0)
        onehot = np.zeros((B, C))
        onehot[np.arange(B), tv] = 1.0
        lt = l[:, np.arange(B), tv]                              # (S, B)
        with np.errstate(all="ignore"):
            mx = lt.max(0)
            safe = np.where(np.isfinite(mx), mx, 0.0)
            lse = safe + np.log(np.exp(lt - safe).sum(0))
            res["brier"] = np.where(ok, ((pb - onehot) ** 2).sum(-1), np.nan)
            res["log_score"] = np.where(ok, -(lse - math.log(S)), np.nan)
    return res


# ------------------------------------------------------------------------------------------------ 2. exact logic on fp32 values
def ent_scale(C: int, K: int) -> np.float32:
    return np.float32(K / math.log(C)) if C > 1 else np.float32(0.0)


def argmax_rows(a) -> np.ndarray:
    a = np.asarray(a)
    if a.shape[0] == 0:
        return np.zeros((0,), dtype=np.int64)
    return np.argmax(a, axis=-1).astype(np.int64)               # a NaN is the maximum, the lowest index wins


def bin_index(v, scale, n: int) -> np.ndarray:
    """clamp((int)(v * scale), 0, n - 1) of finite fp32 values: the product in fp32, clamped to [0, n] before the truncation."""
    with np.errstate(all="ignore"):
        p = (np.asarray(v, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    p = np.minimum(np.maximum(p, np.float32(0)), np.float32(n))
    return np.clip(p.astype(np.int64), 0, n - 1)


def mutual_information(total, expected) -> np.ndarray:
    with np.errstate(all="ignore"):
        d = (np.asarray(total, dtype=np.float32) - np.asarray(expected, dtype=np.float32)).astype(np.float32)
    return np.where(d < 0, np.float32(0), d).astype(np.float32)


def totals(rows: dict, target, C: int, M: int, K: int) -> dict:
    """Every total of one call from the per-row fp32 values ``rows`` (confidence, total_entropy, expected_entropy,
    mutual_information, brier, log_score, pred_bma), as if the totals had been zero before; ``terms``: per sum the float64
    values that enter it."""
    conf, tot, exp_, mi = (np.asarray(rows[k], dtype=np.float32)
                           for k in ("confidence", "total_entropy", "expected_entropy", "mutual_information"))
    pred = np.asarray(rows["pred_bma"], dtype=np.int64)
    B = conf.shape[0]
    if target is None:
        ok, t = np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int64)
    else:
        t = np.asarray(target, dtype=np.int64)
        ok = (t >= 0) & (t < C)
    fin = np.isfinite(conf) & np.isfinite(tot) & np.isfinite(exp_) & np.isfinite(mi)
    ls = np.asarray(rows["log_score"], dtype=np.float32)
    ls_fin = np.isfinite(ls)
    hit = ok & (pred == t)
    res = {"rows": B, "rows_with_target": int(ok.sum()), "bad_targets": 0 if target is None else int((~ok).sum()),
           "correct_bma": int(hit.sum()), "nonfinite_rows": int((~fin).sum()), "log_score_nonfinite": int((fin & ok & ~ls_fin).sum())}
    mb = bin_index(conf[fin], M, M)
    count = lambda idx, n: np.bincount(idx, minlength=n).astype(np.int64)
    res["bin_rows"] = count(mb, M)
    res["bin_rows_with_target"] = count(bin_index(conf[fin & ok], M, M), M)
    res["bin_correct"] = count(bin_index(conf[fin & hit], M, M), M)
    sc = ent_scale(C, K)
    one_minus = (np.float32(1) - conf[fin]).astype(np.float32)
    res["hist"] = np.stack([count(bin_index(tot[fin], sc, K), K), count(bin_index(mi[fin], sc, K), K),
                            count(bin_index(one_minus, K, K), K)])
    f64 = lambda a, mask: np.asarray(a, dtype=np.float32)[mask].astype(np.float64)
    res["terms"] = {"total_entropy": f64(tot, fin), "expected_entropy": f64(exp_, fin), "mutual_information": f64(mi, fin),
                    "confidence": f64(conf, fin), "brier": f64(rows["brier"], fin & ok), "log_score": f64(ls, fin & ok & ls_fin)}
    tconf, tbin = f64(conf, fin & ok), bin_index(conf[fin & ok], M, M)
    res["bin_conf_terms"] = [tconf[tbin == m] for m in range(M)]
    return res


def add_totals(parts) -> dict:
    out = {k: sum(p[k] for p in parts) for k in COUNT_NAMES + ("bin_rows", "bin_rows_with_target", "bin_correct", "hist")}
    out["terms"] = {k: np.concatenate([p["terms"][k] for p in parts]) for k in SUM_NAMES}
    out["bin_conf_terms"] = [np.concatenate([p["bin_conf_terms"][m] for p in parts]) for m in range(len(parts[0]["bin_conf_terms"]))]
    return out


def calibration(n_t, n_c, conf_sum) -> dict:
    """ECE, MCE and the accuracy against coverage from the reliability bins of the rows with a target."""
    n_t, n_c, conf_sum = np.asarray(n_t, dtype=np.int64), np.asarray(n_c, dtype=np.int64), np.asarray(conf_sum, dtype=np.float64)
    M, N = n_t.shape[0], int(n_t.sum())
    ece, mce = 0.0, 0.0
    for m in range(M):
        if n_t[m]:
            gap = abs(n_c[m] / n_t[m] - conf_sum[m] / n_t[m])
            ece += n_t[m] / N * gap
            mce = max(mce, gap)
    cov = [n_t[k:].sum() / N if N else float("nan") for k in range(M)]
    acc = [n_c[k:].sum() / n_t[k:].sum() if n_t[k:].sum() else float("nan") for k in range(M)]
    return {"ece": ece if N else float("nan"), "mce": mce if N else float("nan"), "coverage": np.array(cov), "accuracy": np.array(acc)}


def auroc_hist(h_in, h_out):
    """(auroc, half_width) from two histograms of the same score: pairs in the same bin count 1/2."""
    h_in, h_out = np.asarray(h_in, dtype=np.int64), np.asarray(h_out, dtype=np.int64)
    wins = ties = 0
    below = 0
    for k in range(h_in.shape[0]):
        wins += int(h_out[k]) * below
        ties += int(h_in[k]) * int(h_out[k])
        below += int(h_in[k])
    pairs = int(h_in.sum()) * int(h_out.sum())
    return (wins + 0.5 * ties) / pairs, 0.5 * ties / pairs


def auroc_pairs(s_in, s_out) -> float:
    """P(out > in) + P(out == in) / 2 over all pairs, by brute force."""
    a, b = np.asarray(s_in, dtype=np.float64)[:, None], np.asarray(s_out, dtype=np.float64)[None, :]
    return float(((b > a).sum() + 0.5 * (b == a).sum()) / (a.shape[0] * b.shape[1]))
