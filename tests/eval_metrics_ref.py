"""numpy restatement of what lbbnn_eval_metrics computes (include/lbbnn.h) -- the numbers of the reference's evaluation
loops: test_ensemble (LBBNN-GP-MF-MNF.py:312-323: the mean over the members, its argmax, the posterior-mean argmax, the two
correct counts), outofsample (:370-392: per member sigmoid / row sum, the member mean, -sum p log p, per-member and ensemble
correct counts) and variational dropout's validation (variational_dropout.py:160-176: the member mean, nll_loss(sum), the
correct count, confusion[target][prediction]).

The mean uses the order the header states, in np.float32 arithmetic (IEEE add and divide: the kernel's bits); predictions are
np.argmax (a NaN is the maximum, the lowest index wins a tie); the entropy and the sums are float64."""
import numpy as np

COUNT_NAMES = ("rows", "rows_with_target", "bad_targets", "correct_ensemble", "correct_posterior_mean", "entropy_nonfinite")


def ensemble_mean(outputs: np.ndarray) -> np.ndarray:
    """acc = logp[0]; acc += logp[m] for m ascending, in fp32; then acc / (float)S."""
    o = np.asarray(outputs, dtype=np.float32)
    S = o.shape[0]
    with np.errstate(all="ignore"):
        acc = o[0].copy()
        for m in range(1, S):
            acc = (acc + o[m]).astype(np.float32)
        return (acc / np.float32(S)).astype(np.float32)


def argmax_rows(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a)
    if a.shape[0] == 0:
        return np.zeros((0,), dtype=np.int64)
    return np.argmax(a, axis=-1).astype(np.int64)


def entropy64(outputs: np.ndarray) -> np.ndarray:
    """outofsample's predictive entropy (the expression of evaluate.predictive_entropy) in float64."""
    o = np.asarray(outputs, dtype=np.float64)
    with np.errstate(all="ignore"):
        p = 1.0 / (1.0 + np.exp(-o))
        p = p / p.sum(-1, keepdims=True)
        m = p.mean(0)
        return -(m * np.log(m)).sum(-1)


def metrics(outputs, target=None, mean_outputs=None) -> dict:
    """Everything one lbbnn_eval_metrics call reports for one batch, totals as if they had been zero before."""
    o = np.asarray(outputs, dtype=np.float32)
    S, B, C = o.shape
    mean = ensemble_mean(o)
    pred = argmax_rows(mean)
    ent = entropy64(o)
    res = {"mean_log_probs": mean, "pred_ensemble": pred, "entropy": ent}
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["rows"] = B
    counts["entropy_nonfinite"] = int((~np.isfinite(ent)).sum())
    member = np.zeros(S, dtype=np.int64)
    conf = np.zeros((C, C), dtype=np.int64)
    nll_terms = np.zeros(0, dtype=np.float64)
    pm = None
    if mean_outputs is not None:
        pm = argmax_rows(np.asarray(mean_outputs, dtype=np.float32))
        res["pred_posterior_mean"] = pm
    if target is not None:
        t = np.asarray(target, dtype=np.int64)
        ok = (t >= 0) & (t < C)
        counts["rows_with_target"] = int(ok.sum())
        counts["bad_targets"] = int((~ok).sum())
        tv = t[ok]
        counts["correct_ensemble"] = int((pred[ok] == tv).sum())
        if pm is not None:
            counts["correct_posterior_mean"] = int((pm[ok] == tv).sum())
        for m in range(S):
            member[m] = int((argmax_rows(o[m])[ok] == tv).sum())
        np.add.at(conf, (tv, pred[ok]), 1)                    # rows: the true labels
        nll_terms = -mean[ok, tv].astype(np.float64)          # exact fp32 values, summed in double
    res.update(counts)
    res["correct_member"], res["confusion"], res["nll_terms"] = member, conf, nll_terms
    with np.errstate(all="ignore"):
        res["nll_sum"] = float(nll_terms.sum()) if nll_terms.size else 0.0
    return res


def add_totals(parts) -> dict:
    """The totals of several batches (what consecutive calls accumulate)."""
    out = {k: sum(p[k] for p in parts) for k in COUNT_NAMES}
    out["correct_member"] = sum(p["correct_member"] for p in parts)
    out["confusion"] = sum(p["confusion"] for p in parts)
    out["nll_terms"] = np.concatenate([p["nll_terms"] for p in parts])
    with np.errstate(all="ignore"):
        out["nll_sum"] = float(out["nll_terms"].sum()) if out["nll_terms"].size else 0.0
    return out
