"""numpy float64 restatement of what lbbnn_elbo_loss_monitor keeps in a TrainMonitor (include/lbbnn.h): the
counts, the three sums over the steps whose loss is finite and the two values of the last step.

Predictions are np.argmax (a NaN is the maximum, the lowest index wins a tie) and count only for rows with a valid target;
``loss`` is the fp32 number the kernel writes, (float32)(nll + kl * kl_scale) with the sums in float64, and "finite" is said
of that fp32 number.  Every step also reports the absolute values of the terms its sums are made of, for the worst-case
rounding bound of the tests."""
import numpy as np

COUNT_NAMES = ("steps", "rows", "correct", "bad_targets", "nonfinite_rows", "nonfinite_steps", "skipped_steps", "nll_rows")
SUM_NAMES = ("nll_sum", "kl_term_sum", "loss_sum")


def step(log_probs, target, kl=None, kl_scale=1.0) -> dict:
    """One call: its own numbers (not yet totals)."""
    lp = np.asarray(log_probs, dtype=np.float32)
    t = np.asarray(target, dtype=np.int64).reshape(-1)
    B, C = lp.shape
    assert t.shape == (B,)
    ok = (t >= 0) & (t < C)
    pred = np.argmax(lp, axis=1)
    terms = -lp[ok, t[ok]].astype(np.float64)
    with np.errstate(all="ignore"):
        nll = float(terms.sum()) if terms.size else 0.0
        kl_term = float(np.float64(np.float32(kl)) * np.float64(np.float32(kl_scale))) if kl is not None else 0.0
        loss32 = np.float32(nll + kl_term)
    return {"rows": B, "valid": int(ok.sum()), "bad_targets": int((~ok).sum()),
            "correct": int((pred[ok] == t[ok]).sum()),
            "nonfinite_rows": int((~np.isfinite(lp).all(axis=1)).sum()),
            "nll": nll, "kl_term": kl_term, "loss": float(loss32), "loss64": nll + kl_term,
            "finite": bool(np.isfinite(loss32)), "abs_terms": float(np.abs(terms).sum()) if terms.size else 0.0}


def totals(steps, skipped_steps=0) -> dict:
    """The totals after the calls ``steps`` (dicts of ``step``), from zero.  ``<sum>_abs``: the sum of the absolute values of what
    the sum added, the scale of its rounding bound."""
    out = dict.fromkeys(COUNT_NAMES, 0)
    out.update({k: 0.0 for k in SUM_NAMES})
    out.update({k + "_abs": 0.0 for k in SUM_NAMES})
    out["skipped_steps"] = int(skipped_steps)
    out["last_nll"] = out["last_loss"] = 0.0
    for s in steps:
        out["steps"] += 1
        for k in ("rows", "correct", "bad_targets", "nonfinite_rows"):
            out[k] += s[k]
        if s["finite"]:                                       # one bad batch does not destroy the means of the epoch
            out["nll_rows"] += s["valid"]
            out["nll_sum"] += s["nll"]
            out["kl_term_sum"] += s["kl_term"]
            out["loss_sum"] += s["loss64"]
            out["nll_sum_abs"] += s["abs_terms"]
            out["kl_term_sum_abs"] += abs(s["kl_term"])
            out["loss_sum_abs"] += s["abs_terms"] + abs(s["kl_term"])
        else:
            out["nonfinite_steps"] += 1
        out["last_nll"], out["last_loss"] = s["nll"], s["loss"]
    div = lambda x, d: x / d if d else float("nan")
    out["nll_mean"] = div(out["nll_sum"], out["nll_rows"])
    out["loss_mean"] = div(out["loss_sum"], out["steps"] - out["nonfinite_steps"])
    out["accuracy"] = div(out["correct"], out["rows"] - out["bad_targets"])
    return out
