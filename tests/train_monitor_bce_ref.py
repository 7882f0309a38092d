"""numpy float64 restatement of what lbbnn_elbo_bce_loss_monitor keeps in a TrainMonitor (include/lbbnn.h): the
counts, the three sums over the steps whose loss is finite and the two values of the last step -- tests/train_monitor_ref.py
for the binary loss.  The unit of account is one element (b, o) of the (B, O) block.

A term is the fp32 number the kernel forms, (y - 1) fmax(log1p(-p), -100) - y fmax(log p, -100) with every operation rounded to
float32 and fmax returning its number when the other side is a NaN (so a NaN probability against a valid target costs 100 and
leaves the loss finite); the terms are then added in float64.  The fp32 logarithms come from a maths library and the device's
rounds the last bit differently from numpy's (and from torch.log's): ``step(..., terms=)`` takes the (B, O) fp32 terms formed
elsewhere (the GPU tests take them from lbbnn_elbo_bce_loss on one element at a time) and checks nothing but their shape;
without it they are numpy's.  ``loss``
is the fp32 number the kernel writes, (float32)(nll + kl * kl_scale), and "finite" is said of that fp32 number.  Every step
also reports the absolute values of the terms its sums are made of, for the worst-case rounding bound of the tests."""
import numpy as np

from train_monitor_ref import COUNT_NAMES, SUM_NAMES, totals  # noqa: F401  (the totals of steps are family-independent)


def bce_terms(probs, target):
    """(B, O) float32: the kernel's term per element in numpy's float32 arithmetic; 0 where the target is not in [0, 1]."""
    p = np.asarray(probs, dtype=np.float32)
    y = np.asarray(target, dtype=np.float32).reshape(p.shape)
    m100, one = np.float32(-100.0), np.float32(1.0)
    with np.errstate(all="ignore"):
        ok = (y >= 0) & (y <= 1)                              # False for NaN
        lp = np.fmax(np.log(p), m100)
        lq = np.fmax(np.log1p(-p), m100)
        t = ((y - one) * lq).astype(np.float32) - (y * lp).astype(np.float32)
    return np.where(ok, t, np.float32(0.0)).astype(np.float32)


def step(probs, target, kl=None, kl_scale=1.0, terms=None) -> dict:
    """One call: its own numbers (not yet totals), with the keys of ``train_monitor_ref.step``; "rows" are elements."""
    p = np.asarray(probs, dtype=np.float32)
    assert p.ndim == 2
    y = np.asarray(target, dtype=np.float32).reshape(p.shape)
    with np.errstate(all="ignore"):
        ok = (y >= 0) & (y <= 1)
        t = bce_terms(p, y) if terms is None else np.asarray(terms, dtype=np.float32)
        assert t.shape == p.shape
        used = t[ok].astype(np.float64)
        nll = float(used.sum()) if used.size else 0.0
        kl_term = float(np.float64(np.float32(kl)) * np.float64(np.float32(kl_scale))) if kl is not None else 0.0
        loss32 = np.float32(nll + kl_term)
        correct = ((p > 0.5) == (y > 0.5)) & ok
        abs_terms = float(np.abs(used).sum()) if used.size else 0.0
    return {"rows": int(p.size), "valid": int(ok.sum()), "bad_targets": int((~ok).sum()), "correct": int(correct.sum()),
            "nonfinite_rows": int((~np.isfinite(p)).sum()),
            "nll": nll, "kl_term": kl_term, "loss": float(loss32), "loss64": nll + kl_term,
            "finite": bool(np.isfinite(loss32)), "abs_terms": abs_terms, "n_terms": int(used.size)}
