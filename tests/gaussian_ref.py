"""Float64 restatement of csrc/gaussian_head.hip and csrc/eval_regression.hip (include/lbbnn.h: lbbnn_elbo_gaussian_loss*,
lbbnn_eval_regression) on float32 inputs, in numpy; the two bit-reproducible outputs (pred_mean, epistemic_var) in numpy float32
in the documented order.  Imported by the host and GPU tests of the regression column; nothing here touches a device."""
import math

import numpy as np

LOG_2PI = math.log(2.0 * math.pi)
DBL = 1e-12                      # fp64 totals against the fp64 sum of the same terms: |diff| <= DBL * sum|term|


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _lv_block(lv, shape):
    lv = _f64(lv)
    return np.broadcast_to(lv, shape) if lv.ndim == 1 else lv


# ------------------------------------------------------------------------------------------------------------------- the loss
def parts(mean, target, log_var):
    """(ok, d, q, lv) of every element in float64: ok = the target is finite, d = y - m (0 where not ok), q = d^2 exp(-lv)."""
    m, y = _f64(mean), _f64(target).reshape(np.shape(mean))
    lv = _lv_block(log_var, m.shape)
    ok = np.isfinite(y)
    with np.errstate(all="ignore"):
        d = np.where(ok, y - m, 0.0)
        q = d * d * np.exp(-lv)
    return ok, d, q, lv


def terms(mean, target, log_var):
    """0.5 (log 2 pi + lv + (y - m)^2 exp(-lv)) per element, 0 for a bad target."""
    ok, d, q, lv = parts(mean, target, log_var)
    with np.errstate(all="ignore"):
        return np.where(ok, 0.5 * (LOG_2PI + lv + q), 0.0)


def magnitude(mean, target, log_var):
    """0.5 (|log 2 pi| + |lv| + q) per element: what a term's rounding errors are relative to (the term itself may cancel)."""
    ok, d, q, lv = parts(mean, target, log_var)
    return np.where(ok, 0.5 * (LOG_2PI + np.abs(lv) + q), 0.0)


def loss(mean, target, log_var, kl=None, scale=1.0):
    return float(terms(mean, target, log_var).sum()) + (float(kl) * float(scale) if kl is not None else 0.0)


def grads(g, mean, target, log_var, scale):
    """(g_mean (B, O), g_lv in the shape of log_var, g_kl) in float64."""
    ok, d, q, lv = parts(mean, target, log_var)
    g = float(g)
    g_mean = np.where(ok, g * (-d) * np.exp(-lv), 0.0)
    e = np.where(ok, g * 0.5 * (1.0 - q), 0.0)
    return g_mean, (e.sum(0) if np.ndim(log_var) == 1 else e), g * float(scale)


def grad_lv_magnitude(g, mean, target, log_var):
    """|g| 0.5 (1 + q) per element (summed over the batch for a shared log_var): what g_lv's rounding errors are relative to."""
    ok, d, q, lv = parts(mean, target, log_var)
    e = np.where(ok, abs(float(g)) * 0.5 * (1.0 + q), 0.0)
    return e.sum(0) if np.ndim(log_var) == 1 else e


def stats(mean, target):
    """[squared-error sum, absolute-error sum, elements with a valid target, bad targets] of one call."""
    m, y = _f64(mean), _f64(target).reshape(np.shape(mean))
    ok = np.isfinite(y)
    d = np.where(ok, y - m, 0.0)
    return [float((d * d).sum()), float(np.abs(d).sum()), float(ok.sum()), float((~ok).sum())]


def counts(mean, target, log_var):
    """The integer counts a monitored call adds: rows, correct (inside one standard deviation), bad_targets, nonfinite_rows.
    `correct` uses float32 arithmetic for the comparison's two sides, as the kernel does: |y - m| <= expf(0.5f * lv)."""
    m32, y32 = np.asarray(mean, np.float32), np.asarray(target, np.float32).reshape(np.shape(mean))
    lv32 = np.broadcast_to(np.asarray(log_var, np.float32), m32.shape) if np.ndim(log_var) == 1 else np.asarray(log_var, np.float32)
    ok = np.isfinite(y32)
    with np.errstate(all="ignore"):
        inside = ok & (np.abs(y32 - m32) <= np.exp((np.float32(0.5) * lv32).astype(np.float64)))
    return {"rows": int(m32.size), "correct": int(inside.sum()), "bad_targets": int((~ok).sum()),
            "nonfinite_rows": int((~np.isfinite(m32) | ~np.isfinite(lv32)).sum())}


# ------------------------------------------------------------------------------------------------------------- the metrics
def pred_mean_f32(out):
    """acc = m_0; acc += m_s ascending; acc / (float)S, in float32: the kernel's bits."""
    out = np.asarray(out, np.float32)
    acc = out[0].copy()
    for s in range(1, out.shape[0]):
        acc = (acc + out[s]).astype(np.float32)
    return (acc / np.float32(out.shape[0])).astype(np.float32)


def epistemic_var_f32(out, pm=None):
    """d_s = m_s - pred_mean; acc = d_0 d_0; acc += d_s d_s ascending; acc / (float)S, in float32: the kernel's bits."""
    out = np.asarray(out, np.float32)
    pm = pred_mean_f32(out) if pm is None else np.asarray(pm, np.float32)
    acc = None
    with np.errstate(invalid="ignore"):                          # (an infinite member: inf - inf)
        for s in range(out.shape[0]):
            d = (out[s] - pm).astype(np.float32)
            dd = (d * d).astype(np.float32)
            acc = dd if acc is None else (acc + dd).astype(np.float32)
    return (acc / np.float32(out.shape[0])).astype(np.float32)


_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def metrics(out, target, log_var):
    """The per-element outputs in float64 from float32 inputs (pred_mean and epistemic_var: the float32 values above, as the
    kernel derives the others from them): dict of (B, O) arrays; NaN in sq_err / log_density / pit without a valid target.
    ``log_density_mag``: max_s (|log 2 pi| + |lv| + q_s), what log_density's rounding errors are relative to."""
    o32 = np.asarray(out, np.float32)
    S, B, O = o32.shape
    lv = np.broadcast_to(_f64(np.asarray(log_var, np.float32)), (B, O))
    pm32 = pred_mean_f32(o32)
    ev32 = epistemic_var_f32(o32, pm32)
    res = {"pred_mean": pm32, "epistemic_var": ev32, "aleatoric_var": np.exp(lv),
           "total_std": np.sqrt(_f64(ev32) + np.exp(lv))}
    nan = np.full((B, O), np.nan)
    if target is None:
        res.update(sq_err=nan, log_density=nan, pit=nan, log_density_mag=nan, valid=np.zeros((B, O), bool))
        return res
    y = _f64(np.asarray(target, np.float32)).reshape(B, O)
    ok = np.isfinite(y)
    ys = np.where(ok, y, 0.0)
    with np.errstate(all="ignore"):
        r = ys[None] - _f64(o32)
        q = r * r * np.exp(-lv)[None]
        t = -0.5 * (LOG_2PI + lv[None] + q)
        mx = t.max(0)
        ld = mx + np.log(np.exp(t - mx[None]).sum(0)) - math.log(S)
        pit = (0.5 * _erfc(-(r * np.exp(-0.5 * lv)[None]) / math.sqrt(2.0))).mean(0)
        mag = (LOG_2PI + np.abs(lv)[None] + q).max(0)
    e = ys - _f64(pm32)
    res.update(sq_err=np.where(ok, e * e, np.nan), log_density=np.where(ok, ld, np.nan), pit=np.where(ok, pit, np.nan),
               log_density_mag=np.where(ok, mag, np.nan), valid=ok)
    return res


def totals(per_batch, pit_bins, kernel=None):
    """Counts, float64 sums and the PIT histogram of a pass from [(out, target, log_var, mean_out or None)].  ``kernel``: per
    batch the dict of the kernel's own float32 per-element outputs -- the sums are then those of ITS values in float64 (what
    the DBL bar is about); the histogram is always the float64 reference's."""
    c = dict(elements=0, elements_with_target=0, bad_targets=0, nonfinite_elements=0, scored_elements=0)
    names = ("sq_err", "abs_err", "log_density", "epistemic_var", "total_var", "y", "y2", "posterior_mean_sq_err")
    s, a = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0)
    hist = np.zeros(pit_bins, np.int64)
    for i, (out, target, lv, mean_out) in enumerate(per_batch):
        o32 = np.asarray(out, np.float32)
        S, B, O = o32.shape
        ref = metrics(o32, target, lv)
        k = ref if kernel is None else {n: _f64(v) for n, v in kernel[i].items()}
        lv32 = np.broadcast_to(np.asarray(lv, np.float32), (B, O))
        fin = np.isfinite(o32).all(0) & np.isfinite(lv32)
        has_t = target is not None
        y32 = np.asarray(target, np.float32).reshape(B, O) if has_t else np.full((B, O), np.nan, np.float32)
        ok = np.isfinite(y32)
        scored = fin & ok
        c["elements"] += B * O
        c["elements_with_target"] += int(ok.sum())
        c["bad_targets"] += int((~ok).sum()) if has_t else 0
        c["nonfinite_elements"] += int((~fin).sum())
        c["scored_elements"] += int(scored.sum())
        pm = _f64(k["pred_mean"])
        vals = {"sq_err": _f64(k["sq_err"]), "abs_err": np.abs(_f64(y32) - pm) if kernel is None else
                _f64(np.abs((y32 - np.asarray(kernel[i]["pred_mean"], np.float32)).astype(np.float32))),
                "log_density": _f64(k["log_density"]), "y": _f64(y32), "y2": _f64((y32 * y32).astype(np.float32))}
        if mean_out is not None:
            f = (y32 - np.asarray(mean_out, np.float32)).astype(np.float32)
            vals["posterior_mean_sq_err"] = _f64((f * f).astype(np.float32))
        for n, v in vals.items():
            s[n] += float(v[scored].sum())
            a[n] += float(np.abs(v[scored]).sum())
        ev = _f64(k["epistemic_var"])
        tv = _f64((np.asarray(k["epistemic_var"], np.float32) + np.asarray(k["aleatoric_var"], np.float32)).astype(np.float32)) \
            if kernel is not None else ev + _f64(ref["aleatoric_var"])
        for n, v in (("epistemic_var", ev), ("total_var", tv)):
            s[n] += float(v[fin].sum())
            a[n] += float(np.abs(v[fin]).sum())
        if has_t:
            b = np.clip(np.floor(ref["pit"][scored] * pit_bins).astype(np.int64), 0, pit_bins - 1)
            hist += np.bincount(b, minlength=pit_bins)
    return c, s, a, hist


def pit_margin(out, target, log_var, pit_bins):
    """The smallest distance of pit * pit_bins from an integer over the SCORED elements -- a valid target, every member and the
    log-variance finite: the elements that enter a bin -- by the float64 reference."""
    ref = metrics(out, target, log_var)
    o32 = np.asarray(out, np.float32)
    fin = np.isfinite(o32).all(0) & np.isfinite(np.broadcast_to(np.asarray(log_var, np.float32), o32.shape[1:]))
    v = ref["pit"][ref["valid"] & fin] * pit_bins
    return float(np.abs(v - np.round(v)).min()) if v.size else float("inf")
