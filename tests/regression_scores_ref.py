"""Float64 restatement of csrc/eval_scores.hip (include/lbbnn.h: lbbnn_eval_regression_scores) on float32 inputs, in numpy: the
per-element outputs, the CRPS of a Gaussian mixture in closed form with the magnitude its rounding errors are relative to, the
mixture's quantiles by 200-step bisection with the density at them, the totals of a pass and the margins the exact integer
checks need.  The two bit-reproducible outputs come from gaussian_ref.  Imported by the host and GPU tests of the regression
scores; nothing here touches a device."""
import math

import numpy as np
from scipy import special

import gaussian_ref as g

LOG_2PI = g.LOG_2PI
DBL = g.DBL
MAX_ABS_LV = 80.0
MAX_LEVELS = 4
BISECTIONS = 200
COUNT_NAMES = ("elements", "elements_with_target", "bad_targets", "nonfinite_elements", "scored_elements")
SUM_NAMES = ("sq_err", "abs_err", "log_density", "epistemic_var", "total_var", "y", "y2", "posterior_mean_sq_err", "aleatoric_var",
             "crps")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def lv_block(log_var, shape):
    """The float32 log-variance operand -- (O,), (B, O) or (S, B, O) -- as a float64 (S, B, O) block."""
    return np.broadcast_to(_f64(np.asarray(log_var, np.float32)), shape)


def level_f32(p):
    """The level the kernel reads: the float32 nearest to p, as a float64."""
    return float(np.float32(p))


def finite(out, log_var):
    """(B, O) bool: every member's mean finite and every member's log-variance within +-80 (a NaN fails)."""
    o32 = np.asarray(out, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(o32).all(0) & (np.abs(lv_block(log_var, o32.shape)) <= MAX_ABS_LV).all(0)


def a_term(m, v):
    """A(m, v) = 2 sd phi(m / sd) + m (2 Phi(m / sd) - 1) = E|N(m, v)|, sd = sqrt v: non-negative."""
    sd = np.sqrt(v)
    z = m / sd
    return 2.0 * sd * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) + m * special.erf(z / math.sqrt(2.0))


def crps_mixture(means, variances, y):
    """(crps, M) of the equal-weight Gaussian mixture with ``means`` / ``variances`` (S, ...) at y (...): Grimit et al. 2006,
    crps = t1 - t2 with t1 = (1 / S) sum_s A(y - m_s, v_s) and t2 = (1 / 2 S^2) sum_{s,t} A(m_s - m_t, v_s + v_t); M = t1 + t2
    is what the rounding errors of an evaluation are relative to (every A is non-negative, the difference cancels)."""
    m, v = _f64(means), _f64(variances)
    S = m.shape[0]
    t1 = a_term(_f64(y)[None] - m, v).mean(0)
    t2 = a_term(m[:, None] - m[None, :], v[:, None] + v[None, :]).sum((0, 1)) / (2.0 * S * S)
    return t1 - t2, t1 + t2


def crps_normal(mean, sd, y):
    """The CRPS of one normal: sd (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt pi), z = (y - mean) / sd."""
    z = (_f64(y) - mean) / sd
    return sd * (z * (2.0 * special.ndtr(z) - 1.0) + 2.0 * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) - 1.0 / math.sqrt(math.pi))


def cdf(x, means, sds):
    """The mixture CDF at x (..., B, O) for members (S, B, O)."""
    return special.ndtr((_f64(x)[None] - means.reshape((means.shape[0],) + (1,) * (np.ndim(x) - 2) + means.shape[1:])) /
                        sds.reshape((sds.shape[0],) + (1,) * (np.ndim(x) - 2) + sds.shape[1:])).mean(0)


def density(x, means, sds):
    """The mixture density at x (..., B, O)."""
    shape = (means.shape[0],) + (1,) * (np.ndim(x) - 2) + means.shape[1:]
    m, s = means.reshape(shape), sds.reshape(shape)
    z = (_f64(x)[None] - m) / s
    return (np.exp(-0.5 * z * z) / (s * math.sqrt(2.0 * math.pi))).mean(0)


def quantiles(means, sds, probs):
    """(q (Q, B, O), lo (B, O), hi (B, O)): the ``probs`` quantiles of the mixture by BISECTIONS float64 bisection steps from
    the bracket [min_s (m_s - 8 sd_s), max_s (m_s + 8 sd_s)]."""
    lo0, hi0 = (means - 8.0 * sds).min(0), (means + 8.0 * sds).max(0)
    pr = _f64(probs).reshape(-1, 1, 1)
    lo, hi = np.broadcast_to(lo0, (len(pr),) + lo0.shape).copy(), np.broadcast_to(hi0, (len(pr),) + hi0.shape).copy()
    for _ in range(BISECTIONS):
        mid = 0.5 * (lo + hi)
        below = cdf(mid, means, sds) < pr
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi), lo0, hi0


def metrics(out, target, log_var, levels=()):
    """The per-element outputs in float64 from float32 inputs (pred_mean and epistemic_var: gaussian_ref's float32 values).
    dict of (B, O) arrays -- ``lower`` / ``upper`` / ``interval_score`` / ``density_lower`` / ``density_upper``: (levels, B, O) --
    NaN in every one for a non-finite element, NaN in sq_err / log_density / pit / crps / interval_score without a valid target.
    ``log_density_mag``: max_s (|log 2 pi| + |lv_s| + q_s); ``crps_mag``: M of crps_mixture; ``bracket_lo`` / ``bracket_hi``: the
    quantile bracket; ``valid``: the target is finite; ``finite``: the element is."""
    o32 = np.asarray(out, np.float32)
    S, B, O = o32.shape
    L = len(levels)
    fin = finite(o32, log_var)
    nan = np.full((B, O), np.nan)
    with np.errstate(all="ignore"):
        lv = np.where(fin[None], lv_block(log_var, o32.shape), 0.0)
        m = np.where(fin[None], _f64(o32), 0.0)
        var, sd = np.exp(lv), np.exp(0.5 * lv)
        pm32 = g.pred_mean_f32(o32)
        ev32 = g.epistemic_var_f32(o32, pm32)
        av = var.mean(0)
        res = {"pred_mean": np.where(fin, pm32, np.float32(np.nan)).astype(np.float32),
               "epistemic_var": np.where(fin, ev32, np.float32(np.nan)).astype(np.float32),
               "aleatoric_var": np.where(fin, av, np.nan), "total_std": np.where(fin, np.sqrt(_f64(ev32) + av), np.nan),
               "finite": fin}
        probs = [0.5 * (1.0 - level_f32(p)) for p in levels] + [0.5 * (1.0 + level_f32(p)) for p in levels]
        if L:
            q, lo, hi = quantiles(m, sd, probs)
            f = density(q, m, sd)
            res.update(lower=np.where(fin[None], q[:L], np.nan), upper=np.where(fin[None], q[L:], np.nan),
                       density_lower=np.where(fin[None], f[:L], np.nan), density_upper=np.where(fin[None], f[L:], np.nan),
                       bracket_lo=np.where(fin, lo, np.nan), bracket_hi=np.where(fin, hi, np.nan))
        else:
            res.update({k: np.zeros((0, B, O)) for k in ("lower", "upper", "density_lower", "density_upper")})
            res.update(bracket_lo=nan, bracket_hi=nan)
        if target is None:
            res.update(sq_err=nan, log_density=nan, pit=nan, crps=nan, crps_mag=nan, log_density_mag=nan,
                       interval_score=np.full((L, B, O), np.nan), valid=np.zeros((B, O), bool))
            return res
        y = _f64(np.asarray(target, np.float32)).reshape(B, O)
        ok = np.isfinite(y)
        use = ok & fin
        ys = np.where(ok, y, 0.0)
        r = ys[None] - m
        qq = r * r * np.exp(-lv)
        t = -0.5 * (LOG_2PI + lv + qq)
        mx = t.max(0)
        ld = mx + np.log(np.exp(t - mx[None]).sum(0)) - math.log(S)
        pit = special.ndtr(r / sd).mean(0)
        mag = (LOG_2PI + np.abs(lv) + qq).max(0)
        c, cm = crps_mixture(m, var, ys)
        e = ys - _f64(pm32)
        res.update(sq_err=np.where(use, e * e, np.nan), log_density=np.where(use, ld, np.nan), pit=np.where(use, pit, np.nan),
                   log_density_mag=np.where(use, mag, np.nan), crps=np.where(use, c, np.nan), crps_mag=np.where(use, cm, np.nan),
                   valid=ok)
        if L:
            k = np.array([2.0 / (1.0 - level_f32(p)) for p in levels]).reshape(L, 1, 1)
            sc = (q[L:] - q[:L]) + k * (np.maximum(q[:L] - ys[None], 0.0) + np.maximum(ys[None] - q[L:], 0.0))
            res["interval_score"] = np.where(use[None], sc, np.nan)
        else:
            res["interval_score"] = np.zeros((0, B, O))
    return res


def quantile_bars(ref, d_cdf):
    """(bar_lower, bar_upper) (levels, B, O): 2 dF / f(q) + 2^-22 (|q| + hi - lo) -- a CDF evaluation good to ``d_cdf`` moves
    the root by d_cdf / f(q); the second term is the float32 resolution of the bisection's bracket and midpoints."""
    span = (ref["bracket_hi"] - ref["bracket_lo"])[None]
    with np.errstate(all="ignore"):
        return tuple(2.0 * d_cdf / ref["density_" + k] + 2.0 ** -22 * (np.abs(ref[k]) + span) for k in ("lower", "upper"))


def interval_score_bar(ref, levels, bars):
    """The quantile bars through (u - l) + k ((l - y)+ + (y - u)+), k = 2 / (1 - p): each of the three terms moves by at most its
    quantile's bar, so (1 + k) (bar_l + bar_u); plus 1e-6 of the score for the float32 formula itself (k, two differences, a
    product and two sums: under 8 ulp of terms that are each at most the score)."""
    k = np.array([2.0 / (1.0 - level_f32(p)) for p in levels]).reshape(-1, 1, 1)
    return (1.0 + k) * (bars[0] + bars[1]) + 1e-6 * np.abs(ref["interval_score"])


def scored(ref):
    return ref["finite"] & ref["valid"]


def pit_margin(ref, pit_bins):
    """The smallest distance of pit * pit_bins from an integer over the scored elements."""
    v = ref["pit"][scored(ref)] * pit_bins
    return float(np.abs(v - np.round(v)).min()) if v.size else float("inf")


def interval_margin(ref, d_cdf):
    """min over the scored elements and both ends of every level of |y - q| / bar(q): how many quantile bars the nearest
    interval end is away from its target (the count of targets inside an interval is exact when this is > 1)."""
    s = scored(ref)
    if not s.any() or not ref["lower"].shape[0]:
        return float("inf")
    bars = quantile_bars(ref, d_cdf)
    y = ref["y"][None]
    worst = float("inf")
    for k, bar in zip(("lower", "upper"), bars):
        with np.errstate(all="ignore"):
            ratio = np.abs(y - ref[k]) / bar
        worst = min(worst, float(ratio[:, s].min()))
    return worst


def with_target(ref, target):
    """``ref`` with the float64 targets stored under "y" (what interval_margin and totals read)."""
    B, O = ref["finite"].shape
    ref["y"] = _f64(np.asarray(target, np.float32)).reshape(B, O) if target is not None else np.full((B, O), np.nan)
    return ref


def totals(per_batch, pit_bins, levels, kernel=None):
    """(counts, inside, sums, abs sums, level sums, abs level sums, pit histogram) of a pass from [(out, target, log_var, mean
    columns or None)].  ``kernel``: per batch the dict of the kernel's own float32 per-element outputs -- the sums are then those
    of ITS values in float64 (what the DBL bar is about); the histogram and the inside counts are always the float64
    reference's."""
    L = len(levels)
    c = dict.fromkeys(COUNT_NAMES, 0)
    inside = np.zeros(L, np.int64)
    s, a = dict.fromkeys(SUM_NAMES, 0.0), dict.fromkeys(SUM_NAMES, 0.0)
    ls = {k: np.zeros(L) for k in ("width", "interval_score")}
    la = {k: np.zeros(L) for k in ("width", "interval_score")}
    hist = np.zeros(pit_bins, np.int64)
    for i, (out, target, lv, mean_out) in enumerate(per_batch):
        o32 = np.asarray(out, np.float32)
        S, B, O = o32.shape
        ref = metrics(o32, target, lv, levels)
        k = ref if kernel is None else kernel[i]
        f32 = lambda n: np.asarray(k[n], np.float32)
        fin, has_t = ref["finite"], target is not None
        y32 = np.asarray(target, np.float32).reshape(B, O) if has_t else np.full((B, O), np.nan, np.float32)
        ok = np.isfinite(y32)
        sc = fin & ok
        c["elements"] += B * O
        c["elements_with_target"] += int(ok.sum())
        c["bad_targets"] += int((~ok).sum()) if has_t else 0
        c["nonfinite_elements"] += int((~fin).sum())
        c["scored_elements"] += int(sc.sum())
        with np.errstate(all="ignore"):
            if kernel is None:
                vals = {"sq_err": ref["sq_err"], "abs_err": np.abs(_f64(y32) - _f64(ref["pred_mean"])), "log_density": ref["log_density"],
                        "crps": ref["crps"], "y": _f64(y32), "y2": _f64(y32) * _f64(y32)}
                fvals = {"epistemic_var": _f64(ref["epistemic_var"]), "aleatoric_var": ref["aleatoric_var"],
                         "total_var": _f64(ref["epistemic_var"]) + ref["aleatoric_var"]}
                lvals = {"width": ref["upper"] - ref["lower"], "interval_score": ref["interval_score"]}
            else:
                vals = {"sq_err": _f64(f32("sq_err")), "abs_err": _f64(np.abs((y32 - f32("pred_mean")).astype(np.float32))),
                        "log_density": _f64(f32("log_density")), "crps": _f64(f32("crps")), "y": _f64(y32),
                        "y2": _f64((y32 * y32).astype(np.float32))}
                fvals = {"epistemic_var": _f64(f32("epistemic_var")), "aleatoric_var": _f64(f32("aleatoric_var")),
                         "total_var": _f64((f32("epistemic_var") + f32("aleatoric_var")).astype(np.float32))}
                lvals = {"width": _f64((f32("upper") - f32("lower")).astype(np.float32)), "interval_score": _f64(f32("interval_score"))}
            if mean_out is not None:
                d = (y32 - np.asarray(mean_out, np.float32)).astype(np.float32)
                vals["posterior_mean_sq_err"] = _f64((d * d).astype(np.float32))
        for n, v in vals.items():
            s[n] += float(v[sc].sum())
            a[n] += float(np.abs(v[sc]).sum())
        for n, v in fvals.items():
            s[n] += float(v[fin].sum())
            a[n] += float(np.abs(v[fin]).sum())
        for n, v in lvals.items():
            ls[n] += v[:, sc].sum(1)
            la[n] += np.abs(v[:, sc]).sum(1)
        if has_t:
            b = np.clip(np.floor(ref["pit"][sc] * pit_bins).astype(np.int64), 0, pit_bins - 1)
            hist += np.bincount(b, minlength=pit_bins)
            yy = _f64(y32)[None]
            with np.errstate(invalid="ignore"):
                inside += ((ref["lower"] <= yy) & (yy <= ref["upper"]))[:, sc].sum(1)
    return c, inside, s, a, ls, la, hist
