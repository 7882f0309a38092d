"""Test helper: float64 restatement of what lbbnn_lrt_study_fit (include/lbbnn.h; csrc/lrt_study.hip) does to ONE replicate --
a one-layer LRT network I -> O with a sigmoid head, BCELoss(sum) + kl * batch / N, analytic gradients, Adam with per-epoch
rates and restarts, the guard and the per-epoch history -- in torch CPU ops, with eps_out from tests/philox_ref.normal_matrix.
Not part of the product.  The expressions are those of LBBNN-GP-MF-LRT.py:167-194 and of torch's binary_cross_entropy / Adam;
``loss_terms`` is differentiable, so tests/test_replicate_study_host.py holds ``analytic_grads`` against torch.autograd on it."""
import math

import numpy as np
import torch

import philox_ref

NAMES = ("weight_mu", "weight_rho", "lambdal", "bias_mu", "bias_rho")
STREAM_EPS_OUT = 0                         # LBBNN_STREAM_EPS_OUT * 64 + layer id 0
FLOOR = float(np.float32(1e-12))           # the backward's denominator floor, the kernel's 1e-12f
PRIORS = dict(mu_prior=0.0, sigma_prior=1.0, alpha_prior=0.05, bias_mu_prior=0.0, bias_sigma_prior=1.0)


def priors_dict(p=None):
    """A bnn_amd.Priors (or None: the defaults) as a dict of the float32 values the kernel reads."""
    if p is None:
        return dict(PRIORS)
    if isinstance(p, dict):
        return {k: float(np.float32(v)) for k, v in p.items()}
    return {k: float(np.float32(getattr(p, k))) for k in PRIORS}


def f64(P):
    return {k: torch.as_tensor(v).detach().cpu().to(torch.float64).clone() for k, v in P.items()}


def target_ok(y):
    return (y >= 0) & (y <= 1)             # False for NaN


def loss_terms(P, x, y, eps, pri, kl_scale):
    """(nll, kl, probs, std) of one batch in float64 torch ops, differentiable in P."""
    alpha = 1 / (1 + torch.exp(-P["lambdal"]))
    sigma = torch.log1p(torch.exp(P["weight_rho"]))
    sb = torch.log1p(torch.exp(P["bias_rho"]))
    e_w = P["weight_mu"] * alpha
    var_w = sigma ** 2 * alpha ** 2
    mean = x @ e_w.T + P["bias_mu"]
    std = torch.sqrt((x ** 2) @ var_w.T + sb ** 2)
    p = 1 / (1 + torch.exp(-(mean + std * eps)))
    ok = target_ok(y)
    ys = torch.where(ok, y, torch.zeros_like(y))
    lp = torch.clamp(torch.log(p), min=-100)
    lq = torch.clamp(torch.log1p(-p), min=-100)
    t = (ys - 1) * lq - ys * lp
    t = torch.where(torch.isnan(t), torch.full_like(t, 100.0), t)            # fmax returns its number: a NaN probability costs 100
    nll = torch.where(ok, t, torch.zeros_like(t)).sum()
    sp, bsp = pri["sigma_prior"], pri["bias_sigma_prior"]
    kl_bias = (torch.log(bsp / sb) - 0.5 + (sb ** 2 + (P["bias_mu"] - pri["bias_mu_prior"]) ** 2) / (2 * bsp ** 2)).sum()
    kl_w = (alpha * (torch.log(sp / sigma) - 0.5 + torch.log(alpha / pri["alpha_prior"])
                     + (sigma ** 2 + (P["weight_mu"] - pri["mu_prior"]) ** 2) / (2 * sp ** 2))
            + (1 - alpha) * torch.log((1 - alpha) / (1 - pri["alpha_prior"]))).sum()
    return nll, kl_bias + kl_w, p, std


def analytic_grads(P, x, y, eps, pri, kl_scale):
    """d (nll + kl * kl_scale) / d P by hand: the logits, the batch reductions to d e_w, d var_w, d bias, d bias_var, the chain
    through alpha, sigma and the KL terms."""
    mu, rho, lam, bmu, brho = (P[n] for n in NAMES)
    alpha = 1 / (1 + torch.exp(-lam))
    sigma = torch.log1p(torch.exp(rho))
    dsig = 1 / (1 + torch.exp(-rho))
    sb = torch.log1p(torch.exp(brho))
    dsb = 1 / (1 + torch.exp(-brho))
    _, _, p, std = loss_terms(P, x, y, eps, pri, kl_scale)
    ok = target_ok(y)
    d = (1 - p) * p
    g = torch.where(ok, (p - torch.where(ok, y, torch.zeros_like(y))) / torch.clamp(d, min=FLOOR) * d, torch.zeros_like(p))
    gv = g * eps / (2 * std)
    dWm, dWv = g.T @ x, gv.T @ (x ** 2)
    g_sum, gv_sum = g.sum(0), gv.sum(0)
    inv_sp2 = 1 / pri["sigma_prior"] ** 2
    dd = mu - pri["mu_prior"]
    T = (math.log(pri["sigma_prior"]) - torch.log(sigma)) - 0.5 + (torch.log(alpha) - math.log(pri["alpha_prior"])) \
        + (sigma ** 2 + dd ** 2) * 0.5 * inv_sp2
    Gmu = dWm * alpha + kl_scale * alpha * dd * inv_sp2
    Gsig = dWv * 2 * sigma * alpha ** 2 + kl_scale * alpha * (sigma * inv_sp2 - 1 / sigma)
    Gal = dWm * mu + dWv * 2 * sigma ** 2 * alpha + kl_scale * (T - (torch.log(1 - alpha) - math.log(1 - pri["alpha_prior"])))
    binv = 1 / pri["bias_sigma_prior"] ** 2
    return {"weight_mu": Gmu, "weight_rho": Gsig * dsig, "lambdal": Gal * alpha * (1 - alpha),
            "bias_mu": g_sum + kl_scale * (bmu - pri["bias_mu_prior"]) * binv,
            "bias_rho": (gv_sum * 2 * sb + kl_scale * (sb * binv - 1 / sb)) * dsb}


def fit(P0, x, y, epochs, batch, lr, restarts=(), betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, seed=0, offset=0, priors=None,
        state=None, drop_steps=()):
    """T = epochs * ceil(N / batch) steps of one replicate in float64.  P0: the float32 parameters; x (N, I), y (N, O); lr: the
    (epochs) rates as float32 values; state: dict(exp_avg, exp_avg_sq, step, offset, skipped) to continue.  ``drop_steps``:
    global step indices treated as skipped whatever their loss (the guard test states its expectation with it).
    Returns dict(params, exp_avg, exp_avg_sq, step, offset, skipped, history (epochs, 6), grads [per step: dict or None],
    finite [per step])."""
    pri = priors_dict(priors)
    P = f64(P0)
    x = torch.as_tensor(x).detach().cpu().to(torch.float64)
    y = torch.as_tensor(y).detach().cpu().to(torch.float64)
    N, O = x.shape[0], P["bias_mu"].numel()
    nb = -(-N // batch)
    kl_scale = float(np.float32(batch / N))
    b1, b2, eps_a, wd = (float(np.float32(v)) for v in (betas[0], betas[1], eps, weight_decay))
    lr = [float(np.float32(v)) for v in (lr if hasattr(lr, "__len__") else [lr] * epochs)]
    if state is None:
        m, v = {k: torch.zeros_like(t) for k, t in P.items()}, {k: torch.zeros_like(t) for k, t in P.items()}
        step, skipped = 0, 0
    else:
        m, v, step, skipped, offset = f64(state["exp_avg"]), f64(state["exp_avg_sq"]), int(state["step"]), int(state["skipped"]), int(state["offset"])
    history = np.zeros((epochs, 6))
    grads, finite_steps, t_global = [], [], 0
    for ep in range(epochs):
        if ep in restarts:
            m, v, step = {k: torch.zeros_like(t) for k, t in P.items()}, {k: torch.zeros_like(t) for k, t in P.items()}, 0
        s_loss = s_nll = 0.0
        n_fin = n_ok = n_el = n_skip = 0
        last_loss = last_nll = 0.0
        for k in range(nb):
            xb, yb = x[k * batch:(k + 1) * batch], y[k * batch:(k + 1) * batch]
            e = torch.from_numpy(philox_ref.normal_matrix(seed, offset, STREAM_EPS_OUT, xb.shape[0], O))
            nll, kl, p, _ = loss_terms(P, xb, yb, e, pri, kl_scale)
            kl32 = float(np.float32(float(kl)))                          # the KL is a float32 number before it is scaled
            loss = float(nll) + kl32 * kl_scale
            with np.errstate(over="ignore"):
                loss32 = float(np.float32(loss))
            finite = bool(np.isfinite(loss32)) and bool(torch.isfinite(p).all()) and t_global not in drop_steps
            ok = target_ok(yb)
            p32, y32 = p.to(torch.float32), yb.to(torch.float32)
            n_ok += int((((p32 > 0.5) == (y32 > 0.5)) & ok).sum())
            n_el += p.numel()
            last_loss, last_nll = loss32, float(nll)
            if finite:
                g = analytic_grads(P, xb, yb, e, pri, kl_scale)
                step += 1
                bc1, bc2s = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
                for name in NAMES:
                    gq = g[name] + wd * P[name]
                    m[name] = b1 * m[name] + (1 - b1) * gq
                    v[name] = b2 * v[name] + (1 - b2) * gq * gq
                    P[name] = P[name] - (lr[ep] / bc1) * (m[name] / (torch.sqrt(v[name]) / bc2s + eps_a))
                s_loss += loss; s_nll += float(nll); n_fin += 1
                grads.append(g)
            else:
                skipped += 1; n_skip += 1
                grads.append(None)
            finite_steps.append(finite)
            offset += 1
            t_global += 1
        history[ep] = [s_loss / n_fin if n_fin else float("nan"), s_nll / n_fin if n_fin else float("nan"), n_ok / n_el,
                       last_loss, last_nll, n_skip]
    return dict(params=P, exp_avg=m, exp_avg_sq=v, step=step, offset=offset, skipped=skipped, history=history, grads=grads,
                finite=finite_steps)


def pack(P):
    """A replicate's packed row: [weight_mu | weight_rho | lambdal | bias_mu | bias_rho]."""
    return torch.cat([torch.as_tensor(P[n]).reshape(-1) for n in NAMES])
