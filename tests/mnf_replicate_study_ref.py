"""Test helper: float64 restatement of what lbbnn_mnf_study_fit (include/lbbnn.h; csrc/lrt_study.hip, the MNF instantiation)
does to ONE replicate -- a one-layer planar-MNF network I -> O with a sigmoid head.  The loss of a batch is
``oracle.mnf_forward`` (planar flows: ``planar_step_1d``) + BCELoss(sum) + kl * batch / N, its gradients are torch.autograd's in
float64, the draws come from tests/philox_ref, and Adam, restarts, the guard and the history are written as in
tests/replicate_study_ref.fit, with three rate groups (the ten named tensors | z_flow | r_flow).  Not part of the product.

``acting`` is the second parameter setting of the tests: the seeded initialisation, u, w ~ U(+-0.01), leaves every log-det at
1e-7 of the KL, so it gives u elements of order one, builds w and the bias so that u.w and w.z + b (on the KL draw of the first
step) take the values of planar_forward_ref.UW / INNER -- one of them with 1 + (1 - th^2) u.w < 0, the abs() branch -- and draws
q0_log_var from U(-3, 0).  A draw is kept only if the float64 reference alone shows the conditioning of
``planar_forward_ref.conditioned``; otherwise the next seed is taken."""
import math

import numpy as np
import torch

import philox_ref
import planar_forward_ref as pfr
from oracle import lbbnn_oracle as orc
from replicate_study_ref import PRIORS, f64, priors_dict, target_ok  # noqa: F401

BASE_NAMES = ("weight_mu", "weight_rho", "lambdal", "bias_mu", "bias_rho", "q0_mean", "q0_log_var", "r0_c", "r0_b1", "r0_b2")
STREAM_EPS_OUT, STREAM_EPS_Z, STREAM_EPS_Z2, STREAM_EPS_ACT = 0, 64, 128, 192         # LBBNN_STREAM_* * 64 + layer id 0


def names(Tz, Tr):
    """A replicate's tensors in the order of its packed row (MNFBayesianLinear._param_list())."""
    out = list(BASE_NAMES)
    for fl, T in (("z_flow", Tz), ("r_flow", Tr)):
        for t in range(T):
            out += ["%s.%d.u" % (fl, t), "%s.%d.w" % (fl, t), "%s.%d.b" % (fl, t)]
    return out


def group_of(name):
    return 1 if name.startswith("z_flow") else 2 if name.startswith("r_flow") else 0


def counts(P):
    return (sum(1 for k in P if k.startswith("z_flow") and k.endswith(".u")),
            sum(1 for k in P if k.startswith("r_flow") and k.endswith(".u")))


def net_params(net):
    """{name: CPU float32 clone} of a one-layer mnf.BayesianNetwork."""
    l1 = net.l1
    P = {n: getattr(l1, n).detach().cpu().clone() for n in BASE_NAMES}
    for fl in ("z_flow", "r_flow"):
        for t, tr in enumerate(getattr(l1, fl).transforms):
            for short, attr in (("u", "u"), ("w", "w"), ("b", "bias")):
                P["%s.%d.%s" % (fl, t, short)] = getattr(tr, attr).detach().cpu().clone()
    return P


def set_net_params(net, P):
    l1 = net.l1
    with torch.no_grad():
        for n in BASE_NAMES:
            getattr(l1, n).copy_(P[n].to(torch.float32))
        for fl in ("z_flow", "r_flow"):
            for t, tr in enumerate(getattr(l1, fl).transforms):
                for short, attr in (("u", "u"), ("w", "w"), ("b", "bias")):
                    getattr(tr, attr).copy_(P["%s.%d.%s" % (fl, t, short)].to(torch.float32))


def draws(seed, offset, B, I, O):
    """The draws of one step, float64: the keys of oracle.mnf_forward's ``noise``."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return {"eps_z": t(philox_ref.normal_vector(seed, offset, STREAM_EPS_Z, I)).reshape(1, I),
            "eps_z2": t(philox_ref.normal_vector(seed, offset, STREAM_EPS_Z2, I)).reshape(1, I),
            "eps_act": t(philox_ref.normal_vector(seed, offset, STREAM_EPS_ACT, O)),
            "eps_out": t(philox_ref.normal_matrix(seed, offset, STREAM_EPS_OUT, B, O))}


def flows_of(P):
    Tz, Tr = counts(P)
    mk = lambda fl, T: orc.Flow("Planar", [{"u": P["%s.%d.u" % (fl, t)], "w": P["%s.%d.w" % (fl, t)], "bias": P["%s.%d.b" % (fl, t)]}
                                           for t in range(T)])
    return mk("z_flow", Tz), mk("r_flow", Tr)


def loss_terms(P, x, y, noise, pri):
    """(nll, kl, probs) of one batch in float64 torch ops, differentiable in P: oracle.mnf_forward, the sigmoid head and
    torch's BCELoss(sum) (the logs clamped at -100)."""
    zf, rf = flows_of(P)
    act, kl, _ = orc.mnf_forward(x, P, zf, rf, noise, priors=orc.Priors(**pri))
    p = 1 / (1 + torch.exp(-act))
    ok = target_ok(y)
    ys = torch.where(ok, y, torch.zeros_like(y))
    t = (ys - 1) * torch.clamp(torch.log1p(-p), min=-100) - ys * torch.clamp(torch.log(p), min=-100)
    t = torch.where(torch.isnan(t), torch.full_like(t, 100.0), t)            # fmax returns its number: a NaN probability costs 100
    nll = torch.where(ok, t, torch.zeros_like(t)).sum()
    return nll, kl.reshape(()), p


def gradients(P, x, y, noise, pri, kl_scale):
    """d (nll + kl * kl_scale) / d P by torch.autograd in float64."""
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    nll, kl, _ = loss_terms(Pg, x, y, noise, pri)
    (nll + kl * kl_scale).backward()
    return {k: v.grad for k, v in Pg.items()}


def fit(P0, x, y, epochs, batch, lr, restarts=(), betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, seed=0, offset=0, priors=None,
        state=None, drop_steps=()):
    """replicate_study_ref.fit for an MNF replicate.  lr: (epochs, 3) rates -- the named tensors, z_flow, r_flow -- as float32
    values, or one number.  Returns the same dict."""
    pri = priors_dict(priors)
    P = f64(P0)
    nm = [n for n in names(*counts(P))]
    x = torch.as_tensor(x).detach().cpu().to(torch.float64)
    y = torch.as_tensor(y).detach().cpu().to(torch.float64)
    N, (O, I) = x.shape[0], P["weight_mu"].shape
    nb = -(-N // batch)
    kl_scale = float(np.float32(batch / N))
    b1, b2, eps_a, wd = (float(np.float32(v)) for v in (betas[0], betas[1], eps, weight_decay))
    lr = np.broadcast_to(np.asarray(lr, dtype=np.float32).reshape(-1, 3) if np.ndim(lr) else np.float32(lr), (epochs, 3)).astype(np.float64)
    zeros = lambda: {k: torch.zeros_like(t) for k, t in P.items()}
    if state is None:
        m, v, step, skipped = zeros(), zeros(), 0, 0
    else:
        m, v, step, skipped, offset = f64(state["exp_avg"]), f64(state["exp_avg_sq"]), int(state["step"]), int(state["skipped"]), int(state["offset"])
    history = np.zeros((epochs, 6))
    grads, finite_steps, t_global = [], [], 0
    for ep in range(epochs):
        if ep in restarts:
            m, v, step = zeros(), zeros(), 0
        s_loss = s_nll = 0.0
        n_fin = n_ok = n_el = n_skip = 0
        last_loss = last_nll = 0.0
        for k in range(nb):
            xb, yb = x[k * batch:(k + 1) * batch], y[k * batch:(k + 1) * batch]
            noise = draws(seed, offset, xb.shape[0], I, O)
            with torch.no_grad():
                nll, kl, p = loss_terms(P, xb, yb, noise, pri)
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
                g = gradients(P, xb, yb, noise, pri, kl_scale)
                step += 1
                bc1, bc2s = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
                for name in nm:
                    gq = g[name] + wd * P[name]
                    m[name] = b1 * m[name] + (1 - b1) * gq
                    v[name] = b2 * v[name] + (1 - b2) * gq * gq
                    P[name] = P[name] - (lr[ep, group_of(name)] / bc1) * (m[name] / (torch.sqrt(v[name]) / bc2s + eps_a))
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
    """A replicate's packed row."""
    return torch.cat([torch.as_tensor(P[n]).reshape(-1) for n in names(*counts(P))])


# ------------------------------------------------------------------------------------------------ the acting-flows setting
def _k3_view(P, noise):
    """The replicate's flow inputs under planar_forward_ref's names."""
    d = {"q0_mean": P["q0_mean"], "q0_log_var": P["q0_log_var"], "eps_fwd": noise["eps_z"].reshape(-1).float(),
         "eps_kl": noise["eps_z2"].reshape(-1).float()}
    for fl, short in (("z_flow", "z"), ("r_flow", "r")):
        for t in range(counts(P)[0 if short == "z" else 1]):
            for k in ("u", "w", "b"):
                d["%s.%d.%s" % (short, t, k)] = P["%s.%d.%s" % (fl, t, k)]
    return d


def _acting_draw(P0, gen_seed, noise):
    P = {k: v.clone() for k, v in P0.items()}
    Tz, Tr = counts(P)
    I = P["q0_mean"].numel()
    g = torch.Generator().manual_seed(gen_seed)
    n = lambda k: torch.randn(k, generator=g)
    P["q0_log_var"] = torch.empty(I).uniform_(-3.0, 0.0, generator=g)
    z = P["q0_mean"].double() + torch.exp(0.5 * P["q0_log_var"].double()) * noise["eps_z2"].reshape(-1)
    for fl, T in (("z_flow", Tz), ("r_flow", Tr)):
        for t in range(T):
            k = t + (Tz if fl == "r_flow" else 0)
            u = n(I)
            noise_w = 0.3 * n(I) / math.sqrt(I)
            c = pfr.UW[k % 4] - float(torch.dot(u.double(), noise_w.double()))
            w = (noise_w.double() + c * u.double() / torch.dot(u.double(), u.double())).float()
            b = torch.tensor([pfr.INNER[k % 5] - float(torch.dot(w.double(), z))], dtype=torch.float32)
            P["%s.%d.u" % (fl, t)], P["%s.%d.w" % (fl, t)], P["%s.%d.b" % (fl, t)] = u, w, b
            z = z + u.double() * torch.tanh(torch.dot(w.double(), z) + b.double())
    return P


def acting(P0, seed, offset, gen_seed=0):
    """P0 (float32, a seeded network's values) with acting flows for the step drawn from Philox state {seed, offset}: the first
    draw (gen_seed, gen_seed + 1000, ...) that planar_forward_ref.conditioned accepts.  Returns float32 tensors."""
    O, I = P0["weight_mu"].shape
    noise = draws(seed, offset, 1, I, O)
    Tz, Tr = counts(P0)
    for redraw in range(pfr.MAX_REDRAWS):
        P = _acting_draw(P0, gen_seed + 1000 * redraw, noise)
        if not pfr.conditioned(_k3_view(P, noise), Tz, Tr):
            return P
    raise RuntimeError("no well-conditioned acting-flows draw at %r" % ((O, I, Tz, Tr, seed, offset, gen_seed),))
