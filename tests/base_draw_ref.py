"""Plain references of the baseline LBBNN's in-kernel draws, shared by the GPU tests: torch's RelaxedBernoulli of given
uniforms (pinned to torch itself by tests/test_base_draws_host.py), the reparameterised Gamma precision, Philox snapshots,
the training kernels' chain of one network forward, and an fp64 network oracle built on ``oracle.lbbnn_oracle.base_forward``
that regenerates every draw from the documented Philox streams."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import lbbnn_oracle as orc

F32 = torch.finfo(torch.float32)


def _rng(dev, seed, offset):
    """A {seed, offset} Philox snapshot (2 int64 on the device)."""
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


def _clamp_probs(p):
    return p.clamp(min=F32.eps, max=1 - F32.eps)


def _relaxed(alpha, u, T):
    """torch's RelaxedBernoulli(probs=alpha, temperature=T).rsample() of fp32 probabilities given its uniforms u (the fp32
    clamps also when evaluated in fp64)."""
    p, uc = _clamp_probs(alpha), _clamp_probs(u)
    z = (uc.log() - (-uc).log1p() + p.log() - (-p).log1p()) / T
    return torch.clamp(torch.sigmoid(z), min=F32.tiny, max=1.0 - F32.eps)


def _presig(alpha, u, T):
    """The pre-clamp sigmoid of ``_relaxed`` (fp64 in, fp64 out)."""
    p, uc = _clamp_probs(alpha), _clamp_probs(u)
    return torch.sigmoid((uc.log() - (-uc).log1p() + p.log() - (-p).log1p()) / T)


ULP_MARGIN = 64


def gate_clamp_classes(alpha64, u64, T):
    """Split the relaxed gates of one layer by their clamps, from the fp64 pre-clamp sigmoid s and alpha:
    ``inside``: s and alpha more than ULP_MARGIN fp32 ulps inside both clamp bounds (the gate carries d gate / d alpha);
    ``outside``: s or alpha beyond a bound by more than ULP_MARGIN ulps (the clamp zeroes that derivative);
    the rest lie within ULP_MARGIN ulps of a bound, where the fp32 kernel and fp64 may put the gate on different sides."""
    s = _presig(alpha64, u64, T)
    lo, hi = float(F32.tiny), 1.0 - float(F32.eps)
    m_lo = ULP_MARGIN * float(np.spacing(np.float32(F32.tiny)))
    m_hi = ULP_MARGIN * float(np.spacing(np.float32(hi)))
    a_lo, a_hi = float(F32.eps), 1.0 - float(F32.eps)
    ma_lo, ma_hi = ULP_MARGIN * float(np.spacing(np.float32(a_lo))), ULP_MARGIN * float(np.spacing(np.float32(a_hi)))
    a_in = (alpha64 > a_lo + ma_lo) & (alpha64 < a_hi - ma_hi)
    a_out = (alpha64 < a_lo - ma_lo) | (alpha64 > a_hi + ma_hi)
    inside = a_in & (s > lo + m_lo) & (s < hi - m_hi)
    outside = a_out | (s < lo - m_lo) | (s > hi + m_hi)
    return inside, outside


class _GammaRep(torch.autograd.Function):
    """tau = x / b for a fixed standard-Gamma draw x, with d tau / d a = g(x, a) / b (g: scipy fp64 finite difference)."""

    @staticmethod
    def forward(ctx, a, b, x):
        from scipy import special, stats
        an, xn = a.detach().numpy(), x.numpy()
        h = 1e-6 * np.maximum(an, 1.0)
        dF = (special.gammainc(an + h, xn) - special.gammainc(an - h, xn)) / (2 * h)
        ctx.save_for_backward(b, x, torch.from_numpy(-dF / stats.gamma.pdf(xn, an)))
        return x / b

    @staticmethod
    def backward(ctx, g):
        b, x, gg = ctx.saved_tensors
        return g * gg / b, -g * x / b ** 2, None


def _chain(net, x, rng):
    """The training kernels on the same draws: sample_forward of the three layers at one Philox snapshot (a head of more than
    16 classes takes torch's log_softmax, as the ensemble does)."""
    h = x.view(-1, net.dims[0])
    head = "log_softmax" if net.dims[-1] <= 16 else None
    for k, l in enumerate((net.l1, net.l2, net.l3)):
        h, _, _ = l.sample_forward(h, activation="relu" if k < 2 else head, rng=rng)
    return h if head else F.log_softmax(h, dim=1)


class _Alpha32(torch.autograd.Function):
    """alpha = sigmoid(lambdal) held at a given fp32 value ``a`` -- the probability torch's fp32 RelaxedBernoulli and the
    kernels compute with -- with the sigmoid's derivative a (1 - a) at that value, as torch's sigmoid backward forms it.
    (Near alpha = 0 or 1 an fp32 ulp of alpha moves logit(alpha) by up to ~2e-4, which 1/T amplifies: an fp64 alpha would
    measure the rounding of the probability, not the kernels.)"""

    @staticmethod
    def forward(ctx, lam, a):
        ctx.save_for_backward(a)
        return a.clone()

    @staticmethod
    def backward(ctx, g):
        a, = ctx.saved_tensors
        return g * a * (1 - a), None


def alpha32_ulps(alpha, lambdal):
    """Largest distance, in fp32 ulps, of the kernels' fp32 alpha from the reference's fp32 1 / (1 + exp(-lambdal))
    (LBBNN-GP-MF.py:292) evaluated by torch on the CPU."""
    ref = (1 / (1 + torch.exp(-lambdal.detach().float().cpu()))).numpy()
    return float((np.abs(alpha.cpu().numpy().astype(np.float64) - ref) / np.spacing(ref)).max())


def layer_draws(ops, layer, rng, T):
    """Every draw of one layer's training step at the snapshot ``rng``, regenerated from the documented streams: uniforms,
    eps_w, eps_b (fp64, CPU) and the standard-Gamma draws behind tau_w and tau_b (fp64, CPU; tau = draw / rate)."""
    O, I, L = layer.out_features, layer.in_features, layer._layer_id
    return {"u": ops.philox_uniform(rng, ops.STREAM_GATE * 64 + L, O, I).double().cpu(),
            "eps_w": ops.philox_normal(rng, ops.STREAM_EPS_W * 64 + L, O, I).double().cpu(),
            "eps_b": ops.philox_normal(rng, ops.STREAM_EPS_B * 64 + L, 0, O).double().cpu(),
            "xw": ops.philox_std_gamma(rng, ops.STREAM_GAMMA_W * 64 + L, layer.weight_a).double().cpu(),
            "xb": ops.philox_std_gamma(rng, ops.STREAM_GAMMA_B * 64 + L, layer.bias_a).double().cpu()}


def exact_of(layer):
    return {"weight_prior": bool(layer.weight_prior.exact), "bias_prior": bool(layer.bias_prior.exact),
            "gamma_prior": bool(layer.gamma_prior.exact), "gamma": bool(layer.gamma.exact)}


def layer_oracle(x64, P64, d, T, hard_gates=None, exact=None, alpha32=None):
    """fp64 forward of one layer in training mode on the regenerated draws ``d`` (``layer_draws``): gates are
    ``_relaxed(alpha, u, T)`` (differentiable) or the given hard gates, alpha = sigmoid(lambdal) in fp64 or, given
    ``alpha32``, held at that fp32 probability (``_Alpha32``).  Returns (out, log_prior, log_q, gates)."""
    if alpha32 is None:
        alpha = 1 / (1 + torch.exp(-P64["lambdal"]))
    else:
        alpha = _Alpha32.apply(P64["lambdal"], alpha32.detach().double().cpu())
    cg = _relaxed(alpha, d["u"], T) if hard_gates is None else hard_gates
    tau_w = _GammaRep.apply(P64["weight_a"], P64["weight_b"], d["xw"])
    tau_b = _GammaRep.apply(P64["bias_a"], P64["bias_b"], d["xb"])
    o, lp, lq = orc.base_forward(x64, P64, cg, {"eps_w": d["eps_w"], "eps_b": d["eps_b"], "tau_w": tau_w, "tau_b": tau_b},
                                 mode="sample", gamma_alpha=alpha, exact=exact)
    return o, lp, lq, cg


def net_elbo_oracle(ops, net, x, y, rng, T, num_batches):
    """fp64 ``sample_elbo(draws="hip")`` of one sample at the snapshot ``rng``: (loss, log_prior, log_q, nll, P64 per layer).
    alpha is the kernels' fp32 alpha (``_Alpha32``), read from the layers after the hip call; hard gates (``gamma.exact``)
    are u < alpha."""
    h = x.reshape(-1, net.dims[0]).double().cpu()
    lp = lq = 0
    P = []
    for k, l in enumerate((net.l1, net.l2, net.l3)):
        P64 = {n: getattr(l, n).detach().double().cpu().requires_grad_(True) for n in l._names}
        d = layer_draws(ops, l, rng, T)
        hard = (d["u"] < l.alpha.double().cpu()).double() if l.gamma.exact else None
        h, lp_l, lq_l, _ = layer_oracle(h, P64, d, T, hard, exact_of(l), alpha32=l.alpha)
        h = torch.relu(h) if k < 2 else torch.log_softmax(h, dim=1)
        lp, lq = lp + lp_l, lq + lq_l
        P.append(P64)
    nll = F.nll_loss(h, y.cpu(), reduction="sum")
    return nll + (lq - lp) / num_batches, lp, lq, nll, P


def net_eval_oracle(ops, net, x, rng, gates):
    """fp64 evaluation forward of one ensemble member at the snapshot ``rng`` with the given per-layer gates."""
    h = x.reshape(-1, net.dims[0]).double().cpu()
    for k, l in enumerate((net.l1, net.l2, net.l3)):
        O, I, L = l.out_features, l.in_features, l._layer_id
        P64 = {n: getattr(l, n).detach().double().cpu() for n in l._names}
        noise = {"eps_w": ops.philox_normal(rng, ops.STREAM_EPS_W * 64 + L, O, I).double().cpu(),
                 "eps_b": ops.philox_normal(rng, ops.STREAM_EPS_B * 64 + L, 0, O).double().cpu()}
        h, _, _ = orc.base_forward(h, P64, gates[k].double().cpu(), noise, mode="sample", compute_lp=False)
        h = torch.relu(h) if k < 2 else torch.log_softmax(h, dim=1)
    return h
