"""References of the baseline LBBNN at depth, shared by tests/test_base_depth_gpu.py: the per-layer pieces of base_draw_ref
(``layer_draws``, ``layer_oracle``, ``exact_of``, ``_relaxed``, ``_rng``) composed over any number of layers.  A CPU fp64 result
is computed once per case and kept unchanged in ``_CACHE``."""
import numpy as np
import torch
import torch.nn.functional as F

from base_draw_ref import _relaxed, _rng, exact_of, layer_draws, layer_oracle      # noqa: F401  (re-exported)
from oracle import lbbnn_oracle as orc

NETS = {
    "n1": (12, 8),
    "n2": (12, 8, 5),
    "n3": (20, 16, 12, 3),
    "n4": (20, 16, 12, 8, 3),
    "n5": (20, 16, 12, 10, 7, 3),                    # two groups; widths with I % 4 != 0
    "n5c20": (20, 16, 12, 10, 7, 20),                # a 20-class head: torch's log_softmax
    "n9": (12, 16, 8, 12, 16, 8, 12, 16, 8, 4),      # three groups
    "n16": (8,) * 16 + (3,),                         # every stream id
}
_CACHE = {}


def make_net(bnn, dims, hard, seed):
    """A CPU network with parameters that let every layer reach the output: weight_mu ~ N(0, 4 / I),
    lambdal ~ U(-3, 3); everything else as constructed."""
    torch.manual_seed(seed)
    net = bnn.base.BayesianNetwork(dims)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for l in net._layers():
            l.weight_mu.copy_(torch.randn(l.weight_mu.shape, generator=g) * (2.0 / l.in_features ** 0.5))
            l.lambdal.copy_(torch.rand(l.lambdal.shape, generator=g) * 6 - 3)
            l.gamma.exact = hard
    return net


def data(dims, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, dims[0], generator=g), torch.randint(0, dims[-1], (B,), generator=g)


def chain(net, x, rng):
    """The training kernels on the same draws: sample_forward of every layer at one Philox snapshot (a head of more than 16
    classes takes torch's log_softmax, as the ensemble does)."""
    layers = net._layers()
    h = x.view(-1, net.dims[0])
    head = "log_softmax" if net.dims[-1] <= 16 else None
    for k, l in enumerate(layers):
        h, _, _ = l.sample_forward(h, activation="relu" if k < len(layers) - 1 else head, rng=rng)
    return h if head else F.log_softmax(h, dim=1)


def alpha_ref(layer):
    """The reference's fp32 alpha = 1 / (1 + exp(-lambdal)) (LBBNN-GP-MF.py:292), by torch on the CPU."""
    return 1 / (1 + torch.exp(-layer.lambdal.detach().float().cpu()))


def elbo_oracle(ops, net, x, y, rng, T, num_batches, alphas=None, scale=None, grad=True):
    """fp64 ``sample_elbo(draws="hip")`` of one sample at the snapshot ``rng``, any depth: dict(loss, lp, lq, nll, out, P).
    ``alphas``: per layer the fp32 alpha to hold (default ``alpha_ref``; the parity tests pass the kernels' own, read from the
    layers after the hip call).  Hard gates (``gamma.exact``) are u < alpha.  ``scale`` = (layer index, factor) multiplies that
    layer's weight_mu (the sensitivity check)."""
    layers = net._layers()
    h = x.reshape(-1, net.dims[0]).double().cpu()
    lp = lq = 0
    P, conds = [], []
    for k, l in enumerate(layers):
        P64 = {n: getattr(l, n).detach().double().cpu() for n in l._names}
        if scale is not None and scale[0] == k:
            P64["weight_mu"] = P64["weight_mu"] * scale[1]
        if grad:
            P64 = {n: v.requires_grad_(True) for n, v in P64.items()}
        a32 = (alpha_ref(l) if alphas is None else alphas[k]).detach().float().cpu()
        d = layer_draws(ops, l, rng, T)
        hard = (d["u"] < a32.double()).double() if l.gamma.exact else None
        h, lp_l, lq_l, cg = layer_oracle(h, P64, d, T, hard, exact_of(l), alpha32=a32)
        conds.append(min(pb_condition(cg.detach(), P64["pa"].detach(), P64["pb"].detach()),
                         pa_condition(P64["pa"].detach(), P64["pb"].detach())))
        h = torch.relu(h) if k < len(layers) - 1 else torch.log_softmax(h, dim=1)
        lp, lq = lp + lp_l, lq + lq_l
        P.append(P64)
    nll = F.nll_loss(h, y.cpu(), reduction="sum")
    return {"loss": nll + (lq - lp) / num_batches, "lp": lp, "lq": lq, "nll": nll, "out": h, "P": P, "prior_cond": conds}


def pa_condition(pa, pb):
    """The same for d log BetaBinomial / d pa, whose per-weight term does not depend on the gate: psi(pa + pb) - psi(1 + pa + pb)
    - psi(pa) = -1 / (pa + pb) - psi(pa), two numbers near -0.48 and -0.50 whose difference crosses zero at pa = 1.064 (pb = 1.03)
    -- inside the U(1, 1.1) the parameters are created from."""
    psi = torch.special.digamma
    c = psi(pa + pb) - psi(1 + pa + pb)
    return float((c - psi(pa)).abs() / (c.abs() + psi(pa).abs()))


def pb_condition(g, pa, pb):
    """|sum t| / sum |t| of the per-weight terms t = d log BetaBinomial(g; pa, pb) / d pb (LBBNN-GP-MF.py:162-173) of one layer:
    how much of its terms the scalar gradient d log_prior / d pb keeps.  With pa, pb near 1 a shut gate contributes about
    +1 / pb - 1 / (pa + pb) = +0.47 and an open one -1 / (pa + pb) = -0.48: a layer with half its gates open cancels."""
    psi = torch.special.digamma
    t = psi(1 + pb - g) + psi(pa + pb) - psi(1 + pa + pb) - psi(pb)
    return float(t.sum().abs() / t.abs().sum())


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64).cpu(), torch.as_tensor(b, dtype=torch.float64).cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def sensitivity(ops, net, x, y, rng, T, num_batches):
    """The smallest move, over the layers, of the fp64 oracle's output (the log-probabilities) when ONE layer's weight_mu is
    scaled by 1.01 (relative, conftest.rel_err's measure); and the move per layer."""
    with torch.no_grad():
        ref = elbo_oracle(ops, net, x, y, rng, T, num_batches, grad=False)
        moves = []
        for i in range(len(net._layers())):
            r = elbo_oracle(ops, net, x, y, rng, T, num_batches, scale=(i, 1.01), grad=False)
            moves.append(rel(r["out"], ref["out"]))
    return min(moves), moves


def eval_oracle(ops, net, x, rng, gates, scale=None):
    """fp64 evaluation forward of one ensemble member at the snapshot ``rng`` with the given per-layer gates, any depth.
    ``scale`` = (layer index, factor) multiplies that layer's weight_mu."""
    layers = net._layers()
    h = x.reshape(-1, net.dims[0]).double().cpu()
    for k, l in enumerate(layers):
        O, I, L = l.out_features, l.in_features, l._layer_id
        P64 = {n: getattr(l, n).detach().double().cpu() for n in l._names}
        if scale is not None and scale[0] == k:
            P64["weight_mu"] = P64["weight_mu"] * scale[1]
        noise = {"eps_w": ops.philox_normal(rng, ops.STREAM_EPS_W * 64 + L, O, I).double().cpu(),
                 "eps_b": ops.philox_normal(rng, ops.STREAM_EPS_B * 64 + L, 0, O).double().cpu()}
        h, _, _ = orc.base_forward(h, P64, gates[k].double().cpu(), noise, mode="sample", compute_lp=False)
        h = torch.relu(h) if k < len(layers) - 1 else torch.log_softmax(h, dim=1)
    return h


def eval_sensitivity(ops, net, x, rng, gates, ref):
    """The smallest move, over the layers, of ``eval_oracle``'s output ``ref`` when ONE layer's weight_mu is scaled by 1.01."""
    return min(rel(eval_oracle(ops, net, x, rng, gates, scale=(i, 1.01)), ref) for i in range(len(net._layers())))


def mean_oracle(net, x):
    """fp64 posterior-mean forward (mode 2: weight = alpha * mu with alpha = sigmoid(lambdal), LBBNN-GP-MF.py:369-374, :413)."""
    layers = net._layers()
    h = x.reshape(-1, net.dims[0]).double().cpu()
    for k, l in enumerate(layers):
        P64 = {n: getattr(l, n).detach().double().cpu() for n in l._names}
        alpha = 1 / (1 + torch.exp(-P64["lambdal"]))
        h, _, _ = orc.base_forward(h, P64, None, {}, mode="mean", compute_lp=False, alpha_attr=alpha)
        h = torch.relu(h) if k < len(layers) - 1 else torch.log_softmax(h, dim=1)
    return h


def fold32(values):
    """((0 + v0) + v1) + ... in fp32 on the CPU."""
    s = np.float32(0.0)
    for v in values:
        s = np.float32(s + np.float32(float(v)))
    return s
