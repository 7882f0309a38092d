"""numpy float64 restatement of evaluate.explain (include/lbbnn.h, lbbnn_explain_step): the exact local linear model of a ReLU
chain on fixed operands,

    logits[b, c] = sum_i J[b, c, i] x[b, i] + k[b, c],   J(b) = W_L D_{L-1}(b) .. D_1(b) W_1,   D_l(b) = diag(masks[l][b])

The masks are an ARGUMENT: a unit whose pre-activation is within rounding of 0 can then not flip the whole Jacobian between the
device's fp32 forward and this fp64 one.  ``relu_masks`` gives the chain's own (fp64) masks and pre-activations.

Also here: the networks of the GPU tier (``CASES``, ``build_net``) -- built on the CPU from a seed, so the host tier checks the
choice of seeds (few units near 0) without a device -- and the fp64 operands of a frozen model's snapshot."""
import numpy as np
import torch


def relu_masks(Ws, bs, x):
    """(masks, pre): per HIDDEN layer the (B, O_l) bool pattern a_l > 0 and the fp64 pre-activations a_l of the chain's own
    forward h_l = relu(h_{l-1} W_l^T + b_l)."""
    h = np.asarray(x, dtype=np.float64)
    masks, pre = [], []
    for W, b in zip(Ws[:-1], bs[:-1]):
        a = h @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        pre.append(a)
        masks.append(a > 0)
        h = np.where(a > 0, a, 0.0)
    return masks, pre


def explain_ref(Ws, bs, x, masks):
    """J (B, C, I), contributions (B, C, I) = J * x, intercept (B, C) and logits (B, C) of the chain under the GIVEN masks
    (per hidden layer (B, O_l) bool).  The logits come from the masked forward, not from the sum: ``logits - (contributions.sum(-1)
    + intercept)`` is this reference's own completeness error."""
    Ws = [np.asarray(W, dtype=np.float64) for W in Ws]
    bs = [np.asarray(b, dtype=np.float64) for b in bs]
    x = np.asarray(x, dtype=np.float64)
    masks = [np.asarray(m, dtype=bool) for m in masks]
    n, B = len(Ws), x.shape[0]
    assert len(masks) == n - 1
    h = x
    for l in range(n):
        a = h @ Ws[l].T + bs[l]
        h = a * masks[l] if l < n - 1 else a
    logits = h
    G = np.broadcast_to(Ws[-1][None], (B,) + Ws[-1].shape).copy()          # (B, C, width of h_{L-1})
    k = np.broadcast_to(bs[-1][None], (B, Ws[-1].shape[0])).copy()
    for l in range(n - 2, -1, -1):
        G = G * masks[l][:, None, :]
        k = k + G @ bs[l]
        G = G @ Ws[l]
    return dict(J=G, contributions=G * x[:, None, :], intercept=k, logits=logits)


# ------------------------------------------------------------------------------------------------ the GPU tier's networks
# (dims, head, family, B, seed); lambdal ~ N(0, 3): a median probability model keeps about half its weights
CASES = {
    "20-1": ((20, 1), "sigmoid", "lrt", 7, 101),
    "12-24-8-3": ((12, 24, 8, 3), "log_softmax", "lrt", 5, 102),
    "8-32-2": ((8, 32, 2), "identity", "lrt", 70, 103),
    "13-9-5-2": ((13, 9, 5, 2), "log_softmax", "lrt", 3, 104),
    "12-24-3-mnf": ((12, 24, 3), "log_softmax", "mnf", 5, 105),
    "8-16x4-4": ((8, 16, 16, 16, 16, 4), "log_softmax", "lrt", 65, 106),
    # beyond the issue's list: a shape whose hidden layers the bf16 hi | lo format takes (lbbnn_explain_operand)
    "16-24-40-3": ((16, 24, 40, 3), "log_softmax", "lrt", 6, 107),
}
NEAR_ZERO = 1e-4          # a unit is left out of the mask comparison when |a| < NEAR_ZERO * max|a| of its layer
NEAR_ZERO_CAP = 0.01      # ... and at most this share of all units of a case may be


def build_net(bnn, name):
    """(net on the CPU, x (B, dims[0]) on the CPU) of a case: lambdal ~ N(0, 3), bias_mu ~ N(0, 0.5) (non-zero), x ~ N(0, 1),
    weight_mu ~ N(0, 4 / in_features), an MNF layer's q0_mean ~ N(1, 0.1), from the case's seed alone."""
    dims, head, family, B, seed = CASES[name]
    torch.manual_seed(seed)
    if family == "mnf":
        net = bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar", head=head)
    else:
        net = bnn.lrt.BayesianNetwork(dims, head=head)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.copy_(torch.randn(l.lambdal.shape, generator=g) * 3.0)
            l.bias_mu.copy_(torch.randn(l.bias_mu.shape, generator=g) * 0.5)
            # Every error of the GPU tier is measured against max|contributions|, so the input path must not vanish beside the
            # bias path: the fp32 rounding of a logit of size 1 (6e-8) reads as 5e-3 against contributions of 1e-5.  As
            # constructed weight_mu ~ U(+-0.2) (MNF: U(+-0.01)) shrinks the signal layer by layer -- five layers, or two MNF
            # layers, leave contributions 1e3 to 1e4 times smaller than the intercept.  weight_mu ~ N(0, 4 / in_features) keeps
            # the activations' scale through a layer that prunes half its weights and a ReLU that zeroes half its units ...
            l.weight_mu.copy_(torch.randn(l.weight_mu.shape, generator=g) * (4.0 / l.in_features) ** 0.5)
            if family == "mnf":
                # ... and z around 1, as a trained MNF layer has it (as constructed q0_mean ~ N(0, 0.01): z ~ 0.1 per layer)
                l.q0_mean.copy_(1.0 + 0.1 * torch.randn(l.q0_mean.shape, generator=g))
    x = torch.randn(B, dims[0], generator=g)
    return net, x


def mpm_operands(net):
    """fp64 (W_l, b_l) of the median probability model of an LRT network on the CPU: mu where lambdal > 0, else 0."""
    Ws = [np.where(l.lambdal.detach().numpy() > 0, l.weight_mu.detach().numpy(), 0.0).astype(np.float64) for l in net._layers()]
    bs = [l.bias_mu.detach().numpy().astype(np.float64) for l in net._layers()]
    return Ws, bs


def near_zero_share(pre):
    """The share of hidden units, over all layers and rows, whose fp64 pre-activation lies within NEAR_ZERO * max|a| of 0."""
    near = sum(int((np.abs(a) < NEAR_ZERO * np.abs(a).max()).sum()) for a in pre)
    total = sum(a.size for a in pre)
    return near / total if total else 0.0


def snapshot_operands(fz, z=None):
    """fp64 (W_l, b_l) from a frozen model's own buffers, as the forward's products read them: e0 for an fp32 LRT layer;
    (e0 * z) in fp32 for an MNF layer (``z``: what explain returned; a compact model reads z at its live columns); and the
    bf16 hi + lo of that value where the layer's operand is in the split format."""
    Ws, bs = [], []
    for i in range(fz.n_layers):
        O, I = fz.dims[i + 1], fz.dims[i]
        w = getattr(fz, "e0_%d" % i)[:, :I].clone()
        if z is not None:
            zi = z[i]
            if fz.compact:
                zi = zi[getattr(fz, "live_%d" % i).long()]
            w = w * zi[None, :]
        if fz._split[i]:
            hi = w.bfloat16().float()
            w = hi + (w - hi).bfloat16().float()
        Ws.append(w.double().cpu().numpy())
        bs.append(getattr(fz, "bias_mu_%d" % i).double().cpu().numpy())
    return Ws, bs
