"""Shared inputs and references of the baseline family's sparse median-probability model tests
(tests/test_base_sparse_host.py, _gpu.py): ``evaluate.freeze_base(net, "mpm", sparse=True)``.

Inputs: tests/frozen_sparse_ref.py's lambdal structures (an empty row, a pruned column 0, a full row, a row with one kept weight
and, for I > 70, a row of 65; every lambdal at least 1e-3 from the cut) applied to a ``base.BayesianNetwork``.  For these
shapes ``sigmoid(lambdal) > threshold`` and ``lambdal > logit(threshold)`` agree everywhere and the smallest |sigmoid(lambdal) -
threshold| is 1.8e-4, a thousand times an fp32 sigmoid's error: the pattern is the same whichever rule a reference uses.

``head == "identity"``: the baseline NETWORK has the log_softmax and the sigmoid head only; the frozen model class takes the
identity head too (the raw logits), so that case binds a ``SparseFrozenBaseNetwork`` with ``head="identity"`` to a log_softmax
network (``freeze_sparse``), and its dense twin likewise."""
import torch

import frozen_sparse_ref as sr

# (dims, head): each the smallest that reaches its case
CASES = [((13, 9, 3), "log_softmax"),                    # I % 4 != 0, a last Philox quad of one column, O % 4 != 0 (bias quads)
         ((76, 12, 5), "log_softmax"),                   # the 65-kept row; a second, partial 64-column step
         ((50, 37, 29, 3), "log_softmax"),               # no width a multiple of 4
         ((16, 16, 16, 16, 16, 4), "log_softmax"),       # five layers: two launch groups
         ((8, 12, 20, 18), "log_softmax"),               # C > 16: the head is a launch of its own
         ((20, 1), "sigmoid"),                           # one layer, one row; at 0.9 one kept weight
         ((8, 32, 2), "identity")]
IDS = ["-".join(map(str, d)) + ("" if h == "log_softmax" else "-" + h) for d, h in CASES]
BIG = (784, 400, 600, 10)                                # the pack and the draw only, at (B, S) = (100, 10)


def make_net(bnn, dev, dims, head, threshold, seed=11):
    """A baseline network with tests/frozen_sparse_ref.py's lambdal structure at ``threshold``; weight_mu scaled so that the
    input path does not vanish beside the bias path (as tests/test_sparse_explain_gpu.py)."""
    torch.manual_seed(seed)
    net = bnn.base.BayesianNetwork(dims, head="sigmoid" if head == "sigmoid" else "log_softmax")
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for l in net._layers():
            l.weight_mu.copy_(torch.randn(l.weight_mu.shape, generator=g) * (4.0 / l.in_features) ** 0.5)
            l.bias_mu.copy_(torch.randn(l.bias_mu.shape, generator=g) * 0.5)
    net = net.to(dev).eval()
    sr.apply(net, sr.lambdals(dims, threshold)[0])
    return net


def freeze_sparse(ev, net, head, threshold):
    if head != "identity":
        return ev.freeze_base(net, "mpm", threshold=threshold, sparse=True)
    fz = ev.SparseFrozenBaseNetwork(net.dims, threshold, device=net._layers()[0].weight_mu.device, head="identity")
    fz.eval()
    return fz._bind(net)


def freeze_dense(ev, net, head, threshold):
    if head != "identity":
        return ev.freeze_base(net, "mpm", threshold=threshold)
    fz = ev.FrozenBaseNetwork(net.dims, "mpm", threshold, device=net._layers()[0].weight_mu.device, head="identity")
    fz.eval()
    return fz._bind(net)


def rows_of(row_ptr):
    """The row of every CSR slot."""
    O = row_ptr.numel() - 1
    return torch.repeat_interleave(torch.arange(O, device=row_ptr.device), (row_ptr[1:] - row_ptr[:-1]).long())


def same_bits(a, b):
    """Bitwise equality of two fp32 tensors, a zero of either sign equal to a zero of the other."""
    ia, ib = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(((ia == ib) | (((ia & 0x7FFFFFFF) == 0) & ((ib & 0x7FFFFFFF) == 0))).all())


def head64(h, head, log_probs=False):
    if head == "identity":
        return h
    if head == "sigmoid":
        if log_probs:
            return torch.cat([torch.nn.functional.logsigmoid(-h), torch.nn.functional.logsigmoid(h)], dim=-1)
        return torch.sigmoid(h)
    return torch.log_softmax(h, dim=-1)


def forward64(x, csrs, weights, biases, dims, head, log_probs=False):
    """One member in fp64 on the CPU from (nnz,) weight vectors: the dense decode of every layer, ReLU between, the head."""
    h = x.double().cpu()
    n = len(csrs)
    for i, (row_ptr, col) in enumerate(csrs):
        W = sr.decode(row_ptr.cpu(), col.cpu(), weights[i].double().cpu(), dims[i + 1], dims[i])
        h = h @ W.T + biases[i].double().cpu()
        if i < n - 1:
            h = torch.relu(h)
    return head64(h, head, log_probs)
