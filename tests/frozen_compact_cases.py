"""Shared inputs of the compact median-probability model tests (tests/test_frozen_compact_host.py, _gpu.py).

Per layer i of a network, lambdal = seeded U(-3, 3) pushed at least 2e-3 away from the cut (0: threshold 0.5); then, in
this order:
  1. every unit u of boundary i (the layer's inputs) with u % 3 == 1 gets column u of layer i set to -2: nobody consumes it;
  2. for i < n-1, column 0 of layer i is -2 except in the rows o % 3 == 1, which are +2: column 0 is kept only by rows that
     rule 1 of the next layer leaves unconsumed -- the cascade case, unit 0 must be dropped;
  3. for i < n-1, row 2 of layer i is all -2: a needed unit with no kept input, which must stay (it emits relu(bias + noise)).
``lambdals`` asserts, from torch alone (brute-force path reachability, the products of the keep matrices): needed < width at
every boundary below the outputs, unit 0 unneeded at boundaries 0 .. n-2, unit 2 needed at boundaries 1 .. n-1, and a needed
count that is no multiple of 8 at some boundary."""
import torch

# (family, dims, planar transforms, head)
CASES = [("lrt", (64, 48, 40, 20), 0, "log_softmax"), ("mnf", (64, 48, 40, 20), 2, "log_softmax"),
         ("mnf", (20, 16, 12, 3), 4, "log_softmax"),              # every compact O <= 16: all layers fp32
         ("lrt", (50, 37, 29, 3), 0, "log_softmax"),              # full model: chain path; compact model: member path
         ("lrt", (784, 400, 600, 10), 0, "log_softmax"), ("mnf", (784, 400, 600, 10), 2, "log_softmax"),
         ("lrt", (32, 24, 24, 24, 24, 10), 0, "log_softmax"),     # five layers: two layer groups
         ("lrt", (20, 1), 0, "sigmoid")]                          # only the inputs shrink
IDS = ["%s-%s%s" % (f, "-".join(map(str, d)), "-T%d" % t if t else "") for f, d, t, _ in CASES]

# the table of the feature's description: needed units, live units per boundary
TABLE = {(64, 48, 40, 20): ((42, 31, 27, 20), (48, 32, 32, 20)),
         (50, 37, 29, 3): ((32, 24, 19, 3), (32, 24, 24, 3)),
         (784, 400, 600, 10): ((522, 266, 400, 10), (528, 272, 400, 10))}


def brute_need(masks):
    """need[b] by path counting: unit j of boundary b is needed iff the product K_{n-1} ... K_b has a nonzero in column j."""
    n = len(masks)
    need = [None] * (n + 1)
    need[n] = torch.ones(masks[-1].shape[0], dtype=torch.bool)
    prod = None
    for i in range(n - 1, -1, -1):
        k = masks[i].double().cpu()
        prod = k if prod is None else prod @ k             # (outputs, width of boundary i): number of kept paths
        need[i] = prod.sum(0) > 0
    return need


def expected_live_sizes(need, align=8):
    n = len(need) - 1
    out = []
    for b, nd in enumerate(need):
        w, c = nd.numel(), int(nd.sum())
        out.append(w if b == n else min(w, max(align, -(-c // align) * align)))
    return out


def lambdals(dims, seed=7, cut=0.0):
    """The lambdal of every layer (CPU fp32) and the keep masks, with the module docstring's assertions made."""
    n = len(dims) - 1
    g = torch.Generator().manual_seed(seed)
    lams = []
    for i in range(n):
        O, I = dims[i + 1], dims[i]
        lam = torch.empty(O, I).uniform_(-3, 3, generator=g)
        d = lam - cut
        lam = torch.where(d.abs() < 2e-3, cut + torch.where(d < 0, -2e-3, 2e-3), lam)
        lam[:, 1::3] = -2.0                                  # 1. units u % 3 == 1 of boundary i: unconsumed
        if i < n - 1:
            lam[:, 0] = -2.0                                 # 2. column 0 kept by unneeded rows only
            lam[1::3, 0] = 2.0
            lam[2, :] = -2.0                                 # 3. a needed unit without kept inputs
        assert float((lam - cut).abs().min()) >= 1e-3
        lams.append(lam)
    masks = [lam > cut for lam in lams]
    need = brute_need(masks)
    counts = [int(nd.sum()) for nd in need]
    for b in range(n):
        assert counts[b] < dims[b], (b, counts[b])
    for b in range(n - 1):
        assert not bool(need[b][0]), b
        assert bool(need[b + 1][2]) and not bool(masks[b][2].any()), b
    assert any(c % 8 for c in counts[:n]), counts
    return lams, masks


def apply(net, lams):
    with torch.no_grad():
        for l, lam in zip(net._layers(), lams):
            l.lambdal.copy_(lam.to(l.lambdal.device))
