"""Shared inputs and references of the threshold-sweep tests (tests/test_threshold_sweep_host.py, _gpu.py).

``lambdals(dims, thresholds, seed)``: per layer lambdal = seeded U(-span, span) (span 6), pushed at least 2e-3 away from every
cut logit(threshold_j); then, in this order (a later rule wins where two meet), with cuts c_0 < ... < c_{K-1}:
  1. row 0 below every cut: empty at every level (a layer of ONE row keeps its random row);
  2. row 1 above every cut: full at every level;
  3. row 2 with exactly one weight (column I // 2), kept at level 0 only;
  4. in layers with I > 70, row 3 keeps 65 weights at level 0 (columns 1 .. 65), 9 at level 1 (columns 1 .. 9) and 8 at level 2
     (columns 1 .. 8), where those levels exist, and none above: one past a wave, one past a chunk of the layer kernel, a chunk.
``empty_last=True`` (the set that ends in 0.99, span 3: logit(0.99) = 4.6): "every cut" of rules 2 to 4 means every cut but
the last, and the last level keeps no weight in any layer.  Every rule is asserted here from torch alone, on the CPU.

The CSR of a level and the float64 member come from tests/frozen_sparse_ref.py (``csr_of``, ``member_from_csr``)."""
import torch

from frozen_sparse_ref import cut_of

# (family, dims, planar transforms, head)
CASES = [("lrt", (64, 48, 40, 20), 0, "log_softmax"),             # O > 16: torch's log_softmax
         ("mnf", (64, 48, 40, 20), 2, "log_softmax"),
         ("lrt", (50, 37, 29, 3), 0, "log_softmax"),              # nothing divisible by 4; the in-kernel log_softmax
         ("lrt", (100, 20, 1), 0, "sigmoid"),
         ("mnf", (8, 32, 2), 2, "identity"),
         ("lrt", (32, 24, 24, 24, 24, 10), 0, "log_softmax")]     # five layers: two layer groups
IDS = ["%s-%s%s" % (f, "-".join(map(str, d)), "-T%d" % t if t else "") for f, d, t, _ in CASES]
BS = [(1, 3), (65, 2), (130, 1), (100, 10)]                       # both rows-per-lane forms, an odd B

# name -> (thresholds, span of the uniform lambdal, whether the last level is empty)
SETS = {"one": ((0.5,), 6.0, False),
        "four": ((0.3, 0.5, 0.9, 0.99), 3.0, True),
        "sixteen": (tuple(0.05 + 0.06 * k for k in range(16)), 6.0, False)}


def batch_sizes(name):
    """The (B, S) of a threshold set: sixteen levels take S <= 2."""
    return [bs for bs in BS if bs[1] <= 2] if name == "sixteen" else BS


def cuts_of(thresholds):
    return [cut_of(t) for t in thresholds]


def keep_masks(lams, thresholds):
    """[level][layer] bool masks lambdal > cut_j, compared in fp32."""
    return [[lam > torch.tensor(c, dtype=torch.float32) for lam in lams] for c in cuts_of(thresholds)]


def lambdals(dims, thresholds, seed=7, span=6.0, empty_last=False):
    """The lambdal of every layer (CPU fp32) and the keep masks [level][layer], with the module docstring's assertions made."""
    cuts = cuts_of(thresholds)
    K = len(cuts)
    assert all(a < b for a, b in zip(cuts, cuts[1:])) and all(b - a > 4e-3 for a, b in zip(cuts, cuts[1:]))
    Ke = K - 1 if empty_last else K                               # the levels the rules speak of
    assert Ke >= 1
    lo = cuts[0] - 2.0
    top = 0.5 * (cuts[Ke - 1] + cuts[K - 1]) if empty_last else cuts[K - 1] + 2.0

    def upto(j):
        """A value kept at the levels 0 .. j and at no other."""
        j = min(j, Ke - 1)
        return top if j == Ke - 1 else 0.5 * (cuts[j] + cuts[j + 1])

    g = torch.Generator().manual_seed(seed)
    lams = []
    for i in range(len(dims) - 1):
        O, I = dims[i + 1], dims[i]
        lam = torch.empty(O, I).uniform_(-span, span, generator=g)
        for c in cuts:
            d = lam - c
            lam = torch.where(d.abs() < 2e-3, c + torch.where(d < 0, -2e-3, 2e-3), lam)
        if O > 1:
            lam[0, :] = lo
            lam[1, :] = top
        if O > 2:
            lam[2, :] = lo
            lam[2, I // 2] = upto(0)
        if I > 70:
            assert O > 3
            lam[3, :] = lo
            lam[3, 1:66] = upto(0)
            lam[3, 1:10] = upto(1)
            lam[3, 1:9] = upto(2)
        assert min(float((lam - c).abs().min()) for c in cuts) >= 1e-3
        lams.append(lam)
    masks = keep_masks(lams, thresholds)
    for j in range(K):
        for i, keep in enumerate(masks[j]):
            O, I = keep.shape
            rows = keep.sum(1)
            live = j < Ke
            if empty_last and not live:
                assert int(keep.sum()) == 0, (i, j)
                continue
            if O > 1:
                assert int(rows[0]) == 0 and int(rows[1]) == I, (i, j)
            if O > 2:
                assert int(rows[2]) == (1 if j == 0 else 0) and bool(keep[2, I // 2]) == (j == 0), (i, j)
            if I > 70:
                assert int(rows[3]) == {0: 65, 1: 9, 2: 8}.get(j, 0), (i, j, int(rows[3]))
            if j:
                assert bool((masks[j - 1][i] | ~keep).all())      # nested: kept at level j, kept at level j - 1
    return lams, masks
