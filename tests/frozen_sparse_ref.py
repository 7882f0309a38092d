"""Shared inputs and references of the sparse median-probability model tests (tests/test_frozen_sparse_host.py, _gpu.py).

Per layer of a network, lambdal = seeded U(-3, 3) pushed at least 2e-3 away from the cut logit(threshold); then, in this
order (a later rule wins where two meet):
  1. row 0 all below the cut: an empty row of a needed unit (a layer of ONE row keeps its random row: the model would be a
     constant otherwise);
  2. column 0 all below the cut;
  3. row 1 all above the cut: a full row (it keeps column 0: the only row that does);
  4. row 2 with exactly one kept weight, at column I // 2;
  5. in layers with I > 70, row 3 with exactly 65 kept weights (columns 1 .. 65): one past a wave.
``lambdals`` asserts, from torch alone, these five facts and, for layers of at least 192 weights, a kept share of 0.25 .. 0.6
at threshold 0.5 and of 0.05 .. 0.25 at threshold 0.9.

``csr_of``: the CSR of a layer from ``nonzero`` of ``lambdal > cut`` (row-major, so columns ascend within a row);
``member_from_csr``: one member's forward in float64 from such CSRs."""
import torch

THRESHOLDS = (0.5, 0.9)

# (family, dims, planar transforms, head)
CASES = [("lrt", (64, 48, 40, 20), 0, "log_softmax"), ("mnf", (64, 48, 40, 20), 2, "log_softmax"),
         ("mnf", (20, 16, 12, 3), 4, "log_softmax"),
         ("lrt", (50, 37, 29, 3), 0, "log_softmax"),              # in_features % 4 != 0 and out_features % 4 != 0
         ("lrt", (2048, 64, 32, 10), 0, "log_softmax"),           # long rows
         ("lrt", (784, 400, 600, 10), 0, "log_softmax"), ("mnf", (784, 400, 600, 10), 2, "log_softmax"),
         ("lrt", (32, 24, 24, 24, 24, 10), 0, "log_softmax"),     # five layers: two layer groups
         ("lrt", (20, 1), 0, "sigmoid"),
         ("mnf", (8, 32, 2), 2, "identity")]
IDS = ["%s-%s%s" % (f, "-".join(map(str, d)), "-T%d" % t if t else "") for f, d, t, _ in CASES]
BIG = (784, 400, 600, 10)                                         # evaluated at (B, S) = (100, 10) only
BS = [(1, 10), (100, 10), (257, 1), (65, 3)]


def batch_sizes(dims):
    return [(100, 10)] if tuple(dims) == BIG else BS


def cut_of(threshold):
    """logit(threshold) as the fp32 value the kernels compare with."""
    return float(torch.logit(torch.tensor(threshold, dtype=torch.float64)).float())


def lambdals(dims, threshold=0.5, seed=7):
    """The lambdal of every layer (CPU fp32) and the keep masks, with the module docstring's assertions made."""
    cut = cut_of(threshold)
    g = torch.Generator().manual_seed(seed)
    lams = []
    for i in range(len(dims) - 1):
        O, I = dims[i + 1], dims[i]
        lam = torch.empty(O, I).uniform_(-3, 3, generator=g)
        d = lam - cut
        lam = torch.where(d.abs() < 2e-3, cut + torch.where(d < 0, -2e-3, 2e-3), lam)
        lo, hi = cut - 2.0, cut + 2.0
        if O > 1:
            lam[0, :] = lo
        lam[:, 0] = lo
        if O > 1:
            lam[1, :] = hi
        if O > 2:
            lam[2, :] = lo
            lam[2, I // 2] = hi
        if I > 70:
            assert O > 3
            lam[3, :] = lo
            lam[3, 1:66] = hi
        assert float((lam - cut).abs().min()) >= 1e-3
        keep = lam > torch.tensor(cut, dtype=torch.float32)
        rows = keep.sum(1)
        if O > 1:
            assert int(rows[0]) == 0 and int(rows[1]) == I
            assert int(keep[:, 0].sum()) == 1 and bool(keep[1, 0])
        else:
            assert not bool(keep[:, 0].any())
        if O > 2:
            assert int(rows[2]) == 1 and bool(keep[2, I // 2])
        if I > 70:
            assert int(rows[3]) == 65
        if O * I >= 192:
            share = float(keep.sum()) / (O * I)
            bounds = {0.5: (0.25, 0.6), 0.9: (0.05, 0.25)}[threshold]
            assert bounds[0] <= share <= bounds[1], (O, I, threshold, share)
        lams.append(lam)
    return lams, [lam > torch.tensor(cut, dtype=torch.float32) for lam in lams]


def apply(net, lams):
    with torch.no_grad():
        for l, lam in zip(net._layers(), lams):
            l.lambdal.copy_(lam.to(l.lambdal.device))


def csr_of(lam, cut):
    """(row_ptr int32 (O + 1), col int32 (nnz), keep) of one layer; NaN is never kept (the comparison is false)."""
    keep = lam.float() > torch.tensor(cut, dtype=torch.float32)
    nz = keep.nonzero()                                       # row-major: columns ascend within a row
    row_ptr = torch.zeros(lam.shape[0] + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(keep.sum(1), 0)
    return row_ptr.to(torch.int32), nz[:, 1].to(torch.int32), keep


def csr_brute(lam, cut):
    """The same CSR by two Python loops."""
    cut32 = torch.tensor(cut, dtype=torch.float32)
    row_ptr, col = [0], []
    for o in range(lam.shape[0]):
        for j in range(lam.shape[1]):
            if bool(lam[o, j].float() > cut32):
                col.append(j)
        row_ptr.append(len(col))
    return torch.tensor(row_ptr, dtype=torch.int32), torch.tensor(col, dtype=torch.int32)


def exclusive_scan(kept_rows):
    out = [0]
    for k in kept_rows.tolist():
        out.append(out[-1] + int(k))
    return torch.tensor(out, dtype=torch.int32)


def decode(row_ptr, col, values, O, I):
    """The dense (O, I) matrix of a CSR (zeros where nothing is kept), in the dtype of ``values``."""
    rows = torch.repeat_interleave(torch.arange(O), (row_ptr[1:] - row_ptr[:-1]).long())
    out = torch.zeros(O, I, dtype=values.dtype)
    out[rows, col.long()] = values
    return out


def member_from_csr(x, layers, head="log_softmax", stochastic=True):
    """One member in float64.  ``layers``: per layer a dict with the CSR (row_ptr, col, mean, var), bias_mu, bias_var, z (None
    or (I,)) and eps (None or (B, O)).  mean = bias_mu + sum_k mean[k] z[col[k]] a[col[k]], var = bias_var + sum_k var[k]
    a[col[k]]^2, out = mean + sqrt(var) eps; ReLU between the layers, then the head."""
    h = x.double()
    for i, l in enumerate(layers):
        O, I = l["bias_mu"].numel(), h.shape[1]
        m = decode(l["row_ptr"], l["col"], l["mean"].double(), O, I)
        if l.get("z") is not None:
            m = m * l["z"].double()[None, :]
        out = h @ m.T + l["bias_mu"].double()
        if stochastic:
            v = decode(l["row_ptr"], l["col"], l["var"].double(), O, I)
            out = out + torch.sqrt((h * h) @ v.T + l["bias_var"].double()) * l["eps"].double()
        h = torch.relu(out) if i < len(layers) - 1 else out
    if head == "sigmoid":
        return torch.sigmoid(h)
    return h if head == "identity" else torch.log_softmax(h, dim=1)
