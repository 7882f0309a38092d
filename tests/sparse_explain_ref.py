"""Shared inputs and float64 references of the sampled-weight member explanations (evaluate.explain_ensemble;
tests/test_sparse_explain_host.py, _gpu.py).

A member has explicit weights on the kept pattern of a sparse median-probability model: per CSR slot w = mean * z[col] +
sqrt(var) * eps, per unit b = bias_mu + sqrt(bias_var) * eps.  It is an ordinary ReLU network, so tests/explain_ref.py's local
linear model applies to its dense decode; the masks are an argument there for the reason given there.

Inputs: tests/frozen_sparse_ref.py -- its CASES without the 784-400-600-10 pair (BIG), its lambdal structures (an empty row, a
column with one entry, a full row, a row of 65, widths that are no multiple of 4, five layers, 20 -> 1, 8 -> 32 -> 2)."""
import numpy as np
import torch

import explain_ref as er
import frozen_sparse_ref as sr

CASES = [c for c in sr.CASES if tuple(c[1]) != sr.BIG]
IDS = [i for i, c in zip(sr.IDS, sr.CASES) if tuple(c[1]) != sr.BIG]
# a single row; one past a wave; one past the two-row tile, with an even remainder
BS = [(1, 3), (65, 3), (130, 2)]


def transpose_brute(row_ptr, col, I):
    """(col_ptr, trow, tslot) of a CSR by Python loops over a dense (O, I) table of slots: column by column, rows ascending,
    tslot the CSR slot of the entry."""
    O = row_ptr.numel() - 1
    rp, cl = row_ptr.tolist(), col.tolist()
    slot = [[-1] * I for _ in range(O)]
    for o in range(O):
        for k in range(rp[o], rp[o + 1]):
            assert slot[o][cl[k]] < 0
            slot[o][cl[k]] = k
    col_ptr, trow, tslot = [0], [], []
    for i in range(I):
        for o in range(O):
            if slot[o][i] >= 0:
                trow.append(o)
                tslot.append(slot[o][i])
        col_ptr.append(len(trow))
    i32 = torch.int32
    return torch.tensor(col_ptr, dtype=i32), torch.tensor(trow, dtype=i32), torch.tensor(tslot, dtype=i32)


def draw_ref(mean, var, eps, zcol=None):
    """(w, bound) in float64: w = mean * z[col] + sqrt(var) * eps and the fp32 bound 4 * 2^-24 * (|mean z| + sqrt(var) |eps|): one
    1-ulp square root, one product rounding and one fma rounding."""
    mz = mean.double() if zcol is None else mean.double() * zcol.double()
    se = torch.sqrt(var.double()) * eps.double()
    return mz + se, 4.0 * 2.0 ** -24 * (mz.abs() + se.abs())


def dense_member(csrs, weights, biases, dims, m):
    """fp64 numpy (Ws, bs) of member m: the dense decode of its (nnz,) weight vectors."""
    Ws, bs = [], []
    for i, (row_ptr, col) in enumerate(csrs):
        Ws.append(sr.decode(row_ptr.cpu(), col.cpu(), weights[i][m].double().cpu(), dims[i + 1], dims[i]).numpy())
        bs.append(biases[i][m].double().cpu().numpy())
    return Ws, bs


def member_ref(Ws, bs, x, masks, targets=None):
    """tests/explain_ref.py's explanation of one member at the explained outputs: contributions (B, C', F), intercept (B, C'),
    logits (B, C), terms (B, C') = sum_i |contributions| + |intercept| + |logit|.  ``targets`` None: every output; else (B,)."""
    ref = er.explain_ref(Ws, bs, x, masks)
    con, k, lg = ref["contributions"], ref["intercept"], ref["logits"]
    if targets is not None:
        rows = np.arange(con.shape[0])
        t = np.asarray(targets)
        con, k, lt = con[rows, t][:, None, :], k[rows, t][:, None], lg[rows, t][:, None]
    else:
        lt = lg
    return dict(contributions=con, intercept=k, logits=lg, terms=np.abs(con).sum(-1) + np.abs(k) + np.abs(lt))


def stats_ref(members):
    """mean, std (unbiased; 0 for one member), counts > 0 and < 0 over axis 0 of the fp64 members (S, ...)."""
    S = members.shape[0]
    std = members.std(axis=0, ddof=1) if S > 1 else np.zeros(members.shape[1:])
    return members.mean(axis=0), std, (members > 0).sum(axis=0), (members < 0).sum(axis=0)


def autograd_contributions(Ws, bs, x):
    """(contributions (B, C, F), logits (B, C)) of the dense ReLU chain by torch.autograd in float64: J from one backward per
    output, times x."""
    Wt = [torch.as_tensor(W, dtype=torch.float64) for W in Ws]
    bt = [torch.as_tensor(b, dtype=torch.float64) for b in bs]
    xt = torch.as_tensor(x, dtype=torch.float64).clone().requires_grad_(True)
    h = xt
    for l, (W, b) in enumerate(zip(Wt, bt)):
        h = h @ W.T + b
        if l < len(Wt) - 1:
            h = torch.relu(h)
    J = torch.stack([torch.autograd.grad(h[:, c].sum(), xt, retain_graph=True)[0] for c in range(h.shape[1])], dim=1)
    return (J * xt.detach()[:, None, :]).numpy(), h.detach().numpy()
