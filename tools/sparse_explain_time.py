#!/usr/bin/env python3
"""Time of evaluate.explain_ensemble (explanations of S = 10 sampled-weight members of the sparse median-probability model,
targets="pred") against a torch spelling of the same computation in the same process:

  hip     evaluate.explain_ensemble(fz, x, 10, targets="pred"): the whole Python call -- z flow, weight draw, members' forward,
          sweep on the transposed pattern, intercept, statistics
  torch   the SAME drawn weights decoded once, outside the timed window, to dense (S, O, I); the members' forward and the sweep
          as torch.bmm over the members, J * x, then mean / std / sign shares over the members; no host read
  bmm     the torch spelling's forward, sweep and J * x alone (no statistics)

for LRT 784-400-400-10 and planar MNF 784-1200-1200-10 at B = 100 and B = 1000, with lambdal = seeded U(-3, 3) and the
threshold moved so that 1, 5 and 10 % of the weights are kept.

The forms alternate; each is timed in --repeats windows (at least five) of calls between two device events after a warm-up of
all, and the fastest and the slowest window of each are on the page.  The logits and every member's contributions of the two
spellings are compared first, the torch one under the call's targets and masks.  REQUIRED, at 5 % kept, for both networks and
both batch sizes: the slowest hip window is faster than the fastest window of BOTH torch forms; each such row says whether it holds.  1 % and 10 % kept are recorded without a bar.
`first` is one call on a freshly frozen model: it includes the one-off build of the transposed pattern (and this process's
first launches of the kernels at that shape), which every later call finds in the model's buffers.

The table goes to stdout and to --out (default profiles/sparse_explain.txt)."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bnn_amd
from bnn_amd import evaluate

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=40, help="calls per window at B = 100 (B = 1000: a quarter of it)")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_explain.txt"))
args = ap.parse_args()
if args.repeats < 5:
    sys.exit("sparse_explain_time: at least five windows per form")
if not torch.cuda.is_available():
    sys.exit("sparse_explain_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S = 10
NETS = {"lrt": (784, 400, 400, 10), "mnf": (784, 1200, 1200, 10)}
KEPT = (0.01, 0.05, 0.10)
REQUIRED = 0.05


def make(kind):
    torch.manual_seed(0)
    dims = NETS[kind]
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
    else:
        net = bnn_amd.lrt.BayesianNetwork(dims)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.copy_(torch.empty(l.out_features, l.in_features).uniform_(-3, 3, generator=g).to(dev))
    return net


def threshold_of(kept):
    """P(U(-3, 3) > cut) = kept  <=>  cut = 3 - 6 kept; the threshold is its sigmoid."""
    return 1.0 / (1.0 + math.exp(-(3.0 - 6.0 * kept)))


def decode(fz, weights):
    """Per layer the dense (S, O, I) weights of the members."""
    out = []
    for i, w in enumerate(weights):
        row_ptr, col, _, _ = fz.csr(i)
        O, I = fz.dims[i + 1], fz.dims[i]
        rows = torch.repeat_interleave(torch.arange(O, device=dev), (row_ptr[1:] - row_ptr[:-1]).long())
        d = torch.zeros(S, O, I, device=dev)
        d[:, rows, col.long()] = w
        out.append(d)
    return out


def torch_spelling(Ws, bs, x, stats=True, given=None):
    """``given``: (targets, masks) of the call, for the parity check -- a ReLU unit within rounding of 0, or two logits within
    rounding of each other, then cannot put the two spellings on different linear pieces; the timed windows take their own."""
    n, B = len(Ws), x.shape[0]
    h, masks = x[None].expand(S, B, x.shape[1]), []
    for l in range(n):
        a = torch.baddbmm(bs[l][:, None, :], h, Ws[l].transpose(1, 2))
        if l < n - 1:
            masks.append(a > 0 if given is None else given[1][l])
            h = a * masks[-1] if given is not None else torch.relu(a)
    t = a.mean(0).argmax(1)
    if given is not None:
        return a, t, torch_sweep(Ws, x, given[0], masks)
    return torch_sweep(Ws, x, t, masks, stats)


def torch_sweep(Ws, x, t, masks, stats=False):
    n = len(Ws)
    G = Ws[-1][:, t, :]                                      # (S, B, width): the explained output's row of the last layer
    for l in range(n - 2, -1, -1):
        G = torch.bmm(G * masks[l], Ws[l])
    con = G * x[None]
    if not stats:
        return con
    return con.mean(0), con.std(0), (con > 0).float().mean(0), (con < 0).float().mean(0)


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("S = %d members, targets=\"pred\"; per form %d windows (ms per call: fastest .. slowest; %d calls per window at B = 100, %d "
    "at B = 1000), the forms alternating, after %d warm-up calls of each" % (S, args.repeats, args.calls, max(1, args.calls // 4),
                                                                            args.warmup))
say("device: %s" % torch.cuda.get_device_name(0))
held = []
for kind, dims in NETS.items():
    net = make(kind)
    for kept in KEPT:
        for B in (100, 1000):
            fz = evaluate.freeze(net, "mpm", threshold=threshold_of(kept), sparse=True)
            x = torch.rand(B, 784, generator=torch.Generator().manual_seed(1)).to(dev)
            bnn_amd.manual_seed(1, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evaluate.explain_ensemble(fz, x, S, targets="pred", keep_weights=True, keep_masks=True, keep_members=True)
            torch.cuda.synchronize()
            first = 1e3 * (time.perf_counter() - t0)
            Ws, bs = decode(fz, res["weights"]), [b.contiguous() for b in res["biases"]]
            # parity, under the call's own targets and masks: logits and every member's contributions; and how many rows the
            # torch spelling's own argmax explains differently
            lg, t_own, con = torch_spelling(Ws, bs, x, given=(res["targets"], res["masks"]))
            differ = int((t_own != res["targets"]).sum())
            err_l = float((res["logits"] - lg).abs().max() / lg.abs().max())
            scale = float(con.abs().max())
            err = "%.2g" % (float((res["members"][:, :, 0] - con).abs().max()) / scale) if scale > 0 else \
                "n/a (every explained contribution is exactly 0 in both: the timing is of an all-zero explanation)"
            del lg, con
            fns = {"hip": lambda: evaluate.explain_ensemble(fz, x, S, targets="pred"),
                   "torch": lambda: torch_spelling(Ws, bs, x),
                   "bmm": lambda: torch_spelling(Ws, bs, x, stats=False)}
            for _ in range(args.warmup):
                for f in fns.values():
                    f()
            calls = args.calls if B == 100 else max(1, args.calls // 4)
            t = {k: [] for k in fns}
            for _ in range(args.repeats):
                for k, f in fns.items():
                    t[k].append(window(f, calls))
            verdict = ""
            if kept == REQUIRED:
                ok = max(t["hip"]) < min(min(t["torch"]), min(t["bmm"]))
                held.append(ok)
                verdict = "  required (slowest hip < fastest torch and bmm): %s" % ("HOLDS" if ok else "DOES NOT HOLD")
            say("%s kept %.4f (nnz %d) B=%-4d  %s  first %.2f  bmm/hip %.2fx  vs torch under the call's targets and masks: logits "
                "rel. diff %.2g, contributions %s; rows where torch's own argmax differs: %d%s"
                % (kind, fz.density, fz.nnz, B, "  ".join("%s [%.4f .. %.4f]" % (k, min(v), max(v)) for k, v in t.items()), first,
                   min(t["bmm"]) / min(t["hip"]), err_l, err, differ, verdict))
            del Ws, bs, res
say("the requirement holds in %d of %d rows (5 %% kept)" % (sum(held), len(held)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
