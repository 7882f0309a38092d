#!/usr/bin/env python3
"""Time of the uncertainty metrics (lbbnn_eval_uncertainty) on one MI355X, S = 10 members, frozen LRT 784-400-400-10 and frozen
planar MNF 784-1200-1200-10, B in {100, 1000}:

  alone   on fixed outputs: UncertaintyAccumulator.update (2 launches) against ``torch_update``, the same per-row numbers and
          the same totals (counts, six double sums, reliability bins, three histograms) composed from torch calls, also without
          a host read
  pass    a whole batch: fz.ensemble + fz(x, sample=False) + EvalAccumulator.update, with and without
          UncertaintyAccumulator.update on the same outputs.  eval_metrics.hip is unchanged, so the pass without it is what the
          tree did before; the difference is the added cost per batch

Device events around windows of --calls batches, the two forms of a pair alternating, --repeats windows each after a warm-up of
both; every window is printed, the fastest is compared, and the spread (slowest / fastest - 1) of each form stands next to the
difference.  The kernel form counts as slower than the torch composition only beyond the larger of the two spreads.  Before
timing, the torch composition's totals are compared with the kernel's (integers must agree up to rows whose fp32 value sits on
a bin edge; both numbers are printed)."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd
from bnn_amd import evaluate

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("eval_uncertainty_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S, C, M, K = 10, 10, 20, 1024
NETS = {"lrt": (784, 400, 400, 10), "mnf": (784, 1200, 1200, 10)}


def make(kind):
    torch.manual_seed(0)
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork(NETS[kind], 2, z_flow_type="Planar", r_flow_type="Planar")
    else:
        net = bnn_amd.lrt.BayesianNetwork(NETS[kind])
    return net.to(dev).eval()


def batch(B):
    g = torch.Generator().manual_seed(1)
    return torch.rand(B, 784, generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)


class TorchTotals:
    """The totals of UncertaintyAccumulator as torch tensors, added to by ``torch_update``."""

    def __init__(self):
        self.counts = torch.zeros(6, dtype=torch.int64, device=dev)
        self.sums = torch.zeros(6, dtype=torch.float64, device=dev)
        self.bins = torch.zeros(3, M, dtype=torch.int64, device=dev)
        self.bin_conf = torch.zeros(M, dtype=torch.float64, device=dev)
        self.hist = torch.zeros(3, K, dtype=torch.int64, device=dev)


def torch_update(tt, o, y):
    """The per-row numbers and totals of lbbnn_eval_uncertainty as a torch composition (valid targets assumed, no host read)."""
    B = o.shape[1]
    p = o.exp()
    pb = p.mean(0)
    zero = torch.zeros((), device=dev)
    total = -torch.where(pb == 0, zero, pb * pb.log()).sum(-1)
    expected = (-torch.where(p == 0, zero, p * o).sum(-1)).mean(0)
    mi = (total - expected).clamp_min(0.0)
    conf, pred = pb.max(-1)
    idx = torch.arange(B, device=dev)
    brier = ((pb - torch.nn.functional.one_hot(y, C)) ** 2).sum(-1)
    ls = -(torch.logsumexp(o[:, idx, y], 0) - math.log(S))
    fin = torch.isfinite(conf) & torch.isfinite(total) & torch.isfinite(expected) & torch.isfinite(mi)
    hit = pred.eq(y)
    lsf = torch.isfinite(ls)
    tt.counts[:2] += B
    tt.counts[3:] += torch.stack([hit.sum(), (~fin).sum(), (fin & ~lsf).sum()])
    w = fin.double()
    tt.sums += torch.stack([(total.double() * w).sum(), (expected.double() * w).sum(), (mi.double() * w).sum(),
                            (conf.double() * w).sum(), (brier.double() * w).sum(), (ls.double() * (fin & lsf).double()).sum()])
    safe = lambda v: torch.where(fin, v, zero)
    mb = (safe(conf) * M).clamp(0, M).long().clamp(0, M - 1)
    ones = fin.long()
    tt.bins[0].index_add_(0, mb, ones)
    tt.bins[1].index_add_(0, mb, ones)
    tt.bins[2].index_add_(0, mb, ones * hit.long())
    tt.bin_conf.index_add_(0, mb, conf.double() * w)
    sc = float(K / math.log(C))
    for i, (v, s) in enumerate(((total, sc), (mi, sc), (1.0 - conf, float(K)))):
        tt.hist[i].index_add_(0, (safe(v) * s).clamp(0, K).long().clamp(0, K - 1), ones)
    return pb, pred, conf, total, expected, mi, brier, ls


def window(fn, n):
    """ms per call of n calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def pair(f0, f1):
    """Both forms warmed up, then --repeats alternating windows each: (windows of f0, windows of f1)."""
    for i in range(args.warmup):
        f0(i)
        f1(i)
    t0, t1 = [], []
    for _ in range(args.repeats):
        t0.append(window(f0, args.calls))
        t1.append(window(f1, args.calls))
    return t0, t1


fmt = lambda v: " ".join("%.4f" % u for u in v)
spread = lambda v: max(v) / min(v) - 1.0
print("S = %d members, C = %d, conf_bins = %d, hist_bins = %d; per form %d windows of %d batches (ms per batch, device events), "
      "the forms alternating, after %d warm-up batches of each" % (S, C, M, K, args.repeats, args.calls, args.warmup))
slower = []
for kind, dims in NETS.items():
    fz = evaluate.freeze(make(kind))
    name = "%s %s" % (kind, "-".join(map(str, dims)))
    for B in (100, 1000):
        x, y = batch(B)
        bnn_amd.manual_seed(1, 0)
        o, m = fz.ensemble(x, S).clone(), fz(x, sample=False).clone()
        # the two compositions agree: integers up to bin-edge rows, sums to fp32 rounding
        u, tt = evaluate.UncertaintyAccumulator(C, S, dev, conf_bins=M, hist_bins=K), TorchTotals()
        u.update(o, y)
        torch_update(tt, o, y)
        r = u.result()
        d_hist = int((torch.from_numpy(r["histograms"]["total_entropy"]["counts"]).to(dev) - tt.hist[0]).abs().sum()) // 2
        d_bins = int((torch.from_numpy(r["bin_rows"]).to(dev) - tt.bins[0]).abs().sum()) // 2
        d_sum = max(abs(r[k + "_sum"] - float(tt.sums[i])) / max(1.0, abs(r[k + "_sum"]))
                    for i, k in enumerate(("total_entropy", "expected_entropy", "mutual_information", "confidence", "brier", "log_score")))
        agree = "kernel vs torch totals: correct_bma %d / %d, rows in another entropy bin %d, in another confidence bin %d, " \
                "largest relative difference of the six sums %.2e" % (r["correct_bma"], int(tt.counts[3]), d_hist, d_bins, d_sum)

        def kernel_alone(i):
            u.update(o, y)

        def torch_alone(i):
            torch_update(tt, o, y)

        tk, tt_ = pair(kernel_alone, torch_alone)
        lim = max(spread(tk), spread(tt_))
        if min(tk) > min(tt_) * (1.0 + lim):
            slower.append((kind, B))
        print("%s B=%-4d alone on fixed outputs  kernel [%s] spread %.1f%%  torch [%s] spread %.1f%%  min/min torch/kernel %.2fx; %s"
              % (name, B, fmt(tk), 100 * spread(tk), fmt(tt_), 100 * spread(tt_), min(tt_) / min(tk), agree))
        acc0, acc1 = evaluate.EvalAccumulator(C, S, dev), evaluate.EvalAccumulator(C, S, dev)
        u1 = evaluate.UncertaintyAccumulator(C, S, dev, conf_bins=M, hist_bins=K)

        def pass_metrics(i):
            acc0.update(fz.ensemble(x, S), y, fz(x, sample=False))

        def pass_both(i):
            out = fz.ensemble(x, S)
            acc1.update(out, y, fz(x, sample=False))
            u1.update(out, y)

        t0, t1 = pair(pass_metrics, pass_both)
        print("%s B=%-4d whole pass  EvalAccumulator alone [%s] spread %.1f%%  + UncertaintyAccumulator [%s] spread %.1f%%  "
              "added per batch %.1f us (min - min; eval_metrics_kernel itself: 7-9 us)"
              % (name, B, fmt(t0), 100 * spread(t0), fmt(t1), 100 * spread(t1), 1e3 * (min(t1) - min(t0))))
print("kernel form slower than the torch composition beyond the larger window spread: %s" % (slower if slower else "nowhere"))
