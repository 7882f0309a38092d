#!/usr/bin/env python3
"""Time of the regression scores on one MI355X (lbbnn_eval_regression_scores: per-member noise, CRPS, prediction intervals), one
process.  Device events around windows of calls, the forms of a comparison alternating window by window after a warm-up of each;
the fastest window and the window spread (slowest / fastest - 1) are printed.  Writes profiles/regression_scores.txt.

At S = 10 members, B = 100 / 1000 / 4096 rows, O = 1 and 16 units, levels (0.5, 0.9):

  (a) the graphed evaluation step of a frozen 8 -> 32 -> O LRT network (make_graphed_eval_step: ensemble + posterior-mean forward +
      the metrics call) with a RegressionScoreAccumulator against the same step with a RegressionAccumulator, both reading one
      (units,) log-variance tensor: the difference is the cost of the CRPS and four quantiles per element.  For O = 1 also the
      8 -> 32 -> 2 network scored with log_var="output";
  (b) the scores call alone with an accumulator (a graph of 20 consecutive calls, per call) on a (S, B, O) block with a
      log-variance per member and element, against a torch spelling of the same numbers on the device -- mixture log density, PIT,
      closed-form CRPS over all member pairs, 26 bisection steps for the four quantiles, interval scores, the sums -- followed by
      the one host read that a torch spelling ends with.

    python tools/regression_scores_time.py

There is no pass threshold: a row that comes out slower than its comparison is printed as such."""
import argparse
import math
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import torch
import bnn_amd
from bnn_amd import evaluate

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--replays", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "regression_scores.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("regression_scores_time: needs a HIP device (no CPU path, no CPU timing)")
dev = torch.device("cuda:0")
S, LEVELS, CALLS = 10, (0.5, 0.9), 20
LOG_2PI = math.log(2.0 * math.pi)
lines = []
say = lambda s: (lines.append(s), print(s, flush=True))


def timed(fns, calls):
    """{name: [ms per call of each window]}, the forms' windows alternating."""
    for f in fns.values():
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(args.windows):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            torch.cuda.synchronize()
            res[k].append(a.elapsed_time(b) / calls)
    return res


def row(label, ws, unit=1.0, what="ms"):
    say("  %-38s fastest %.4f %s  spread %.1f %%  (slowest %.4f, median %.4f)"
        % (label, unit * min(ws), what, 100 * (max(ws) / min(ws) - 1), unit * max(ws), unit * sorted(ws)[len(ws) // 2]))
    return min(ws), max(ws) / min(ws) - 1


def verdict(name, a, b, name_b):
    (fa, sa), (fb, sb) = a, b
    tag = "within" if abs(fa - fb) <= sb * fb else ("FASTER than" if fa < fb else "SLOWER than")
    say("  %s / %s = %.3f (%+.4f ms): %s %s's own window spread (%.1f %%)" % (name, name_b, fa / fb, fa - fb, tag, name_b, 100 * sb))


say("tools/regression_scores_time.py: device events around windows of calls, %d windows per form, forms alternating, after %d "
    "warm-up calls of each; fastest window, spread = slowest / fastest - 1; S = %d, levels %s" % (args.windows, args.warmup, S, LEVELS))
gen = torch.Generator().manual_seed(0)


def frozen(units_out):
    torch.manual_seed(0)
    return evaluate.freeze(bnn_amd.lrt.BayesianNetwork((8, 32, units_out), head="identity").to(dev).eval(), gates="mpm")


# ---- (a) the graphed evaluation step
for O in (1, 16):
    fz = frozen(O)
    lv = torch.full((O,), -1.0, device=dev)
    for B in (100, 1000, 4096):
        x = torch.randn(B, 8, generator=gen).to(dev)
        y = torch.randn(B, O, generator=gen).to(dev)
        forms = {"RegressionAccumulator": evaluate.RegressionAccumulator(O, S, dev, lv),
                 "RegressionScoreAccumulator": evaluate.RegressionScoreAccumulator(O, S, dev, lv, levels=LEVELS)}
        steps = {k: bnn_amd.graphs.make_graphed_eval_step(fz, x, y, S, a) for k, a in forms.items()}
        if O == 1:
            fz2 = frozen(2)
            steps["RegressionScoreAccumulator \"output\""] = bnn_amd.graphs.make_graphed_eval_step(
                fz2, x, y, S, evaluate.RegressionScoreAccumulator(1, S, dev, "output", levels=LEVELS))
        res = timed({k: s.graph.replay for k, s in steps.items()}, args.replays)
        say("(a) graphed evaluation step, LRT 8-32-%d frozen (mpm), B = %d: ensemble + posterior mean + metrics call, no host read" % (O, B))
        got = {k: row(k, ws) for k, ws in res.items()}
        for k in got:
            if k != "RegressionAccumulator":
                verdict(k, got[k], got["RegressionAccumulator"], "RegressionAccumulator")
        del steps


# ---- (b) the scores call alone against a torch spelling
def a_term(m, v):
    sd = torch.sqrt(v)
    z = m.abs() / sd
    return 2.0 * sd * torch.exp(-0.5 * z * z) * 0.3989422804014327 + m.abs() * torch.erf(z * 0.7071067811865476)


def phi(z):
    return 0.5 * torch.special.erfc(-z * 0.7071067811865476)


@torch.no_grad()
def torch_scores(o, y, lv, tot):
    var, sd = torch.exp(lv), torch.exp(0.5 * lv)
    r = y[None] - o
    ld = torch.logsumexp(-0.5 * ((LOG_2PI + lv) + (r * r) * torch.exp(-lv)), 0) - math.log(S)
    pit = phi(r / sd).mean(0)
    crps = a_term(r, var).mean(0) - a_term(o[:, None] - o[None], var[:, None] + var[None]).sum((0, 1)) / (2.0 * S * S)
    pm = o.mean(0)
    ev = ((o - pm[None]) ** 2).mean(0)
    av = var.mean(0)
    pt = torch.tensor([0.5 * (1 - p) for p in LEVELS] + [0.5 * (1 + p) for p in LEVELS], device=o.device).view(-1, 1, 1)
    lo = (o - 8.0 * sd).amin(0).expand(pt.shape[0], -1, -1).clone()
    hi = (o + 8.0 * sd).amax(0).expand(pt.shape[0], -1, -1).clone()
    for _ in range(26):
        mid = 0.5 * (lo + hi)
        below = phi((mid[None] - o[:, None]) / sd[:, None]).mean(0) < pt
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    q = 0.5 * (lo + hi)
    L = len(LEVELS)
    l, u = q[:L], q[L:]
    k = torch.tensor([2.0 / (1 - p) for p in LEVELS], device=o.device).view(-1, 1, 1)
    score = (u - l) + k * ((l - y[None]).clamp_min(0) + (y[None] - u).clamp_min(0))
    inside = ((l <= y[None]) & (y[None] <= u)).sum((1, 2)).double()
    e = y - pm
    tot.add_(torch.cat([torch.stack([(e * e).sum(), e.abs().sum(), ld.sum(), ev.sum(), (ev + av).sum(), av.sum(), crps.sum()]).double(),
                        (u - l).sum((1, 2)).double(), score.sum((1, 2)).double(), inside, torch.histc(pit, 20, 0.0, 1.0).double()]))
    return tot.tolist()                                                 # the host read a torch spelling ends with


for O in (1, 16):
    for B in (100, 1000, 4096):
        centre = 2.0 * torch.randn(B, O, generator=gen)
        lv = (-0.5 + 0.5 * torch.randn(S, B, O, generator=gen)).to(dev)
        o = (centre[None] + 0.4 * torch.randn(S, B, O, generator=gen)).to(dev)
        y = (centre + torch.randn(B, O, generator=gen)).to(dev)
        acc = evaluate.RegressionScoreAccumulator(O, S, dev, 0.0, levels=LEVELS)
        acc.update(o, y, log_var=lv)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(CALLS):
                acc.update(o, y, log_var=lv)
        tot = torch.zeros(7 + 3 * len(LEVELS) + 20, dtype=torch.float64, device=dev)
        res_k = timed({"kernel": graph.replay}, max(1, args.replays // 4))
        res_t = timed({"torch": lambda: torch_scores(o, y, lv, tot)}, max(1, args.replays // 20))
        say("(b) the scores call alone, B = %d, O = %d, a log-variance per member and element (kernel: graph of %d calls with "
            "totals, per call, no host read; torch: the same numbers in torch ops + one host read)" % (B, O, CALLS))
        gk = row("lbbnn_eval_regression_scores", [w / CALLS for w in res_k["kernel"]], 1e3, "us")
        gt = row("torch spelling + host read", res_t["torch"], 1e3, "us")
        verdict("kernel", gk, gt, "torch")
        del graph

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
