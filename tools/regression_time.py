#!/usr/bin/env python3
"""Time of the regression column on one MI355X (identity head, lbbnn_elbo_gaussian_loss*, lbbnn_eval_regression), one process.
Device events around windows of calls, the forms of a comparison alternating window by window after a warm-up of each; the
fastest window and the window spread (slowest / fastest - 1) are printed.  Writes profiles/regression.txt.

  1. the loss launch alone: elbo_gaussian_loss plain (stats=) and monitored, beside elbo_bce_loss plain and monitored, at
     B = 400, O = 1 and B = 4096, O = 1 -- one graph of 100 consecutive launches per form, the four graphs' windows alternating;
  2. the graphed training step of examples/train_regression_synthetic.py's networks (8 -> 32 -> 1, LRT and planar MNF, a learnable
     log_var in its own Adam group, B = 400): the fused loss against its torch spelling
     (0.5 * (log(2 pi) + lv + (y - m)^2 * exp(-lv))).sum() + kl / N, both captured by graphs.make_graphed_train_step;
  3. the evaluation step at S = 10 members, B = 100 and 1000, on the frozen median probability model: the graphed step
     (make_graphed_eval_step with a RegressionAccumulator: ensemble + posterior-mean forward + lbbnn_eval_regression) against
     the eager ensemble followed by torch metrics (rmse, log density by torch.logsumexp, PIT by torch.special.erfc and
     torch.histc) with one host read per batch.

    python tools/regression_time.py

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
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "regression.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("regression_time: needs a HIP device (no CPU path, no CPU timing)")
dev = torch.device("cuda:0")
N, S = 5, 10
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
    say("  %-34s fastest %.4f %s  spread %.1f %%  (slowest %.4f, median %.4f)"
        % (label, unit * min(ws), what, 100 * (max(ws) / min(ws) - 1), unit * max(ws), unit * sorted(ws)[len(ws) // 2]))
    return min(ws), max(ws) / min(ws) - 1


def verdict(name, a, b, name_b):
    (fa, sa), (fb, sb) = a, b
    tag = "within" if abs(fa - fb) <= sb * fb else ("FASTER than" if fa < fb else "SLOWER than")
    say("  %s / %s = %.3f: %s %s's own window spread (%.1f %%)" % (name, name_b, fa / fb, tag, name_b, 100 * sb))


say("tools/regression_time.py: device events around windows of %d calls, %d windows per form, forms alternating, after %d warm-up "
    "calls of each; fastest window, spread = slowest / fastest - 1" % (args.replays, args.windows, args.warmup))

# ---- 1. the loss launch alone
LAUNCHES = 100
gen = torch.Generator().manual_seed(0)
for B in (400, 4096):
    m = torch.randn(B, 1, generator=gen).to(dev)
    yt = (m.cpu() + 0.5 * torch.randn(B, 1, generator=gen)).to(dev)
    lv = torch.zeros(1, device=dev)
    p = torch.sigmoid(m)
    yb = (torch.rand(B, 1, generator=gen) > 0.5).float().to(dev)
    kl = torch.tensor(1234.5, device=dev)
    forms = {"gaussian plain": lambda kw: bnn_amd.elbo_gaussian_loss(m, yt, lv, kl, N, **kw),
             "gaussian monitor": lambda kw: bnn_amd.elbo_gaussian_loss(m, yt, lv, kl, N, **kw),
             "bce plain": lambda kw: bnn_amd.elbo_bce_loss(p, yb, kl, N, **kw),
             "bce monitor": lambda kw: bnn_amd.elbo_bce_loss(p, yb, kl, N, **kw)}
    kws = {"gaussian plain": {"stats": torch.zeros(4, dtype=torch.float64, device=dev)},
           "gaussian monitor": {"monitor": bnn_amd.TrainMonitor(1, dev)},
           "bce plain": {"stats": torch.zeros(4, dtype=torch.int32, device=dev)},
           "bce monitor": {"monitor": bnn_amd.TrainMonitor(1, dev)}}
    graphs = {}
    with torch.no_grad():
        for name, fn in forms.items():
            fn(kws[name])
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(LAUNCHES):
                    out = fn(kws[name])
    res = timed({k: g.replay for k, g in graphs.items()}, max(1, args.replays // 4))
    say("1. the loss launch alone, B = %d, O = 1, kl given: graphs of %d launches" % (B, LAUNCHES))
    got = {k: row(k, ws, 1e3 / LAUNCHES, "us") for k, ws in res.items()}
    verdict("gaussian plain", got["gaussian plain"], got["bce plain"], "bce plain")
    verdict("gaussian monitor", got["gaussian monitor"], got["bce monitor"], "bce monitor")
    del graphs

# ---- 2. the graphed training step, 3. the evaluation step
DIMS, B = (8, 32, 1), 400
x = torch.randn(B, DIMS[0], generator=gen).to(dev)
y = torch.randn(B, 1, generator=gen).to(dev)


def make(kind):
    torch.manual_seed(0)
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork(DIMS, 2, z_flow_type="Planar", r_flow_type="Planar", head="identity")
    else:
        net = bnn_amd.lrt.BayesianNetwork(DIMS, head="identity")
    return net.to(dev).train()


def graphed(kind, fused):
    net = make(kind)
    log_var = torch.nn.Parameter(torch.zeros(1, device=dev))
    opt = bnn_amd.optim.Adam([{"params": list(net.parameters())}, {"params": [log_var], "lr": 0.05}], lr=0.01)
    if fused:
        mon = bnn_amd.TrainMonitor(1, dev)
        opt.set_guard(mon)
        st = torch.zeros(4, dtype=torch.float64, device=dev)
        lf = lambda n, a, b: bnn_amd.elbo_gaussian_loss(n(a, sample=True), b, log_var, n.kl(), N, stats=st, monitor=mon)
    else:
        def lf(n, a, b):
            d = b - n(a, sample=True)
            return (0.5 * ((LOG_2PI + log_var) + (d * d) * torch.exp(-log_var))).sum() + n.kl() / N
    step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)
    return net, log_var, step


for kind in ("lrt", "mnf"):
    (net_f, lv_f, step_f), (net_t, lv_t, step_t) = graphed(kind, True), graphed(kind, False)
    res = timed({"fused": step_f.graph.replay, "torch": step_t.graph.replay}, args.replays)
    say("2. %s 8-32-1 graphed training step, B = %d (fused: stats, monitor and guard on; torch spelling: none of them)" % (kind, B))
    got = {k: row(k + " loss", ws) for k, ws in res.items()}
    verdict("fused", got["fused"], got["torch"], "torch")

    net_f.eval()
    fz = evaluate.freeze(net_f, gates="mpm")
    for EB in (100, 1000):
        ex = torch.randn(EB, DIMS[0], generator=gen).to(dev)
        ey = torch.randn(EB, 1, generator=gen).to(dev)
        acc = evaluate.RegressionAccumulator(1, S, dev, lv_f)
        estep = bnn_amd.graphs.make_graphed_eval_step(fz, ex, ey, S, acc)
        tot = torch.zeros(4 + 20, dtype=torch.float64, device=dev)

        @torch.no_grad()
        def eager_torch():
            o = fz.ensemble(ex, S)
            pm = fz(ex, sample=False)
            lvv = lv_f.detach()
            r = ey[None] - o
            t = -0.5 * ((LOG_2PI + lvv) + (r * r) * torch.exp(-lvv))
            ld = torch.logsumexp(t, 0) - math.log(S)
            pit = (0.5 * torch.special.erfc(-(r * torch.exp(-0.5 * lvv)) * 0.7071067811865476)).mean(0)
            e = ey - o.mean(0)
            tot.add_(torch.cat([torch.stack([(e * e).sum(), e.abs().sum(), ld.sum(), ((ey - pm) ** 2).sum()]).double(),
                                torch.histc(pit, 20, 0.0, 1.0).double()]))
            tot.tolist()                                               # the per-batch host read of a torch spelling

        res = timed({"graphed": estep.graph.replay, "eager": eager_torch}, max(1, args.replays // 4))
        say("3. %s 8-32-1 evaluation step, S = %d, B = %d (graphed: ensemble + posterior mean + lbbnn_eval_regression, no host read; "
            "eager: ensemble + posterior mean + torch metrics + one host read)" % (kind, S, EB))
        got = {k: row(k, ws) for k, ws in res.items()}
        verdict("graphed", got["graphed"], got["eager"], "eager")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
