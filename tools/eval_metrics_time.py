#!/usr/bin/env python3
"""Time of one evaluation batch of a frozen model, S = 10 members, with its metrics, three ways in one process:

  parent   what the tree did before lbbnn_eval_metrics: evaluate.ensemble_eval(fz, x, y, 10) (ensemble, posterior-mean forward,
           torch mean / argmax / eq / sum and two int() reads), plus evaluate.predictive_entropy(outputs).mean() and its read
  acc      fz.ensemble + fz(x, sample=False) + EvalAccumulator.update (one lbbnn_eval_metrics call: 2 launches), and ONE
           acc.result() per 10 batches -- the only host read
  graph    graphs.make_graphed_eval_step: the same launches replayed from one HIP graph, one acc.result() per 10 batches

for frozen planar MNF 784-1200-1200-10 and frozen LRT 784-400-400-10, fp32 and bf16x3, B in {100, 1000}.  The three forms
alternate; each is timed REPEATS times as a window of CALLS batches on the host clock between two device synchronisations (the
parent form synchronises in every batch, so its host time IS its time), after a warm-up of all three; every window is printed,
so the spread of each form stands next to the differences between them.  Before timing, the acc and graph forms are run from
the same seed and their totals compared bit for bit, and the parent's correct counts are printed next to the accumulator's.

Also the metrics alone, on fixed outputs: the torch glue of the parent form with its three reads against acc.update.

--trace FORM --net NET --batch B --reps R runs only that form R times (fp32) for a `rocprofv3 --kernel-trace --stats` run of
its own (kernels per batch = calls / R)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd
from bnn_amd import evaluate, graphs

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--trace", choices=("parent", "acc", "graph", "metrics"), default=None)
ap.add_argument("--net", choices=("mnf", "lrt"), default="lrt")
ap.add_argument("--batch", type=int, default=100)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("eval_metrics_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S, READ_EVERY = 10, 10
NETS = {"mnf": (784, 1200, 1200, 10), "lrt": (784, 400, 400, 10)}


def make(kind):
    torch.manual_seed(0)
    dims = NETS[kind]
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
    else:
        net = bnn_amd.lrt.BayesianNetwork(dims)
    return net.to(dev).eval()


def batch(B):
    g = torch.Generator().manual_seed(1)
    return torch.rand(B, 784, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


def forms(fz, x, y):
    """The three per-batch callables (each takes the batch index) and the two accumulators."""
    acc_a, acc_g = evaluate.EvalAccumulator(10, S, dev), evaluate.EvalAccumulator(10, S, dev)
    step = graphs.make_graphed_eval_step(fz, x, y, S, acc_g)
    sx, sy = step.inputs

    def parent(i):
        r = evaluate.ensemble_eval(fz, x, y, S)
        e = evaluate.predictive_entropy(r["outputs"]).mean()
        return r["correct_ensemble"], r["correct_posterior_mean"], float(e)

    def acc(i):
        acc_a.update(fz.ensemble(x, S), y, fz(x, sample=False))
        if i % READ_EVERY == READ_EVERY - 1:
            return acc_a.result()

    def graph(i):
        step(sx, sy)                                          # the batch already lies in the graph's input buffers
        if i % READ_EVERY == READ_EVERY - 1:
            return acc_g.result()

    return {"parent": parent, "acc": acc, "graph": graph}, acc_a, acc_g


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


fmt = lambda v: " ".join("%.4f" % u for u in v)

if args.trace:
    fz = evaluate.freeze(make(args.net))
    x, y = batch(args.batch)
    if args.trace == "metrics":
        o, m = fz.ensemble(x, S), fz(x, sample=False)
        acc = evaluate.EvalAccumulator(10, S, dev)
        fn = lambda i: acc.update(o, y, m)
    else:
        fn = forms(fz, x, y)[0][args.trace]
    torch.cuda.synchronize()
    for i in range(args.reps):
        fn(i)
    torch.cuda.synchronize()
    print("ran the %s form of the %s net %d times at B = %d" % (args.trace, args.net, args.reps, args.batch))
    sys.exit(0)

print("S = %d members; per form %d windows of %d batches (ms per batch, host clock between synchronisations), the forms "
      "alternating, after %d warm-up batches of each; acc / graph read the totals once per %d batches"
      % (S, args.repeats, args.calls, args.warmup, READ_EVERY))
slower = []
for kind, dims in NETS.items():
    net = make(kind)
    for prec in ("fp32", "bf16x3"):
        bnn_amd.set_precision(prec)
        fz = evaluate.freeze(net)
        for B in (100, 1000):
            x, y = batch(B)
            f, acc_a, acc_g = forms(fz, x, y)
            # same seed, same batches: the graph's totals must be the eager accumulator's, bit for bit
            for a in (acc_a, acc_g):
                a.reset()
            bnn_amd.manual_seed(1, 0)
            for i in range(3):
                f["acc"](i)
            bnn_amd.manual_seed(1, 0)
            for i in range(3):
                f["graph"](i)
            same = "bitwise equal" if torch.equal(acc_a._totals, acc_g._totals) else "DIFFERENT"
            bnn_amd.manual_seed(1, 0)
            p = [f["parent"](i) for i in range(3)]
            ra = acc_a.result()
            counts = "parent correct %d / %d, acc %d / %d" % (sum(q[0] for q in p), sum(q[1] for q in p), ra["correct_ensemble"],
                                                              ra["correct_posterior_mean"])
            for i in range(args.warmup):
                for fn in f.values():
                    fn(i)
            t = {k: [] for k in f}
            for _ in range(args.repeats):
                for k, fn in f.items():
                    t[k].append(window(fn, args.calls))
            best = {k: min(v) for k, v in t.items()}
            for k in ("acc", "graph"):
                if best[k] > best["parent"]:
                    slower.append((kind, prec, B, k))
            print("%s %s %-6s B=%-4d  parent [%s]  acc [%s]  graph [%s]  min/min parent/acc %.2fx parent/graph %.2fx  totals "
                  "acc vs graph %s; %s"
                  % (kind, "-".join(map(str, dims)), prec, B, fmt(t["parent"]), fmt(t["acc"]), fmt(t["graph"]),
                     best["parent"] / best["acc"], best["parent"] / best["graph"], same, counts))
            if prec == "fp32":
                # the metrics alone, on fixed outputs
                o, m = fz.ensemble(x, S), fz(x, sample=False)
                a2 = evaluate.EvalAccumulator(10, S, dev)

                def glue(i):
                    pe, pm = o.mean(0).argmax(1), m.argmax(1)
                    return int(pe.eq(y).sum()), int(pm.eq(y).sum()), float(evaluate.predictive_entropy(o).mean())

                def metrics(i):
                    a2.update(o, y, m)
                    if i % READ_EVERY == READ_EVERY - 1:
                        return a2.result()

                for i in range(args.warmup):
                    glue(i)
                    metrics(i)
                tg, tm = [], []
                for _ in range(args.repeats):
                    tg.append(window(glue, args.calls))
                    tm.append(window(metrics, args.calls))
                print("%s metrics alone on fixed outputs B=%-4d  torch glue + 3 reads [%s]  acc.update [%s]  min/min %.2fx"
                      % (kind, B, fmt(tg), fmt(tm), min(tg) / min(tm)))
bnn_amd.set_precision("fp32")
print("slower than the parent form (fastest window against fastest window): %s" % (slower if slower else "nowhere"))
