#!/usr/bin/env python3
"""Evaluation time of the frozen baseline model (evaluate.freeze_base) against base_ensemble on the SAME network, one process:
the reference's baseline network 784-400-600-10, S = 10 members, B = 100 and B = 1000, under fp32 and bf16x3.

One evaluation step is the ensemble, the posterior-mean forward and EvalAccumulator.update:

  loop     base_ensemble(net, x, 10, gates=...) + evaluate._base_mean_forward(net, x) + acc.update   (untouched by the
           frozen model: these are the numbers of the code before it)
  eager    frozen.ensemble(x, 10) + frozen(x) + acc.update
  graph    the same step as one replay of graphs.make_graphed_eval_step

Arms: "sample" on the network as constructed (lambdal ~ U(0, 1)); "mpm" and "compact" on a SYNTHETIC structure, stated in the
output: every second hidden unit has no consumer, and of the weights between the remaining units a random share is kept so
that 10 % of all weights are kept (lambdal = +-3).  "mpm" is the full median-probability model of that network, "compact" is
freeze_base(net, "mpm", compact=True).

The forms of an arm alternate; each is timed --repeats times as a window of calls between two device events after a warm-up of
all, and reported as fastest window [slowest window] in ms per step, so the spread is on the page next to every ratio.  C
calls per step are the calls through the C ABI that enqueue work (a graph replay is one launch of the captured kernels).
The table goes to stdout and to --out (default profiles/base_frozen.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bnn_amd
from bnn_amd import _lib, evaluate, graphs

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=40, help="steps per window")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "base_frozen.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("base_frozen_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
S, DIMS, C = 10, (784, 400, 600, 10), 10


def make(structure):
    torch.manual_seed(0)
    net = bnn_amd.base.BayesianNetwork(DIMS).to(dev).eval()
    if structure:
        g = torch.Generator().manual_seed(2)
        with torch.no_grad():
            layers = net._layers()
            for i, l in enumerate(layers):
                O, I = l.out_features, l.in_features
                rows = torch.ones(O, dtype=torch.bool) if i == len(layers) - 1 else torch.arange(O) % 2 == 0
                cols = torch.ones(I, dtype=torch.bool) if i == 0 else torch.arange(I) % 2 == 0
                region = rows[:, None] & cols[None, :]
                share = 0.1 * O * I / int(region.sum())          # 10 % of ALL weights of the layer, inside the live region
                keep = region & (torch.rand(O, I, generator=g) < share)
                l.lambdal.copy_(torch.where(keep, torch.tensor(3.0), torch.tensor(-3.0)).to(dev))
    return net


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def c_calls(fn):
    _lib.RECORD = []
    try:
        fn()
        return len(_lib.RECORD)
    finally:
        _lib.RECORD = None


lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("784-400-600-10, S = %d members; per form %d windows of %d steps (ms per step: fastest [slowest]), the forms alternating, "
    "after %d warm-up steps of each" % (S, args.repeats, args.calls, args.warmup))
say("device: %s" % torch.cuda.get_device_name(0))
slower = []
for arm in ("sample", "mpm", "compact"):
    net = make(arm != "sample")
    gates = "sample" if arm == "sample" else "mpm"
    for prec in ("fp32", "bf16x3"):
        bnn_amd.set_precision(prec)
        fz = evaluate.freeze_base(net, gates, compact=arm == "compact")
        if prec == "fp32":
            extra = (", dims %s, needed %s, active density %.4f" % ("-".join(map(str, fz.dims)), "/".join(map(str, fz.needed)),
                                                                     fz.active_density)) if arm == "compact" else ""
            say("arm %-7s gates=%s: %s density %.4f%s" % (arm, gates, "expected" if gates == "sample" else "kept-weight",
                                                         fz.density, extra))
        for B in (100, 1000):
            gen = torch.Generator().manual_seed(1)
            x = torch.rand(B, DIMS[0], generator=gen).to(dev)
            y = torch.randint(0, C, (B,), generator=gen).to(dev)
            acc_l, acc_e, acc_g = (evaluate.EvalAccumulator(C, S, dev) for _ in range(3))

            def f_loop():
                out = evaluate.base_ensemble(net, x, S, gates=gates)["outputs"]
                acc_l.update(out, y, evaluate._base_mean_forward(net, x, False))

            def f_eager():
                acc_e.update(fz.ensemble(x, S), y, fz(x, sample=False))

            step = graphs.make_graphed_eval_step(fz, x, y, S, acc_g)
            f_graph = lambda: step(x, y)
            forms = (("loop", f_loop), ("eager", f_eager), ("graph", f_graph))
            for _ in range(args.warmup):
                for _, fn in forms:
                    fn()
            t = dict((name, []) for name, _ in forms)
            for _ in range(args.repeats):
                for name, fn in forms:
                    t[name].append(window(fn, args.calls))
            fmt = lambda v: "%.4f [%.4f]" % (min(v), max(v))
            note = ""
            if arm != "compact" and min(t["eager"]) > max(t["loop"]):
                note = "  eager frozen SLOWER than the loop beyond the window spread"
                slower.append((arm, prec, B))
            say("%-7s %-6s B=%-4d  loop %s  eager %s  graph %s  loop/eager %.3fx  loop/graph %.3fx%s"
                % (arm, prec, B, fmt(t["loop"]), fmt(t["eager"]), fmt(t["graph"]), min(t["loop"]) / min(t["eager"]),
                   min(t["loop"]) / min(t["graph"]), note))
        if prec == "fp32":
            say("%-7s C calls per step: loop %d, eager %d (a graph replay: one launch of the eager step's kernels)"
                % (arm, c_calls(f_loop), c_calls(f_eager)))
bnn_amd.set_precision("fp32")
say("full-shape frozen model slower than base_ensemble beyond the spread in %d rows%s"
    % (len(slower), (": " + ", ".join("%s %s B=%d" % r for r in slower)) if slower else ""))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
