#!/usr/bin/env python3
"""Time of evaluate.explain against the torch spelling of the same numbers and against the forward alone, one process:
784-400-400-10 (LRT) and 784-1200-1200-10 (planar MNF, two transforms), median probability models as constructed, B in
{100, 1000}, every output and targets="pred".

  explain   evaluate.explain(fz, x[, targets="pred"]): the call as a user makes it -- forward with kept activations, the sweep
            (lbbnn_explain_step between mean-only lbbnn_lrt_gemm calls on transposed fp32 operands), every output tensor
  torch     the same on the device in torch: a forward on dense fp32 weights (an MNF model: the z of one explain call folded
            in once, outside the timed part) that keeps the masks, then per explained output one backward chain of matrix
            products through the masks, the bias dots, contributions = J * x; no host read
  forward   fz(x) alone, what a prediction costs

The forms alternate; each is timed --repeats times as a window of calls between two device events after a warm-up of all, and
reported as fastest window [slowest window] in ms per call.  The table goes to stdout and to --out (default
profiles/explain.txt; whatever that file holds from the line "Parity of the GPU tier" on is kept)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bnn_amd
from bnn_amd import evaluate

KEEP_FROM = "Parity of the GPU tier"

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10, help="calls per window")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("explain_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def torch_spelling(Ws, bs, x, pred):
    """logits, contributions (B, C', I) and intercept (B, C') of the ReLU chain, spelled in torch on the device."""
    h, masks = x, []
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = torch.relu(torch.addmm(b, h, W.t()))
        masks.append(h > 0)
    logits = torch.addmm(bs[-1], h, Ws[-1].t())
    outs = [torch.argmax(logits, 1)] if pred else [torch.full((x.shape[0],), c, device=dev) for c in range(Ws[-1].shape[0])]
    cons, ints = [], []
    for t in outs:
        g, k = Ws[-1][t], bs[-1][t]
        for l in range(len(Ws) - 2, -1, -1):
            g = g * masks[l]
            k = k + g @ bs[l]
            g = g @ Ws[l]
        cons.append(g * x)
        ints.append(k)
    return logits, torch.stack(cons, 1), torch.stack(ints, 1)


lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("evaluate.explain against its torch spelling and against fz(x) alone; per form %d windows (ms per call: fastest [slowest]), "
    "the forms alternating, after %d warm-up calls of each; %d calls per window" % (args.repeats, args.warmup, args.calls))
say("device: %s" % torch.cuda.get_device_name(0))
for family, dims in (("lrt", (784, 400, 400, 10)), ("mnf", (784, 1200, 1200, 10))):
    torch.manual_seed(0)
    if family == "lrt":
        net = bnn_amd.lrt.BayesianNetwork(dims)
    else:
        net = bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
    fz = evaluate.freeze(net.to(dev).eval(), "mpm")
    for B in (100, 1000):
        x = torch.randn(B, dims[0], device=dev)
        first = evaluate.explain(fz, x)
        Ws = [fz._buf("e0", i)[:, :dims[i]] * (first["z"][i][None, :] if family == "mnf" else 1.0) for i in range(len(dims) - 1)]
        Ws = [w.contiguous() for w in Ws]
        bs = [fz._buf("bias_mu", i) for i in range(len(dims) - 1)]
        for pred in (False, True):
            f_explain = lambda: evaluate.explain(fz, x, targets="pred" if pred else None)
            f_torch = lambda: torch_spelling(Ws, bs, x, pred)
            f_forward = lambda: fz(x)
            forms = (("explain", f_explain), ("torch", f_torch), ("forward", f_forward))
            for _ in range(args.warmup):
                for _, fn in forms:
                    fn()
            times = dict((name, []) for name, _ in forms)
            for _ in range(args.repeats):
                for name, fn in forms:
                    times[name].append(window(fn, args.calls))
            fmt = lambda v: "%.4f [%.4f]" % (min(v), max(v))
            say("%-4s %-18s B=%-5d %-5s explain %s  torch %s  forward %s  torch/explain %.2fx  explain/forward %.1fx"
                % (family, "-".join(map(str, dims)), B, "pred" if pred else "all", fmt(times["explain"]), fmt(times["torch"]),
                   fmt(times["forward"]), min(times["torch"]) / min(times["explain"]), min(times["explain"]) / min(times["forward"])))
kept = []
if os.path.exists(args.out):
    old = open(args.out).read().splitlines()
    at = [i for i, l in enumerate(old) if l.startswith(KEEP_FROM)]
    kept = [""] + old[at[0]:] if at else []
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines + kept) + "\n")
