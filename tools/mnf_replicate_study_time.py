#!/usr/bin/env python3
"""Time of an MNF replicate study on one MI355X: R one-layer planar-MNF networks 20 -> 1 (two transforms per flow) with a sigmoid
head, N = 2000 rows, batches of 400, --epochs epochs (default 20: 100 steps per network), in two spellings:

  fit    bnn_amd.study.fit_mnf_replicates(nets, x, y, ...): all R networks in the launches of lbbnn_mnf_study_fit (one workgroup
         per network), the whole call -- stacking the parameters, the launches, copying the trained values back
  loop   what the package offered before: R networks, each trained by its OWN captured step (graphs.make_graphed_train_step,
         bnn_amd.optim.Adam with three groups behind the monitor's guard), one after the other.  Building the R graphs is NOT
         in the window.

Host clock around whole calls that end in a synchronise; --windows windows of each spelling, interleaved (fit, loop, fit, ...),
after one warm-up of each.  Written to profiles/mnf_replicate_study.txt:
  R = 100  fit against loop, every window, and whether the slowest fit window beats the fastest loop window
  R = 1    one workgroup against one graph
  R = 1000 fit alone
  the time per step per replicate of each, beside fit_replicates (the LRT kernel) at R = 100 and R = 1000 in the same run.

    python tools/mnf_replicate_study_time.py"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bnn_amd
from bnn_amd import Priors, study

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnf_replicate_study.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mnf_replicate_study_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
I, O, N, B, T = 20, 1, 2000, 400, 2
NB = N // B
PRIORS = Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
g = torch.Generator().manual_seed(3)
w_true = torch.zeros(I)
w_true[[1, 4, 9, 12, 17]] = torch.tensor([2.0, -1.5, 1.0, -2.5, 1.5])
x = torch.randn(N, I, generator=g)
y = (torch.rand(N, generator=g) < torch.sigmoid(x @ w_true)).float().reshape(N, 1)
x, y = x.to(dev), y.to(dev)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def make_loop(R):
    """R networks with a captured step each; returns run() that trains all of them for args.epochs epochs, one after the other."""
    nets = study.make_mnf_replicates(R, (I, O), num_transforms=T, priors=PRIORS, device=dev)
    steps = []
    for net in nets:
        net.train()
        l1 = net.l1
        named = [getattr(l1, n) for n in l1._names]
        opt = bnn_amd.optim.Adam([{"params": named, "lr": 0.01}, {"params": list(l1.z_flow.parameters()), "lr": 0.004},
                                  {"params": list(l1.r_flow.parameters()), "lr": 0.0035}], lr=0.01)
        mon = bnn_amd.TrainMonitor(O, dev)
        opt.set_guard(mon)

        def elbo(net, data, target, mon=mon):
            return bnn_amd.elbo_bce_loss(net(data, sample=True), target, net.kl(), NB, monitor=mon)
        steps.append(bnn_amd.graphs.make_graphed_train_step(net, opt, elbo, x[:B], y[:B]))

    def run():
        for step in steps:
            for _ in range(args.epochs):
                for k in range(NB):
                    step(x[k * B:(k + 1) * B], y[k * B:(k + 1) * B])
    return run


def make_fit(R):
    nets = study.make_mnf_replicates(R, (I, O), num_transforms=T, priors=PRIORS, device=dev)
    return lambda: study.fit_mnf_replicates(nets, x, y, args.epochs, B, lr=0.01, lr_z_flow=0.004, lr_r_flow=0.0035, seeds=list(range(R)))


def make_lrt_fit(R):
    nets = study.make_replicates(R, (I, O), priors=PRIORS, device=dev)
    return lambda: study.fit_replicates(nets, x, y, args.epochs, B, lr=0.01, seeds=list(range(R)))


def fmt(ts):
    return "[" + " ".join("%.4f" % t for t in ts) + "]"


say("MNF replicate study (bnn_amd.study.fit_mnf_replicates, lbbnn_mnf_study_fit) against the loop of captured steps, one MI355X, one process.")
say()
say("    python tools/mnf_replicate_study_time.py")
say()
say("planar MNF 20 -> 1, %d transforms per flow, sigmoid head, N = %d, batch %d, %d epochs = %d steps per network; host clock, whole"
    % (T, N, B, args.epochs, args.epochs * NB))
say("calls ending in a synchronise, %d windows of each spelling, interleaved, after one warm-up of each; seconds per window" % args.windows)
steps_per_net = args.epochs * NB
for R in (100, 1):
    fit, loop = make_fit(R), make_loop(R)
    clock(fit), clock(loop)
    tf, tl = [], []
    for _ in range(args.windows):
        tf.append(clock(fit))
        tl.append(clock(loop))
    say("R = %4d  fit %s slowest %.4f   loop %s fastest %.4f   fastest loop / slowest fit %.1fx   slowest fit < fastest loop: %s"
        % (R, fmt(tf), max(tf), fmt(tl), min(tl), min(tl) / max(tf), max(tf) < min(tl)))
    say("          per step per replicate: fit %.3f us (fastest window), loop %.3f us"
        % (min(tf) / (R * steps_per_net) * 1e6, min(tl) / (R * steps_per_net) * 1e6))
    del fit, loop
for R in (100, 1000):
    fit, lrt = make_fit(R), make_lrt_fit(R)
    clock(fit), clock(lrt)
    tf, tl = [], []
    for _ in range(args.windows):
        tf.append(clock(fit))
        tl.append(clock(lrt))
    say("R = %4d  MNF fit %s fastest %.4f = %.3f us per step per replicate   LRT fit (fit_replicates) %s fastest %.4f = %.3f us"
        % (R, fmt(tf), min(tf), min(tf) / (R * steps_per_net) * 1e6, fmt(tl), min(tl), min(tl) / (R * steps_per_net) * 1e6))
    del fit, lrt
say()
say("Not measured: other shapes than 20 -> 1 or other transform counts, per-replicate data sets, the kernel's time apart from the")
say("call's host work (stacking and copying back R networks' parameters is inside the fit windows), device counters, a second")
say("process on the device.")
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
