#!/usr/bin/env python3
"""What the one-launch multi-group Adam costs and saves, as replay time of whole captured training steps (the method of
tools/base_step_time.py: device events around windows of graph replays, the forms alternating window by window, the fastest
window and the window spread reported).

Forms (each a graphs.make_graphed_train_step graph; one process per tree and form, so a process holds one graph):
  a        baseline LBBNN 784-400-600-10, B = 100, draws="hip", the reference's 33 single-tensor groups (LBBNN-GP-MF.py:520-554)
  b        the headline MNF net 784-1200-1200-10, planar flows, B = 4096, fp16x3f, one-group bnn_amd.optim.Adam(net.parameters())
  c_hook   form a with COND_OPT as register_hook(gr * l.gammas) on the three weight_mu
  c_mask   form a with COND_OPT as optimizer.set_grad_mask(weight_mu, lambda: l.gammas)
  d        form a with max_grad_norm = 1.0

    python tools/adam_groups_time.py                        # this tree, all forms
    python tools/adam_groups_time.py --parent DIR           # ... and forms a, b, c_hook of a built checkout of the parent
                                                            # commit in DIR: the trees' child processes alternate, form by form
    python tools/adam_groups_time.py --trace 1000 --form a  # replay one form (for `rocprofv3 --kernel-trace --stats`)

A tree without set_grad_mask / max_grad_norm (the parent) runs the forms it has."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--tree", default=HERE)
ap.add_argument("--worker", action="store_true")
ap.add_argument("--forms", default="a,b,c_hook,c_mask,d")
ap.add_argument("--windows", type=int, default=10)
ap.add_argument("--replays", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--trace", type=int, default=0)
ap.add_argument("--form", default="a")
args = ap.parse_args()


def summary(ws):
    return min(ws), (max(ws) - min(ws)) / min(ws)


if not args.worker and not args.trace:
    trees = [("this tree", HERE)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    windows = {name: {} for name, _ in trees}
    for rnd in range(args.rounds):
        for form in args.forms.split(","):
            for name, path in trees:                                   # alternating: this tree, parent, this tree, parent ...
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", path, "--forms", form,
                                    "--windows", str(args.windows), "--replays", str(args.replays)], capture_output=True,
                                   text=True, timeout=600)
                if r.returncode != 0:                                  # nothing more is started on the GPU after a failure
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit("worker for %s, form %s failed (%d)" % (name, form, r.returncode))
                res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                for f, ws in res.items():
                    windows[name].setdefault(f, []).extend(ws)
    print("graph replays, device events around windows of %d replays; %d windows per form (%d processes x %d: one process per tree and "
          "form, one graph per process, trees and forms alternating between processes); ms per step: fastest window, spread = "
          "(slowest - fastest) / fastest" % (args.replays, args.rounds * args.windows, args.rounds, args.windows))
    for name, _ in trees:
        for form, ws in windows[name].items():
            fastest, spread = summary(ws)
            print("  %-10s %-7s fastest %.4f ms  spread %.1f %%  (median window %.4f)"
                  % (name, form, fastest, 100 * spread, sorted(ws)[len(ws) // 2]))
    mine = windows["this tree"]
    if args.parent:
        par = windows["parent"]
        for form in ("a", "b", "c_hook"):
            if form in mine and form in par:
                print("  %s: this tree / parent = %.3f (parent's own spread %.1f %%)"
                      % (form, min(mine[form]) / min(par[form]), 100 * summary(par[form])[1]))
    if "c_mask" in mine and "c_hook" in mine:
        print("  c: mask / hooks = %.3f" % (min(mine["c_mask"]) / min(mine["c_hook"])))
    if "d" in mine and "a" in mine:
        print("  d: clipping costs %.4f ms per step (%.3f x)" % (min(mine["d"]) - min(mine["a"]), min(mine["d"]) / min(mine["a"])))
    sys.exit(0)

# ---- one process, one tree ---------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.abspath(args.tree))
import torch
import bnn_amd

assert os.path.abspath(os.path.dirname(bnn_amd.LIB_PATH)).startswith(os.path.abspath(args.tree)), bnn_amd.LIB_PATH
dev = torch.device("cuda:0")
HAVE_MASK = hasattr(bnn_amd.optim.Adam, "set_grad_mask")


def base_form(cond=None, clip=None):
    torch.manual_seed(0)
    net = bnn_amd.base.BayesianNetwork((784, 400, 600, 10)).to(dev).train()
    ls = (net.l1, net.l2, net.l3)
    rate = dict(bias_mu=1e-4, bias_rho=1e-4, weight_mu=1e-4, weight_rho=1e-4, pa=1e-3, pb=1e-3, weight_a=1e-5, weight_b=1e-5,
                bias_a=1e-5, bias_b=1e-5, lambdal=0.1)
    groups = [{"params": getattr(l, n), "lr": r} for n, r in rate.items() for l in ls]
    opt = bnn_amd.optim.Adam(groups, lr=1e-4, **({"max_grad_norm": clip} if clip else {}))
    for l in ls:
        if cond == "hook":
            l.weight_mu.register_hook(lambda gr, l=l: gr * l.gammas)
        elif cond == "mask":
            opt.set_grad_mask(l.weight_mu, lambda l=l: l.gammas)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(100, 1, 28, 28, generator=g).to(dev)
    y = torch.randint(0, 10, (100,), generator=g).to(dev)
    return bnn_amd.graphs.make_graphed_train_step(net, opt, lambda n, a, b: n.sample_elbo(a, b, draws="hip")[0], x, y)


def mnf_form():
    torch.manual_seed(0)
    net = bnn_amd.mnf.BayesianNetwork((784, 1200, 1200, 10), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
    net.set_precision("fp16x3f")
    opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-3)
    x = torch.rand(4096, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (4096,), device=dev)
    return bnn_amd.graphs.make_graphed_train_step(net, opt, lambda n, a, b: bnn_amd.elbo_loss(n(a, sample=True), b, n.kl(), 15), x, y)


BUILD = {"a": base_form, "b": mnf_form, "c_hook": lambda: base_form(cond="hook"),
         "c_mask": (lambda: base_form(cond="mask")) if HAVE_MASK else None, "d": (lambda: base_form(clip=1.0)) if HAVE_MASK else None}

if args.trace:
    step = BUILD[args.form]()
    for _ in range(args.trace):
        step.graph.replay()
    torch.cuda.synchronize()
    print("replayed form %s %d times" % (args.form, args.trace))
    sys.exit(0)

steps = {f: BUILD[f]() for f in args.forms.split(",") if BUILD.get(f) is not None}
for s in steps.values():
    for _ in range(30):
        s.graph.replay()
torch.cuda.synchronize()
res = {f: [] for f in steps}
for w in range(args.windows):
    for f, s in steps.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.replays):
            s.graph.replay()
        b.record()
        torch.cuda.synchronize()
        res[f].append(a.elapsed_time(b) / args.replays)
print(json.dumps(res))
