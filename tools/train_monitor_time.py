#!/usr/bin/env python3
"""What the training monitor and the guarded optimizer step cost, by the method of tools/adam_groups_time.py:
device events around windows of graph replays, the forms alternating window by window or process by process, the fastest
window and the window spread reported.  Writes profiles/train_monitor.txt.

  1. the loss launch alone: elbo_loss with and without a monitor at B = 4096, C = 10 -- two graphs of 100 consecutive loss
     launches each in one process, their windows alternating;
  2. the headline graphed training step: MNF 784-1200-1200-10, planar flows, B = 4096, fp16x3f, bnn_amd.optim.Adam --
     "off" (no monitor, no guard: the calls of the parent commit) and "on" (elbo_loss(monitor=mon), optimizer.set_guard(mon)),
     one process per tree and form;

    python tools/train_monitor_time.py                     # this tree
    python tools/train_monitor_time.py --parent DIR        # ... and the "off" step of a built checkout of the parent commit in
                                                           # DIR, the trees' processes alternating

The condition the numbers are read against: "off" lies within the parent's own window spread of the parent's step (it makes
the same calls), and "on" within that spread plus the loss-launch difference of part 1."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--tree", default=HERE)
ap.add_argument("--worker", default=None, choices=["loss", "off", "on"])
ap.add_argument("--windows", type=int, default=10)
ap.add_argument("--replays", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "train_monitor.txt"))
args = ap.parse_args()


def fastest_spread(ws):
    return min(ws), (max(ws) - min(ws)) / min(ws)


def run_worker(tree, form):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", form, "--tree", tree, "--windows", str(args.windows),
                        "--replays", str(args.replays)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:                                      # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("worker %s of %s failed (%d)" % (form, tree, r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


if args.worker is None:
    lines = []
    say = lambda s: (lines.append(s), print(s))
    loss = run_worker(HERE, "loss")
    forms = [("this tree", HERE, "off"), ("this tree", HERE, "on")] + \
            ([("parent", os.path.abspath(args.parent), "off")] if args.parent else [])
    windows = {}
    for rnd in range(args.rounds):
        for name, path, form in forms:                         # alternating: off, on, parent, off, on, parent ...
            windows.setdefault((name, form), []).extend(run_worker(path, form)[form])
    say("tools/train_monitor_time.py: device events around windows of graph replays; ms or us per step / launch: fastest window, "
        "spread = (slowest - fastest) / fastest")
    say("1. the loss launch alone, B = 4096, C = 10, kl given: graphs of 100 launches, %d windows of %d replays each, alternating"
        % (args.windows, args.replays))
    lw = {}
    for form in ("plain", "monitor"):
        f, s = fastest_spread(loss[form])
        lw[form] = f
        say("  %-8s fastest %.3f us  spread %.1f %%  (slowest %.3f us, median %.3f us)"
            % (form, 1e3 * f, 100 * s, 1e3 * max(loss[form]), 1e3 * sorted(loss[form])[len(loss[form]) // 2]))
    d_loss = lw["monitor"] - lw["plain"]
    say("  monitor - plain = %+.3f us per launch" % (1e3 * d_loss))
    say("2. the graphed training step, MNF 784-1200-1200-10 planar, B = 4096, fp16x3f, optim.Adam: %d windows of %d replays per form "
        "(%d processes x %d, one graph per process, forms alternating between processes)"
        % (args.rounds * args.windows, args.replays, args.rounds, args.windows))
    best = {}
    for (name, form), ws in windows.items():
        f, s = fastest_spread(ws)
        best[(name, form)] = (f, s)
        say("  %-10s %-4s fastest %.4f ms  spread %.1f %%  (slowest %.4f ms, median %.4f ms)"
            % (name, form, f, 100 * s, max(ws), sorted(ws)[len(ws) // 2]))
    off, on = best[("this tree", "off")][0], best[("this tree", "on")][0]
    say("  on - off = %+.2f us per step" % (1e3 * (on - off)))
    if args.parent:
        par, spread = best[("parent", "off")]
        say("  off / parent = %.4f; the parent's own spread is %.1f %%: %s"
            % (off / par, 100 * spread, "within it" if abs(off - par) <= spread * par else "OUTSIDE it"))
        bound = spread * par + max(d_loss, 0.0)
        say("  on - parent = %+.2f us; spread of the parent + loss-launch difference = %.2f us: %s"
            % (1e3 * (on - par), 1e3 * bound, "within it" if on - par <= bound else "OUTSIDE it"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0)

# ---- one process, one tree ---------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.abspath(args.tree))
import torch
import bnn_amd

assert os.path.abspath(os.path.dirname(bnn_amd.LIB_PATH)).startswith(os.path.abspath(args.tree)), bnn_amd.LIB_PATH
dev = torch.device("cuda:0")


def timed(graphs):
    """{name: [ms per replay of each window]}, the graphs' windows alternating."""
    for g in graphs.values():
        for _ in range(30):
            g.replay()
    torch.cuda.synchronize()
    res = {f: [] for f in graphs}
    for _ in range(args.windows):
        for f, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.replays):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            res[f].append(a.elapsed_time(b) / args.replays)
    return res


if args.worker == "loss":
    LAUNCHES = 100
    g = torch.Generator().manual_seed(0)
    lp = torch.log_softmax(torch.randn(4096, 10, generator=g), dim=1).to(dev)
    y = torch.randint(0, 10, (4096,), generator=g).to(dev)
    kl = torch.tensor(1234.5, device=dev)
    mon = bnn_amd.TrainMonitor(10, dev)
    graphs = {}
    with torch.no_grad():
        for name, kw in (("plain", {}), ("monitor", {"monitor": mon})):
            bnn_amd.elbo_loss(lp, y, kl, 15, **kw)
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(LAUNCHES):
                    out = bnn_amd.elbo_loss(lp, y, kl, 15, **kw)
    res = timed(graphs)
    print(json.dumps({f: [w / LAUNCHES for w in ws] for f, ws in res.items()}))
    sys.exit(0)

torch.manual_seed(0)
net = bnn_amd.mnf.BayesianNetwork((784, 1200, 1200, 10), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
net.set_precision("fp16x3f")
opt = bnn_amd.optim.Adam(net.parameters(), lr=1e-3)
kw = {}
if args.worker == "on":
    mon = bnn_amd.TrainMonitor(10, dev)
    opt.set_guard(mon)
    kw = {"monitor": mon}
x = torch.rand(4096, 1, 28, 28, device=dev)
y = torch.randint(0, 10, (4096,), device=dev)
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lambda n, a, b: bnn_amd.elbo_loss(n(a, sample=True), b, n.kl(), 15, **kw), x, y)
print(json.dumps(timed({args.worker: step.graph})))
