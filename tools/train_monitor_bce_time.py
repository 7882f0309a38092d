#!/usr/bin/env python3
"""What the training monitor costs on the binary loss and the baseline family, by the method of
tools/train_monitor_time.py: device events around windows of graph replays, the forms alternating window by window or process
by process, the fastest window and the window spread reported.  Writes profiles/train_monitor_bce.txt.

  1. the loss launch alone: elbo_bce_loss with and without a monitor at B = 400, O = 1 (the simulation studies' batch) -- two
     graphs of 100 consecutive loss launches each in one process, their windows alternating;
  2. the graphed study steps at B = 400 on 20 covariates: examples/sim_study_synthetic.py's LRT and MNF networks (20 -> 1,
     sigmoid head, optim.Adam) and examples/sim_study_base_synthetic.py's baseline network (optim.SGD, eleven groups,
     sample_elbo(draws="hip"), the six prior groups at rate 0 as after the study's switch epoch) -- "off" (stats=, no monitor, no guard: the calls of the parent commit) and "on" (monitor=mon,
     optimizer.set_guard(mon); for the baseline also the whole ELBO in the one fused loss launch), one process per tree, study
     and form;

    python tools/train_monitor_bce_time.py                     # this tree
    python tools/train_monitor_bce_time.py --parent DIR        # ... and the "off" steps of a built checkout of the parent
                                                               # commit in DIR, the trees' processes alternating

There is no pass threshold.  Where the monitored step is slower than the parent's unmonitored step by more than the parent's
own window spread, the line says so."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUDIES = ("lrt", "mnf", "base")
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--tree", default=HERE)
ap.add_argument("--worker", default=None, choices=["loss"] + [s + "_" + f for s in STUDIES for f in ("off", "on")])
ap.add_argument("--windows", type=int, default=10)
ap.add_argument("--replays", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "train_monitor_bce.txt"))
args = ap.parse_args()


def fastest_spread(ws):
    return min(ws), (max(ws) - min(ws)) / min(ws)


def run_worker(tree, form):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", form, "--tree", tree, "--windows", str(args.windows),
                        "--replays", str(args.replays)], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:                                      # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("worker %s of %s failed (%d)" % (form, tree, r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


if args.worker is None:
    lines = []
    say = lambda s: (lines.append(s), print(s, flush=True))
    loss = run_worker(HERE, "loss")
    say("tools/train_monitor_bce_time.py: device events around windows of graph replays; ms or us per step / launch: fastest "
        "window, spread = (slowest - fastest) / fastest")
    say("1. the loss launch alone, B = 400, O = 1, kl given: graphs of 100 launches, %d windows of %d replays each, alternating"
        % (args.windows, args.replays))
    lw = {}
    for form in ("plain", "monitor"):
        f, s = fastest_spread(loss[form])
        lw[form] = f
        say("  %-8s fastest %.3f us  spread %.1f %%  (slowest %.3f us, median %.3f us)"
            % (form, 1e3 * f, 100 * s, 1e3 * max(loss[form]), 1e3 * sorted(loss[form])[len(loss[form]) // 2]))
    say("  monitor - plain = %+.3f us per launch" % (1e3 * (lw["monitor"] - lw["plain"])))
    say("2. the graphed study steps, 20 -> 1 with a sigmoid head, B = 400: %d windows of %d replays per form (%d processes x %d, "
        "one graph per process, forms alternating between processes)"
        % (args.rounds * args.windows, args.replays, args.rounds, args.windows))
    for study in STUDIES:
        forms = [("this tree", HERE, "off"), ("this tree", HERE, "on")] + \
                ([("parent", os.path.abspath(args.parent), "off")] if args.parent else [])
        windows, counted = {}, []
        for rnd in range(args.rounds):
            for name, path, form in forms:                     # alternating: off, on, parent, off, on, parent ...
                w = study + "_" + form
                got = run_worker(path, w)
                windows.setdefault((name, form), []).extend(got[w])
                if "monitor" in got:
                    counted.append(got["monitor"])
        best = {}
        for (name, form), ws in windows.items():
            f, s = fastest_spread(ws)
            best[(name, form)] = (f, s)
            say("  %-4s %-10s %-4s fastest %.4f ms  spread %.1f %%  (slowest %.4f ms, median %.4f ms)"
                % (study, name, form, f, 100 * s, max(ws), sorted(ws)[len(ws) // 2]))
        off, on = best[("this tree", "off")][0], best[("this tree", "on")][0]
        say("  %-4s on - off = %+.2f us per step; the monitors counted %d steps, %d non-finite, %d skipped"
            % (study, 1e3 * (on - off), sum(c[0] for c in counted), sum(c[1] for c in counted), sum(c[2] for c in counted)))
        if args.parent:
            par, spread = best[("parent", "off")]
            say("  %-4s off / parent = %.4f; on - parent = %+.2f us; the parent's own spread is %.1f %% = %.2f us: the monitored "
                "step is %s" % (study, off / par, 1e3 * (on - par), 100 * spread, 1e3 * spread * par,
                                "within it" if on - par <= spread * par else "SLOWER than the parent's step by more than it"))
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
B, FEATURES, NUM_BATCHES = 400, 20, 5


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


gen = torch.Generator().manual_seed(0)
if args.worker == "loss":
    LAUNCHES = 100
    p = torch.sigmoid(torch.randn(B, 1, generator=gen)).to(dev)
    y = (torch.rand(B, 1, generator=gen) > 0.5).float().to(dev)
    kl = torch.tensor(1234.5, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    mon = bnn_amd.TrainMonitor(1, dev)
    graphs = {}
    with torch.no_grad():
        for name, kw in (("plain", {"stats": st}), ("monitor", {"monitor": mon})):
            bnn_amd.elbo_bce_loss(p, y, kl, NUM_BATCHES, **kw)
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(LAUNCHES):
                    out = bnn_amd.elbo_bce_loss(p, y, kl, NUM_BATCHES, **kw)
    res = timed(graphs)
    print(json.dumps({f: [w / LAUNCHES for w in ws] for f, ws in res.items()}))
    sys.exit(0)

study, form = args.worker.split("_")
x = torch.randn(B, FEATURES, generator=gen).to(dev)
y = (torch.rand(B, 1, generator=gen) > 0.5).float().to(dev)
torch.manual_seed(1)
if study == "base":
    net = bnn_amd.base.BayesianNetwork((FEATURES, 1), head="sigmoid", weight_mu_init=(-0.01, 0.01),
                                       lambdal_init=(-0.5, 0.5)).to(dev).train()
    rates = [("bias_mu", 1e-4), ("bias_rho", 1e-4), ("weight_mu", 1e-4), ("weight_rho", 1e-4), ("pa", 1e-3), ("pb", 1e-3),
             ("weight_a", 1e-3), ("weight_b", 1e-3), ("bias_a", 1e-3), ("bias_b", 1e-3), ("lambdal", 1e-3)]
    opt = bnn_amd.optim.SGD([{"params": getattr(net.l1, n), "lr": r} for n, r in rates], lr=0.01)
    # The six prior groups at rate 0, the study's state after its switch epoch (450 of its 500 epochs): the same launches, the
    # rates are rows of a device table.  With the priors trainable this one batch, replayed, makes weight_b (a Gamma rate)
    # negative in its 477th step and every later loss NaN -- which the "on" form's monitor counts and its guard skips (cheaper
    # steps: not what is to be timed), and the "off" form trains into every parameter unseen.
    for i in range(4, 10):
        opt.param_groups[i]["lr"] = 0.0
else:
    priors = bnn_amd.Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
    if study == "lrt":
        net = bnn_amd.lrt.BayesianNetwork((FEATURES, 1), head="sigmoid", priors=priors, lambdal_init=(1.5, 2.5))
    else:
        net = bnn_amd.mnf.BayesianNetwork((FEATURES, 1), 2, z_flow_type="Planar", r_flow_type="Planar", head="sigmoid",
                                          priors=priors, lambdal_init=(1.5, 2.5))
    net = net.to(dev).train()
    opt = bnn_amd.optim.Adam(net.parameters(), lr=0.01)
if form == "on":
    mon = bnn_amd.TrainMonitor(1, dev)
    opt.set_guard(mon)
    kw = {"monitor": mon}
else:
    kw = {"stats": torch.zeros(4, dtype=torch.int32, device=dev)}
if study == "base":
    lf = lambda n, a, b: n.sample_elbo(a, b, num_batches=NUM_BATCHES, draws="hip", **kw)[0]
else:
    lf = lambda n, a, b: bnn_amd.elbo_bce_loss(n(a, sample=True), b, n.kl(), NUM_BATCHES, **kw)
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)
res = timed({args.worker: step.graph})
if form == "on":                                               # a skipped step would be a cheaper step: say how many there were
    r = mon.result(strict=False)
    res["monitor"] = [r["steps"], r["nonfinite_steps"], r["skipped_steps"]]
print(json.dumps(res))
