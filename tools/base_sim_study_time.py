#!/usr/bin/env python3
"""Time of the baseline simulation study's training step on one MI355X (examples/sim_study_base_synthetic.py: 20 -> 1, B = 400,
eleven single-tensor SGD groups), and of the SGD step by itself.

Training step, ms per step, two spellings alternating window by window (the method of tools/binary_head_time.py: device events
around windows of --replays steps, --windows windows each after a warm-up of both; fastest window and spread = slowest / fastest - 1):

  graph   base.BayesianNetwork((20, 1), head="sigmoid").sample_elbo(draws="hip", stats=...) + bnn_amd.optim.SGD, replayed from a
          HIP graph (graphs.make_graphed_train_step)
  eager   what could be written before the head and the SGD existed, run eagerly because torch.optim.SGD's rates are host numbers
          that a captured step cannot follow: layer.sample_forward(x), torch.sigmoid, nn.BCELoss(reduction='sum') +
          (log_q - log_prior) / N, torch.optim.SGD with the same eleven groups

Optimizer step alone (gradients fixed, eager calls, the host included -- the cost a launch-bound step pays), three optimizers
alternating: bnn_amd.optim.SGD, torch.optim.SGD, bnn_amd.optim.Adam; at the study's 11 groups and at the 33 single-tensor groups of
tools/adam_groups_time.py (784-400-600-10); and the two device-table optimizers replayed from a graph.  No time here is a pass
condition.

Every rate is 0 while the training step is timed: the launches are the ones of any other rate, the parameters stay at their
seeded values, and every window times the same work.  nn.BCELoss asserts on the device that its input lies in [0, 1], which ends
the process on a NaN probability, so the tool checks that both forms are finite before and after the windows."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd

ap = argparse.ArgumentParser()
ap.add_argument("--replays", type=int, default=300)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--warmup", type=int, default=30)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("base_sim_study_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
B, N = 400, 5
STUDY = dict(weight_mu_init=(-0.01, 0.01), lambdal_init=(-0.5, 0.5))
RATES = [("bias_mu", 1e-4), ("bias_rho", 1e-4), ("weight_mu", 1e-4), ("weight_rho", 1e-4), ("pa", 1e-3), ("pb", 1e-3),
         ("weight_a", 1e-3), ("weight_b", 1e-3), ("bias_a", 1e-3), ("bias_b", 1e-3), ("lambdal", 1e-3)]
g = torch.Generator().manual_seed(1)
x = torch.randn(B, 20, generator=g).to(dev)
y = (torch.rand(B, generator=g) > 0.5).float().to(dev)
bce = torch.nn.BCELoss(reduction="sum")


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def rounds(fns, calls):
    for _ in range(args.warmup):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(args.windows):
        for t, f in zip(ts, fns):
            t.append(window(f, calls))
    return ts


fmt = lambda v: " ".join("%.4f" % u for u in v)
spread = lambda v: max(v) / min(v) - 1.0
report = lambda name, t: "%s [%s] fastest %.4f spread %.1f%%" % (name, fmt(t), min(t), 100 * spread(t))
print("B = %d, %d batches per epoch; per form %d windows of %d steps (ms per step, device events), the forms alternating, after %d "
      "warm-up steps of each" % (B, N, args.windows, args.replays, args.warmup))

# ---- the training step ------------------------------------------------------------------------------------------------------
torch.manual_seed(0)
net_g = bnn_amd.base.BayesianNetwork((20, 1), head="sigmoid", **STUDY).to(dev).train()
torch.manual_seed(0)
net_e = bnn_amd.base.BayesianNetwork((20, 1), **STUDY).to(dev).train()
groups = lambda net: [{"params": getattr(net.l1, n), "lr": 0.0 * r} for n, r in RATES]
opt_g, opt_e = bnn_amd.optim.SGD(groups(net_g), lr=0.01), torch.optim.SGD(groups(net_e), lr=0.01)
st = torch.zeros(4, dtype=torch.int32, device=dev)
step_g = bnn_amd.graphs.make_graphed_train_step(
    net_g, opt_g, lambda n, a, b: n.sample_elbo(a, b, num_batches=N, draws="hip", stats=st)[0], x, y)
xs, ys = step_g.inputs
y1 = y.reshape(B, 1)


def step_e():
    opt_e.zero_grad(set_to_none=True)
    out, lp, lq = net_e.l1.sample_forward(x)
    (bce(torch.sigmoid(out), y1) + (lq - lp) / N).backward()
    opt_e.step()


with torch.no_grad():                                           # nn.BCELoss asserts its input range on the device: look first
    assert bool(torch.isfinite(net_e.l1.sample_forward(x)[0]).all()) and bool(torch.isfinite(step_g(xs, ys)))
tg, te = rounds([lambda: step_g(xs, ys), step_e], args.replays)
assert st.tolist()[3] == 0 and all(bool(torch.isfinite(p).all()) for n in (net_g, net_e) for p in n.parameters())
print("training step 20-1  %s  %s  eager / graph %.2fx" % (report("graph", tg), report("eager", te), min(te) / min(tg)))

# ---- the optimizer step alone -----------------------------------------------------------------------------------------------


def optimizers(named):
    """The three optimizers over clones of the same tensors, one single-tensor group each, fixed gradients."""
    out = []
    for make in (lambda gs: bnn_amd.optim.SGD(gs, lr=0.01), lambda gs: torch.optim.SGD(gs, lr=0.01),
                 lambda gs: bnn_amd.optim.Adam(gs, lr=0.01)):
        ps = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
        for p in ps:
            p.grad = torch.full_like(p, 1e-3)
        out.append(make([{"params": [p], "lr": 1e-4 * (1 + i % 3)} for i, p in enumerate(ps)]))
    return out


torch.manual_seed(0)
big = bnn_amd.base.BayesianNetwork((784, 400, 600, 10)).to(dev)
for name, named in (("11 groups (20-1)", list(net_e.named_parameters())), ("33 groups (784-400-600-10)", list(big.named_parameters()))):
    ours, ref, adam = optimizers(named)
    t = rounds([ours.step, ref.step, adam.step], args.replays)
    print("optimizer step, eager, %s  %s  %s  %s  torch SGD / SGD %.2fx  Adam / SGD %.2fx"
          % (name, report("SGD", t[0]), report("torch.optim.SGD", t[1]), report("Adam", t[2]), min(t[1]) / min(t[0]), min(t[2]) / min(t[0])))
    graphs = []
    for o in (ours, adam):
        gr = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with bnn_amd.graphs.capture(gr):
            o.step()
        graphs.append(gr)
    t = rounds([graphs[0].replay, graphs[1].replay], args.replays)
    print("optimizer step, graph replay, %s  %s  %s  Adam / SGD %.2fx" % (name, report("SGD", t[0]), report("Adam", t[1]), min(t[1]) / min(t[0])))
