#!/usr/bin/env python3
"""Time of the binary (sigmoid) head on one MI355X: the two networks of examples/sim_study_synthetic.py (LRT 20 -> 1 and MNF 20 -> 1
with two planar transforms), B = 400, whole training steps replayed from a HIP graph (graphs.make_graphed_train_step,
bnn_amd.optim.Adam), in two spellings:

  head    net = BayesianNetwork((20, 1), head="sigmoid");  elbo_bce_loss(net(x, sample=True), y, net.kl(), N, stats=st)
  layers  what can be written without the head: the layer called by itself, torch.sigmoid on its output,
          nn.BCELoss(reduction='sum')(p, y) + layer.kl / N

and one evaluation pass per batch at S = 10 members, B = 100:

  head    evaluate_batches(freeze(net), [(x, y)], 10, acc=..., uncertainty=...) -- the frozen ensemble, the posterior-mean forward,
          lbbnn_eval_metrics and lbbnn_eval_uncertainty with two classes, one read of the totals
  layers  ten layer calls + torch.sigmoid, the member mean, its accuracy and BCE and the posterior-mean accuracy in torch ops, one
          read of the totals

Device events around windows of --replays steps, the two spellings alternating, --windows windows each after a warm-up of both;
the fastest window and the spread (slowest / fastest - 1) of each spelling are printed.  Kernel launches per step are counted by
torch.profiler on one eager step of each spelling after the timing (--no-count skips that)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bnn_amd
from bnn_amd import Priors, evaluate, layers

ap = argparse.ArgumentParser()
ap.add_argument("--replays", type=int, default=300)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--no-count", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("binary_head_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")
B, N, S, EB = 400, 5, 10, 100
PRIORS = Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)


def make(kind, head):
    torch.manual_seed(0)
    kw = dict(priors=PRIORS, lambdal_init=(1.5, 2.5), head=head)
    if kind == "mnf":
        net = bnn_amd.mnf.BayesianNetwork((20, 1), 2, z_flow_type="Planar", r_flow_type="Planar", **kw)
    else:
        net = bnn_amd.lrt.BayesianNetwork((20, 1), **kw)
    return net.to(dev)


g = torch.Generator().manual_seed(1)
x = torch.randn(B, 20, generator=g).to(dev)
y = (torch.rand(B, 1, generator=g) > 0.5).float().to(dev)
ex, ey = x[:EB].contiguous(), y[:EB].contiguous()
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


def pair(f0, f1, calls):
    for _ in range(args.warmup):
        f0()
        f1()
    t0, t1 = [], []
    for _ in range(args.windows):
        t0.append(window(f0, calls))
        t1.append(window(f1, calls))
    return t0, t1


def launches(fn):
    """(kernels, copies / fills) the device ran for one call of fn."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    other = [e for e in ev if e.name.lower().startswith(("memcpy", "memset"))]
    return len(ev) - len(other), len(other)


fmt = lambda v: " ".join("%.4f" % u for u in v)
spread = lambda v: max(v) / min(v) - 1.0
print("B = %d training rows, %d batches per epoch; evaluation S = %d members, B = %d; per spelling %d windows of %d steps (ms per "
      "step, device events), the spellings alternating, after %d warm-up steps of each"
      % (B, N, S, EB, args.windows, args.replays, args.warmup))

for kind in ("lrt", "mnf"):
    # ---- training step
    net_h, net_l = make(kind, "sigmoid").train(), make(kind, "log_softmax").train()
    st = torch.zeros(4, dtype=torch.int32, device=dev)

    def loss_head(n, a, b):
        return bnn_amd.elbo_bce_loss(n(a, sample=True), b, n.kl(), N, stats=st)

    def loss_layers(n, a, b):
        return bce(torch.sigmoid(n.l1(a, sample=True)), b) + n.l1.kl / N

    opt_h, opt_l = (bnn_amd.optim.Adam(n.parameters(), lr=0.01) for n in (net_h, net_l))
    step_h = bnn_amd.graphs.make_graphed_train_step(net_h, opt_h, loss_head, x, y)
    step_l = bnn_amd.graphs.make_graphed_train_step(net_l, opt_l, loss_layers, x, y)
    xs, ys = step_h.inputs
    xl, yl = step_l.inputs
    th, tl = pair(lambda: step_h(xs, ys), lambda: step_l(xl, yl), args.replays)
    print("%s 20-1 training step  head [%s] fastest %.4f spread %.1f%%  layers [%s] fastest %.4f spread %.1f%%  layers / head %.2fx"
          % (kind, fmt(th), min(th), 100 * spread(th), fmt(tl), min(tl), 100 * spread(tl), min(tl) / min(th)))

    # ---- evaluation pass
    net_h.eval()
    net_l.eval()
    fz = evaluate.freeze(net_h)
    acc, unc = evaluate.EvalAccumulator(2, S, dev), evaluate.UncertaintyAccumulator(2, S, dev)
    tot = torch.zeros(3, dtype=torch.float64, device=dev)

    def eval_head():
        evaluate.evaluate_batches(fz, [(ex, ey)], S, acc=acc, uncertainty=unc)

    @torch.no_grad()
    def eval_layers():
        p = torch.stack([torch.sigmoid(net_l.l1(ex, sample=True)) for _ in range(S)])
        pm = p.mean(0)
        mean = torch.sigmoid(net_l.l1(ex, sample=False))
        tot.add_(torch.stack([((pm > 0.5) == (ey > 0.5)).sum().double(), bce(pm, ey).double(),
                              ((mean > 0.5) == (ey > 0.5)).sum().double()]))
        tot.tolist()

    eh, el = pair(eval_head, eval_layers, max(1, args.replays // 3))
    print("%s 20-1 evaluation pass  head [%s] fastest %.4f spread %.1f%%  layers [%s] fastest %.4f spread %.1f%%  layers / head %.2fx"
          % (kind, fmt(eh), min(eh), 100 * spread(eh), fmt(el), min(el), 100 * spread(el), min(el) / min(eh)))

    if not args.no_count:
        net_h.train()
        net_l.train()

        def eager(n, opt, lf):
            def run():
                opt.zero_grad(set_to_none=True)
                with layers.vector_backward_overlap():
                    lf(n, x, y).backward()
                opt.step()
            return run

        kh, kl_ = launches(eager(net_h, opt_h, loss_head)), launches(eager(net_l, opt_l, loss_layers))
        net_h.eval()
        net_l.eval()
        vh, vl = launches(eval_head), launches(eval_layers)
        print("%s 20-1 launches per training step (kernels, copies / fills): head %s  layers %s;  per evaluation pass: head %s  layers %s"
              % (kind, kh, kl_, vh, vl))
