#!/usr/bin/env python3
"""The reference's baseline-LBBNN training loop (LBBNN-GP-MF.py:327-338: net.zero_grad(), net.sample_elbo(data, target),
loss.backward(), the COND_OPT mask weight_mu.grad * gammas, optimizer.step()) with its 33-group Adam (:520-554) as
bnn_amd.optim.Adam, on MNIST-shaped synthetic data (there is no dataset in this image).  The step draws its gates and Gamma
precisions inside the HIP kernels (sample_elbo(draws="hip")), so it is captured once in a HIP graph and replayed.  The ELBO is
one fused loss launch that also keeps the epoch's totals on the device (monitor=), and Adam runs behind the monitor's guard: a
step whose loss is not finite changes no parameter and is counted.

    python examples/train_base_synthetic.py               # graphed hip-draw step
    EAGER=1 python examples/train_base_synthetic.py       # the same step, eager
    COND_OPT=1 python examples/train_base_synthetic.py    # mask the weight_mu gradients with the drawn gates (:333-336)
    DECAY=1 python examples/train_base_synthetic.py       # halve every group's rate each epoch (lr_scheduler, same graph)

It ends with the reference's evaluation on a held-out synthetic batch: bnn_amd.evaluate.ensemble_eval (test_ensemble) and the
accuracy and predictive entropy of the median probability model (outofsample(medimod=True)).
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd.base import BayesianNetwork

DEVICE = torch.device("cuda:0")
BATCH_SIZE, NUM_BATCHES, EPOCHS = 100, 60, 4
COND_OPT = os.environ.get("COND_OPT") == "1"
DECAY = os.environ.get("DECAY") == "1"
torch.manual_seed(0)                                   # also seeds the in-kernel draws

net = BayesianNetwork().to(DEVICE)                     # 784-400-600-10
ls = (net.l1, net.l2, net.l3)
groups = ([{"params": l.bias_mu, "lr": 1e-4} for l in ls] + [{"params": l.bias_rho, "lr": 1e-4} for l in ls]
          + [{"params": l.weight_mu, "lr": 1e-4} for l in ls] + [{"params": l.weight_rho, "lr": 1e-4} for l in ls]
          + [{"params": l.pa, "lr": 1e-3} for l in ls] + [{"params": l.pb, "lr": 1e-3} for l in ls]
          + [{"params": l.weight_a, "lr": 1e-5} for l in ls] + [{"params": l.weight_b, "lr": 1e-5} for l in ls]
          + [{"params": l.bias_a, "lr": 1e-5} for l in ls] + [{"params": l.bias_b, "lr": 1e-5} for l in ls]
          + [{"params": l.lambdal, "lr": 0.1} for l in ls])
optimizer = bnn_amd.optim.Adam(groups, lr=1e-4)
if COND_OPT:
    # weight_mu.grad * gammas.data (:333-336) as a gradient mask of the optimizer: the callable is resolved when step() runs, so
    # under the capture it is the graph's gammas buffer, rewritten by every replay; the product happens inside the update
    # launch (a register_hook(lambda gr: gr * l.gammas) per layer does the same with three more kernels)
    for l in ls:
        optimizer.set_grad_mask(l.weight_mu, lambda l=l: l.gammas)
# the rates live in a device table that the captured update reads, so a scheduler works under the ONE graph: step() below
# pushes the groups' current values before every replay (a copy only when one changed)
scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=1, gamma=0.5) if DECAY else None
# The reference's switch at epoch 20 (:559-604) builds a new optimizer with rate 0 for pa / pb / weight_a / weight_b / bias_a /
# bias_b and 1e-4 for lambdal: here that part is `group["lr"] = ...` on this optimizer, no re-capture.  The same switch also
# sets the priors' `exact` flags, which are host values baked into the captured kernels' arguments: that part still needs
# a new make_graphed_train_step.

g = torch.Generator(device=DEVICE).manual_seed(7)
proj = torch.randn(784, 10, device=DEVICE, generator=g)
train_x = torch.rand(NUM_BATCHES, BATCH_SIZE, 1, 28, 28, device=DEVICE, generator=g)
train_y = (train_x.view(NUM_BATCHES, BATCH_SIZE, 784) @ proj).argmax(-1)


# the reference's train() reads loss, log_prior, log_q and nll back (:339-342); here one read per epoch
monitor = bnn_amd.TrainMonitor(10, DEVICE)
optimizer.set_guard(monitor)


def elbo(net, data, target):
    return net.sample_elbo(data, target, draws="hip", monitor=monitor)[0]


net.train()
if os.environ.get("EAGER") == "1":
    def step(data, target):
        net.zero_grad()
        loss = elbo(net, data, target)
        loss.backward()
        optimizer.step()
        return loss
else:
    step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, train_x[0], train_y[0])

for epoch in range(EPOCHS):
    monitor.reset()                                    # (also drops the warm-up steps of the graphed step's factory)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for b in range(NUM_BATCHES):
        loss = step(train_x[b], train_y[b])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / NUM_BATCHES * 1e3
    m = monitor.result()                               # the epoch's one host read
    print("epoch %d  loss_mean %.1f  nll_mean %.4f  accuracy %.3f  nonfinite_steps %d  skipped_steps %d  (%.3f ms/iteration)%s"
          % (epoch, m["loss_mean"], m["nll_mean"], m["accuracy"], m["nonfinite_steps"], m["skipped_steps"], dt,
             "  lambdal rate %.4g" % optimizer.param_groups[-1]["lr"] if DECAY else ""))
    if scheduler is not None:
        scheduler.step()
with torch.no_grad():
    print("mean inclusion probability per layer:", ["%.3f" % float(l.alpha.mean()) for l in ls])

# test_ensemble (:345-441) on a held-out synthetic batch: hard gates as the reference sets them before its test (:619-621), ten
# members drawn in one launch; then the median probability model of outofsample(medimod=True) (:469-473)
for l in ls:
    l.gamma.exact = True
test_x = torch.rand(1000, 1, 28, 28, device=DEVICE, generator=g)
test_y = (test_x.view(1000, 784) @ proj).argmax(-1)
res = bnn_amd.evaluate.ensemble_eval(net, test_x, test_y, samples=10)
print("held-out: ensemble accuracy %.3f, posterior-mean accuracy %.3f, density %.3f"
      % (res["correct_ensemble"] / 1000, res["correct_posterior_mean"] / 1000, float(res["density"].mean())))
mpm = bnn_amd.evaluate.ensemble_forward(net, test_x, 10, gates="mpm")
print("median probability model: accuracy %.3f, mean predictive entropy %.3f"
      % (float(mpm.mean(0).argmax(1).eq(test_y).float().mean()), float(bnn_amd.evaluate.predictive_entropy(mpm).mean())))

# A whole test pass with ONE host read: several held-out batches through an EvalAccumulator (per batch: base_ensemble, the
# posterior-mean forward and one lbbnn_eval_metrics call; the totals stay on the device until result()) -- the sampled gates,
# then the median probability model.
test_batches = []
for _ in range(5):
    bx = torch.rand(200, 1, 28, 28, device=DEVICE, generator=g)
    test_batches.append((bx, (bx.view(200, 784) @ proj).argmax(-1)))
for gates in ("sample", "mpm"):
    tot = bnn_amd.evaluate.evaluate_batches(net, test_batches, samples=10, gates=gates)
    print("test pass over %d rows, gates=%s (one host read): ensemble %.3f | posterior mean %.3f | members %.3f .. %.3f | nll %.3f "
          "| mean predictive entropy %.3f"
          % (tot["rows"], gates, tot["accuracy_ensemble"], tot["accuracy_posterior_mean"],
             tot["correct_member"].min() / tot["rows_with_target"], tot["correct_member"].max() / tot["rows_with_target"],
             tot["nll_mean"], tot["entropy_mean"]))

# The sparse network the method exists to produce: the median probability model frozen once, without the units no output depends
# on (evaluate.freeze_base(net, "mpm", compact=True)), and the same test pass as replays of ONE HIP graph per batch.
fz = bnn_amd.evaluate.freeze_base(net, "mpm", compact=True)
acc = bnn_amd.evaluate.EvalAccumulator(10, 10, DEVICE)
eval_step = bnn_amd.graphs.make_graphed_eval_step(fz, test_batches[0][0], test_batches[0][1], 10, acc)
for bx, by in test_batches:
    eval_step(bx, by)
tot = acc.result()
print("compact median probability model %s of %s: density %.3f, active density %.3f; graphed test pass over %d rows: ensemble "
      "%.3f | posterior mean %.3f | nll %.3f"
      % ("-".join(map(str, fz.dims)), "-".join(map(str, fz.full_dims)), fz.density, fz.active_density, tot["rows"],
         tot["accuracy_ensemble"], tot["accuracy_posterior_mean"], tot["nll_mean"]))
