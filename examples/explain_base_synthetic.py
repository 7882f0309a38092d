#!/usr/bin/env python3
"""Local explanations of a baseline LBBNN network with uncertainty, on the simulation study's generating process: a baseline
``BayesianNetwork((20, 16, 1), head="sigmoid")`` trained as examples/sim_study_base_synthetic.py trains (BCE ELBO, in-kernel
draws, one-launch SGD with one group per tensor behind the monitor's guard, the whole step a HIP graph, the priors ``exact``
from the switch epoch on), then frozen as its SPARSE median probability model.  Two things differ from the one-layer study, both
because the first layer has 320 weights, not 20: the six prior groups' rates are 0 from the first step (the script sets them to 0
at its switch epoch) -- a prior's shared scalars collect the gradient of every weight of the layer, and at the study's rate 1e-3
``weight_b`` of the first layer turns negative within four epochs, after which every loss is NaN and the guard skips every
step -- and the other rates are the study's times RATE_SCALE (default 10): at the study's own rates the two layers' nll had
not left log 2 = 0.69 in the first epochs.

    fz = evaluate.freeze_base(net, "mpm", sparse=True)            # CSR of the weights with alpha > 0.5
    res = evaluate.evaluate_batches(fz, [(x, y)], samples=10)      # the members touch no pruned weight
    ex = evaluate.explain_ensemble(fz, x[:2], samples=200)         # J_m(b) * x of 200 members: mean, std, sign probability

The baseline member has explicit weights, so the members explained are the members the ensemble evaluates.  The script prints
what it gets -- density, nnz, ensemble accuracy, and for two rows every covariate's contribution (mean +- std over the members,
the share of members with a positive one) beside the covariate's largest first-layer inclusion probability and the true
support; no number is required of it.

    python examples/explain_base_synthetic.py
    EPOCHS=500 SWITCH=50 RATE_SCALE=5 python examples/explain_base_synthetic.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd import base, evaluate

DEVICE = torch.device("cuda:0")
FEATURES, HIDDEN, ROWS, BATCH_SIZE = 20, 16, 2000, 400
NUM_BATCHES = ROWS // BATCH_SIZE
EPOCHS = int(os.environ.get("EPOCHS", "200"))
SWITCH = int(os.environ.get("SWITCH", "50"))
RATE_SCALE = float(os.environ.get("RATE_SCALE", "10"))
MEMBERS = 200

g = torch.Generator().manual_seed(3)
w_true = torch.zeros(FEATURES)
w_true[[1, 4, 9, 12, 17]] = torch.tensor([2.0, -1.5, 1.0, -2.5, 1.5])
x_all = torch.randn(ROWS, FEATURES, generator=g)
y_all = (torch.rand(ROWS, generator=g) < torch.sigmoid(x_all @ w_true)).float()
x_all, y_all = x_all.to(DEVICE), y_all.to(DEVICE)
support = w_true != 0

torch.manual_seed(0)
net = base.BayesianNetwork((FEATURES, HIDDEN, 1), head="sigmoid", weight_mu_init=(-0.2, 0.2), lambdal_init=(-0.5, 0.5)).to(DEVICE).train()
layers = net._layers()
# the script's eleven groups (LBBNN-GP-MFsim_study.py:359-374), per layer; the six prior groups at rate 0 throughout
RATES = [("bias_mu", 1e-4), ("bias_rho", 1e-4), ("weight_mu", 1e-4), ("weight_rho", 1e-4), ("pa", 0.0), ("pb", 0.0),
         ("weight_a", 0.0), ("weight_b", 0.0), ("bias_a", 0.0), ("bias_b", 0.0), ("lambdal", 1e-3)]
groups = [{"params": getattr(l, n), "lr": r * RATE_SCALE} for l in layers for n, r in RATES]
optimizer = bnn_amd.optim.SGD(groups, lr=0.01)
monitor = bnn_amd.TrainMonitor(1, DEVICE)
optimizer.set_guard(monitor)


def elbo(net, data, target):
    return net.sample_elbo(data, target, num_batches=NUM_BATCHES, draws="hip", monitor=monitor)[0]


def capture():
    return bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, x_all[:BATCH_SIZE], y_all[:BATCH_SIZE])


step = capture()
for epoch in range(EPOCHS):
    if epoch == SWITCH:                                              # :377-408, as examples/sim_study_base_synthetic.py
        for l in layers:
            l.gamma_prior.exact = l.bias_prior.exact = l.weight_prior.exact = True
        bnn_amd.graphs.release_module_graph_refs(net)
        del step
        step = capture()
    monitor.reset()
    for b in range(NUM_BATCHES):
        rows = slice(b * BATCH_SIZE, (b + 1) * BATCH_SIZE)
        step(x_all[rows], y_all[rows])
    if epoch % 50 == 49 or epoch == EPOCHS - 1:
        m = monitor.result()                                         # the epoch's one host read
        print("epoch %3d  loss_mean %9.2f  nll_mean %.4f  accuracy %.3f  skipped_steps %d"
              % (epoch + 1, m["loss_mean"], m["nll_mean"], m["accuracy"], m["skipped_steps"]))

net.eval()
fz = evaluate.freeze_base(net, "mpm", sparse=True)
print(fz)
print("density %.4f, nnz %d of %d weights (per layer %s), %d bytes of operands"
      % (fz.density, fz.nnz, FEATURES * HIDDEN + HIDDEN, fz.kept, fz.operand_bytes))
res = evaluate.evaluate_batches(fz, [(x_all, y_all)], samples=10)
print("sparse median probability model: ensemble accuracy %.3f on the training rows" % res["accuracy_ensemble"])

ex = evaluate.explain_ensemble(fz, x_all[:2], samples=MEMBERS)
alpha = net.inclusion_probabilities()[0].detach().cpu()              # (HIDDEN, FEATURES)
top = alpha.max(0).values
mean, std, pos = (ex[k][:, 0].cpu() for k in ("mean", "std", "prob_positive"))
print("contributions J_m(b) * x of %d members to the logit; |residual| <= %.1e" % (MEMBERS, float(ex["residual"].abs().max())))
print("covariate  support  max alpha   row 0: x  mean +- std  P(> 0)      row 1: x  mean +- std  P(> 0)")
for i in range(FEATURES):
    cells = "      ".join("%6.2f  %7.3f +- %.3f  %.2f" % (float(x_all[b, i]), float(mean[b, i]), float(std[b, i]), float(pos[b, i]))
                          for b in range(2))
    print("%9d  %7s  %9.2f   %s" % (i, "yes" if bool(support[i]) else "", float(top[i]), cells))
