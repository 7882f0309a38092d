#!/usr/bin/env python3
"""The baseline network's simulation study (LBBNN-GP-MFsim_study.py) on synthetic data: ONE baseline ``BayesianLinear`` 20 -> 1
with explicit latent binary gates, a sigmoid on its output, BCELoss(sum) + (log_q - log_prior) / NUM_BATCHES, ``optim.SGD`` with
eleven single-tensor groups at two rates, and the posterior inclusion probabilities alpha = sigmoid(lambdal) as the result.

    net = base.BayesianNetwork((20, 1), head="sigmoid", weight_mu_init=(-0.01, 0.01), lambdal_init=(-0.5, 0.5))
    monitor = bnn_amd.TrainMonitor(1, DEVICE); optimizer.set_guard(monitor)
    loss, log_prior, log_q, nll, out = net.sample_elbo(x, y, num_batches=NUM_BATCHES, draws="hip", monitor=monitor)

The data are made here: 2000 rows of 20 standard-normal covariates, a sparse weight vector of this script's own, y ~
Bernoulli(sigmoid(x . w)).  The whole step -- in-kernel draws, forward, head, the whole ELBO as one fused loss launch with the
training monitor, backward, the one-launch SGD behind the monitor's guard -- is captured in a HIP graph.  At the switch epoch (the script's epoch 50) the three priors go ``exact`` and the six prior
groups' rates go to 0; the epoch's mean loss, mean nll and training accuracy come from the monitor's device-side totals, read once per epoch, and
a step whose loss is not finite (the prior parameters are trainable and unchecked: base.VALIDATE_ARGS) changes no parameter.

    python examples/sim_study_base_synthetic.py
    EPOCHS=500 SWITCH=50 python examples/sim_study_base_synthetic.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd import base

DEVICE = torch.device("cuda:0")
FEATURES, ROWS, BATCH_SIZE = 20, 2000, 400
NUM_BATCHES = ROWS // BATCH_SIZE
EPOCHS = int(os.environ.get("EPOCHS", "200"))
SWITCH = int(os.environ.get("SWITCH", "50"))

g = torch.Generator().manual_seed(3)
w_true = torch.zeros(FEATURES)
w_true[[1, 4, 9, 12, 17]] = torch.tensor([2.0, -1.5, 1.0, -2.5, 1.5])
x_all = torch.randn(ROWS, FEATURES, generator=g)
y_all = (torch.rand(ROWS, generator=g) < torch.sigmoid(x_all @ w_true)).float()
x_all, y_all = x_all.to(DEVICE), y_all.to(DEVICE)
support = w_true != 0

torch.manual_seed(0)
net = base.BayesianNetwork((FEATURES, 1), head="sigmoid", weight_mu_init=(-0.01, 0.01), lambdal_init=(-0.5, 0.5)).to(DEVICE).train()
l1 = net.l1
# the script's eleven groups and rates (LBBNN-GP-MFsim_study.py:359-374)
RATES = [("bias_mu", 1e-4), ("bias_rho", 1e-4), ("weight_mu", 1e-4), ("weight_rho", 1e-4), ("pa", 1e-3), ("pb", 1e-3),
         ("weight_a", 1e-3), ("weight_b", 1e-3), ("bias_a", 1e-3), ("bias_b", 1e-3), ("lambdal", 1e-3)]
PRIOR_GROUPS = range(4, 10)                                          # pa, pb, weight_a, weight_b, bias_a, bias_b
optimizer = bnn_amd.optim.SGD([{"params": getattr(l1, n), "lr": r} for n, r in RATES], lr=0.01)
monitor = bnn_amd.TrainMonitor(1, DEVICE)                            # one output unit; the totals count elements (b, o)
optimizer.set_guard(monitor)


def elbo(net, data, target):
    return net.sample_elbo(data, target, num_batches=NUM_BATCHES, draws="hip", monitor=monitor)[0]


def capture():
    return bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, x_all[:BATCH_SIZE], y_all[:BATCH_SIZE])


step = capture()
for epoch in range(EPOCHS):
    if epoch == SWITCH:                                              # :377-408
        # The rates are rows of the optimizer's device table, read when the kernel runs: setting six of them to 0 needs no
        # re-capture (a graphed step pushes the table before its next replay).  The priors' ``exact`` bits are kernel ARGUMENTS of
        # the gate kernels (GateArgs.exact), fixed when the graph was captured: switching them takes ONE re-capture.  Its three
        # eager warm-up steps are training steps like any other, so the rates go to 0 first, as in the script.
        for i in PRIOR_GROUPS:
            optimizer.param_groups[i]["lr"] = 0.0
        frozen = [optimizer.param_groups[i]["params"][0].detach().clone() for i in PRIOR_GROUPS]
        l1.gamma_prior.exact = l1.bias_prior.exact = l1.weight_prior.exact = True
        bnn_amd.graphs.release_module_graph_refs(net)
        del step
        step = capture()
    monitor.reset()                                                  # (also drops the warm-up steps of a capture)
    for b in range(NUM_BATCHES):
        rows = slice(b * BATCH_SIZE, (b + 1) * BATCH_SIZE)
        loss = step(x_all[rows], y_all[rows])
    if epoch % 25 == 24 or epoch == EPOCHS - 1:
        m = monitor.result()                                         # the epoch's one host read
        print("epoch %3d  loss_mean %9.2f  nll_mean %.4f  accuracy %.3f (%d rows)  nonfinite_steps %d  skipped_steps %d"
              % (epoch + 1, m["loss_mean"], m["nll_mean"], m["accuracy"], m["rows"], m["nonfinite_steps"], m["skipped_steps"]))
        assert m["nonfinite_rows"] == 0
if EPOCHS > SWITCH:
    assert all(torch.equal(optimizer.param_groups[i]["params"][0].detach(), f) for i, f in zip(PRIOR_GROUPS, frozen))
    print("the six prior parameters are bitwise what they were at the switch (rate 0 through the device table)")
alpha = net.inclusion_probabilities()[0].reshape(-1).cpu()
chosen = alpha > 0.5
print("inclusion probabilities: %s" % " ".join("%.2f" % a for a in alpha.tolist()))
print("true support %s | selected %s | agreement %d / %d covariates"
      % (support.nonzero().reshape(-1).tolist(), chosen.nonzero().reshape(-1).tolist(), int((chosen == support).sum()), FEATURES))
res = bnn_amd.evaluate.evaluate_batches(net, [(x_all, y_all)], samples=10, gates="mpm")
print("median probability model: ensemble accuracy %.3f on the training rows" % res["accuracy_ensemble"])
