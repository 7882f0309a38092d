#!/usr/bin/env python3
"""Variable selection in a logistic regression with latent binary weights -- the shape of the simulation study of the
latent-binary papers: ONE Bayesian layer 20 -> 1, a sigmoid on its output, BCELoss(sum) + kl / NUM_BATCHES, and the posterior
inclusion probabilities alpha = sigmoid(lambdal) as the result.

    net = lrt.BayesianNetwork((20, 1), head="sigmoid", priors=..., lambdal_init=(1.5, 2.5))
    monitor = bnn_amd.TrainMonitor(1, DEVICE); optimizer.set_guard(monitor)
    loss = bnn_amd.elbo_bce_loss(net(x, sample=True), y, net.kl(), NUM_BATCHES, monitor=monitor)

The data are synthetic and made here: 2000 rows of 20 standard-normal covariates, a sparse weight vector of this script's own
(five non-zero entries), y ~ Bernoulli(sigmoid(x . w)).  The whole step -- forward, head, fused loss with the training monitor, backward,
Adam behind the monitor's guard -- is captured once in a HIP graph; the epoch's mean loss, mean nll and training accuracy come
from the monitor's device-side totals, read once per epoch, and a step whose loss is not finite changes no parameter and is counted.  Run on an LRT network and on an MNF network with this package's planar flows.

    python examples/sim_study_synthetic.py
    EPOCHS=600 python examples/sim_study_synthetic.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd import Priors, lrt, mnf

DEVICE = torch.device("cuda:0")
FEATURES, ROWS, BATCH_SIZE = 20, 2000, 400
NUM_BATCHES = ROWS // BATCH_SIZE
EPOCHS = int(os.environ.get("EPOCHS", "300"))
PRIORS = Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
INIT = (1.5, 2.5)                                    # lambdal ~ U(1.5, 2.5): every covariate starts included (alpha ~ 0.88)

g = torch.Generator().manual_seed(3)
w_true = torch.zeros(FEATURES)
w_true[[1, 4, 9, 12, 17]] = torch.tensor([2.0, -1.5, 1.0, -2.5, 1.5])
x_all = torch.randn(ROWS, FEATURES, generator=g)
y_all = (torch.rand(ROWS, generator=g) < torch.sigmoid(x_all @ w_true)).float().reshape(ROWS, 1)
x_all, y_all = x_all.to(DEVICE), y_all.to(DEVICE)
support = w_true != 0


def run(name, net):
    net = net.to(DEVICE).train()
    optimizer = bnn_amd.optim.Adam(net.parameters(), lr=0.01)
    monitor = bnn_amd.TrainMonitor(1, DEVICE)                        # one output unit; the totals count elements (b, o)
    optimizer.set_guard(monitor)

    def elbo(net, data, target):
        return bnn_amd.elbo_bce_loss(net(data, sample=True), target, net.kl(), NUM_BATCHES, monitor=monitor)

    step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, x_all[:BATCH_SIZE], y_all[:BATCH_SIZE])
    for epoch in range(EPOCHS):
        monitor.reset()                                              # (also drops the warm-up steps of the step's factory)
        for b in range(NUM_BATCHES):
            rows = slice(b * BATCH_SIZE, (b + 1) * BATCH_SIZE)
            loss = step(x_all[rows], y_all[rows])
        if epoch % 50 == 49 or epoch == EPOCHS - 1:
            m = monitor.result()                                         # the epoch's one host read
            print("%s epoch %3d  loss_mean %8.2f  nll_mean %.4f  accuracy %.3f (%d rows)  nonfinite_steps %d  skipped_steps %d"
                  % (name, epoch + 1, m["loss_mean"], m["nll_mean"], m["accuracy"], m["rows"], m["nonfinite_steps"],
                     m["skipped_steps"]))
            assert m["nonfinite_rows"] == 0
    alpha = net.inclusion_probabilities()[0].reshape(-1).cpu()
    chosen = alpha > 0.5
    print("%s inclusion probabilities: %s" % (name, " ".join("%.2f" % a for a in alpha.tolist())))
    print("%s true support %s | selected %s | agreement %d / %d covariates"
          % (name, support.nonzero().reshape(-1).tolist(), chosen.nonzero().reshape(-1).tolist(),
             int((chosen == support).sum()), FEATURES))
    mpm = bnn_amd.evaluate.freeze(net, gates="mpm")
    res = bnn_amd.evaluate.evaluate_batches(mpm, [(x_all, y_all)], samples=10)
    print("%s median probability model: %d of %d weights kept, ensemble accuracy %.3f on the training rows"
          % (name, mpm.kept[0], FEATURES, res["accuracy_ensemble"]))


torch.manual_seed(1)
run("LRT", lrt.BayesianNetwork((FEATURES, 1), head="sigmoid", priors=PRIORS, lambdal_init=INIT))
torch.manual_seed(1)
run("MNF", mnf.BayesianNetwork((FEATURES, 1), 2, z_flow_type="Planar", r_flow_type="Planar", head="sigmoid", priors=PRIORS,
                               lambdal_init=INIT))
