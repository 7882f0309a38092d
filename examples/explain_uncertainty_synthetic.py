#!/usr/bin/env python3
"""Local explanations WITH uncertainty: how sure is the posterior that covariate i pushed THIS row's output up?

The network and the data of examples/explain_synthetic.py (20 standard-normal covariates, five of them in the true support,
y ~ Bernoulli(sigmoid(x . w)); 20 -> 16 -> 1, sigmoid head).  ``explain`` gives one explanation per row: that of the
posterior-mean forward.  The sparse median probability model keeps only the weights with inclusion probability above the
threshold, so S members' explicit weights (w = mu + sigma * eps on the kept pattern) are a few small vectors; each member is an
ordinary ReLU network whose logit is EXACTLY linear in the input, and

    fz = bnn_amd.evaluate.freeze(net, "mpm", sparse=True)
    res = bnn_amd.evaluate.explain_ensemble(fz, x, samples=200, levels=(0.9,))
    res["mean"][b, 0, i], res["std"][b, 0, i]      # J_m[b, 0, i] * x[b, i] over the members m
    res["prob_positive"][b, 0, i]                  # the share of members in which covariate i pushed the logit of row b up
    res["lower"][0][b, 0, i], res["upper"][0][b, 0, i]   # the central 90 % interval

    python examples/explain_uncertainty_synthetic.py
    ROWS=2000 EPOCHS=1000 python examples/explain_uncertainty_synthetic.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd import Priors, lrt

DEVICE = torch.device("cuda:0")
FEATURES, HIDDEN, BATCH_SIZE = 20, 16, 400
ROWS = int(os.environ.get("ROWS", "50000"))
NUM_BATCHES = ROWS // BATCH_SIZE
EPOCHS = int(os.environ.get("EPOCHS", "100"))
SAMPLES = int(os.environ.get("SAMPLES", "1000"))
MEMBERS = int(os.environ.get("MEMBERS", "200"))
LR = float(os.environ.get("LR", "0.01"))
PRIORS = Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=float(os.environ.get("ALPHA_PRIOR", "0.05")), bias_sigma_prior=1.3)
INIT = (1.5, 2.5)

g = torch.Generator().manual_seed(3)
w_true = torch.zeros(FEATURES)
w_true[[1, 4, 9, 12, 17]] = torch.tensor([2.0, -1.5, 1.0, -2.5, 1.5])
x_all = torch.randn(ROWS, FEATURES, generator=g)
y_all = (torch.rand(ROWS, generator=g) < torch.sigmoid(x_all @ w_true)).float().reshape(ROWS, 1)
x_all, y_all = x_all.to(DEVICE), y_all.to(DEVICE)
support = w_true != 0

torch.manual_seed(1)
net = lrt.BayesianNetwork((FEATURES, HIDDEN, 1), head="sigmoid", priors=PRIORS, lambdal_init=INIT).to(DEVICE).train()
optimizer = bnn_amd.optim.Adam(net.parameters(), lr=LR)
monitor = bnn_amd.TrainMonitor(1, DEVICE)
optimizer.set_guard(monitor)


def elbo(net, data, target):
    return bnn_amd.elbo_bce_loss(net(data, sample=True), target, net.kl(), NUM_BATCHES, monitor=monitor)


step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, x_all[:BATCH_SIZE], y_all[:BATCH_SIZE])
for epoch in range(EPOCHS):
    monitor.reset()
    for b in range(NUM_BATCHES):
        rows = slice(b * BATCH_SIZE, (b + 1) * BATCH_SIZE)
        step(x_all[rows], y_all[rows])
    if epoch % 25 == 24 or epoch == EPOCHS - 1:
        m = monitor.result()
        print("epoch %3d  loss_mean %8.2f  nll_mean %.4f  accuracy %.3f" % (epoch + 1, m["loss_mean"], m["nll_mean"], m["accuracy"]))
net.eval()

prob = bnn_amd.evaluate.structure_posterior(net, SAMPLES)["feature_prob"].cpu()
fz = bnn_amd.evaluate.freeze(net, "mpm", sparse=True)
print("sparse median probability model: %d kept weights (density %.4f); %d members" % (fz.nnz, fz.density, MEMBERS))
res = bnn_amd.evaluate.explain_ensemble(fz, x_all[:2], MEMBERS, levels=(0.9,))
point = bnn_amd.evaluate.explain_ensemble(fz, x_all[:2], 1, weight_noise=False)       # the mean network: explain's counterpart
for b in range(2):
    lg = res["logits"][:, b, 0]
    print("row %d: member logits %.4f +- %.4f (mean network %.4f); largest |residual| %.1e"
          % (b, float(lg.mean()), float(lg.std()), float(point["logits"][0, b, 0]), float(res["residual"][:, b, 0].abs().max())))
    print("covariate  in support  true w   P(on an active path)       x   contribution: mean +- std   [90 % interval]   P(> 0)  mean network")
    for i in range(FEATURES):
        print("%9d  %10s  %6.2f  %20.3f  %6.2f  %12.4f +- %-8.4f  [%8.4f, %8.4f]  %6.3f  %12.4f"
              % (i, "yes" if support[i] else "", float(w_true[i]), float(prob[i]), float(x_all[b, i]), float(res["mean"][b, 0, i]),
                 float(res["std"][b, 0, i]), float(res["lower"][0][b, 0, i]), float(res["upper"][0][b, 0, i]),
                 float(res["prob_positive"][b, 0, i]), float(point["mean"][b, 0, i])))
