#!/usr/bin/env python3
"""Where to prune: density, accuracy and NLL of the median probability model at EVERY inclusion threshold, from one freeze.

The network and the data of examples/explain_synthetic.py (20 standard-normal covariates, five of them in the true support,
y ~ Bernoulli(sigmoid(x . w)); 20 -> 16 -> 1, sigmoid head).  After training,

    sw = bnn_amd.evaluate.threshold_sweep(net, thresholds)            # every level's sparse model: one count, one pack
    res = bnn_amd.evaluate.sweep_batches(sw, batches, samples=10)     # one pass: K x S members a layer launch, common draws
    res["density"][j], res["results"][j]["accuracy_ensemble"], ...    # the curve
    fz = sw.model(j)                                                  # the chosen level, a SparseFrozenNetwork: no other freeze

    python examples/threshold_sweep_synthetic.py
    ROWS=2000 EPOCHS=1000 python examples/threshold_sweep_synthetic.py
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
MEMBERS = int(os.environ.get("MEMBERS", "10"))
LR = float(os.environ.get("LR", "0.01"))
PRIORS = Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=float(os.environ.get("ALPHA_PRIOR", "0.05")), bias_sigma_prior=1.3)
INIT = (1.5, 2.5)
THRESHOLDS = (0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)

g = torch.Generator().manual_seed(3)
w_true = torch.zeros(FEATURES)
w_true[[1, 4, 9, 12, 17]] = torch.tensor([2.0, -1.5, 1.0, -2.5, 1.5])
x_all = torch.randn(ROWS, FEATURES, generator=g)
y_all = (torch.rand(ROWS, generator=g) < torch.sigmoid(x_all @ w_true)).float().reshape(ROWS, 1)
x_test = torch.randn(ROWS // 5, FEATURES, generator=g)
y_test = (torch.rand(ROWS // 5, generator=g) < torch.sigmoid(x_test @ w_true)).float()
x_all, y_all, x_test, y_test = x_all.to(DEVICE), y_all.to(DEVICE), x_test.to(DEVICE), y_test.to(DEVICE)

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

sw = bnn_amd.evaluate.threshold_sweep(net, THRESHOLDS)
batches = [(x_test[i:i + BATCH_SIZE], y_test[i:i + BATCH_SIZE]) for i in range(0, x_test.shape[0], BATCH_SIZE)]
res = bnn_amd.evaluate.sweep_batches(sw, batches, MEMBERS)
density = res["density"].tolist()
print("%d test rows, %d members per level, the same draws at every level" % (x_test.shape[0], MEMBERS))
keys = ("accuracy_posterior_mean", "nll_mean", "accuracy_ensemble")
print("threshold   kept  density  " + "  ".join("%-23s" % k for k in keys))
for j, t in enumerate(res["thresholds"]):
    r = res["results"][j]
    print("%9.2f  %5d  %7.4f  " % (t, sw.nnz[j], density[j]) + "  ".join("%-23.4f" % r[k] for k in keys))
j = max(j for j in range(len(THRESHOLDS)) if sw.nnz[j] > 0)
fz = sw.model(j)
print("the sparsest level that keeps a weight, threshold %.2f, goes on as %r" % (THRESHOLDS[j], fz))
