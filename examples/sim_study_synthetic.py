#!/usr/bin/env python3
"""Variable selection in a logistic regression with latent binary weights -- the shape of the simulation study of the
latent-binary papers: ONE Bayesian layer 20 -> 1, a sigmoid on its output, BCELoss(sum) + kl / NUM_BATCHES, and the posterior
inclusion probabilities alpha = sigmoid(lambdal) as the result.

    net = lrt.BayesianNetwork((20, 1), head="sigmoid", priors=..., lambdal_init=(1.5, 2.5))
    loss = bnn_amd.elbo_bce_loss(net(x, sample=True), y, net.kl(), NUM_BATCHES, stats=stats)

The data are synthetic and made here: 2000 rows of 20 standard-normal covariates, a sparse weight vector of this script's own
(five non-zero entries), y ~ Bernoulli(sigmoid(x . w)).  The whole step -- forward, head, fused loss with its counts, backward,
Adam -- is captured once in a HIP graph; the training accuracy of an epoch comes from the device-side counts, read once per
epoch.  Run on an LRT network and on an MNF network with this package's planar flows.

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
    stats = torch.zeros(4, dtype=torch.int32, device=DEVICE)         # correct, elements, bad targets, non-finite probabilities

    def elbo(net, data, target):
        return bnn_amd.elbo_bce_loss(net(data, sample=True), target, net.kl(), NUM_BATCHES, stats=stats)

    step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, x_all[:BATCH_SIZE], y_all[:BATCH_SIZE])
    for epoch in range(EPOCHS):
        stats.zero_()
        for b in range(NUM_BATCHES):
            rows = slice(b * BATCH_SIZE, (b + 1) * BATCH_SIZE)
            loss = step(x_all[rows], y_all[rows])
        if epoch % 50 == 49 or epoch == EPOCHS - 1:
            correct, elements, bad, nonfinite = stats.tolist()           # the epoch's one host read
            print("%s epoch %3d  loss %8.2f  training accuracy %.3f (%d rows)" % (name, epoch + 1, float(loss.detach()), correct / elements, elements))
            assert bad == 0 and nonfinite == 0
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
