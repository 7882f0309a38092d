#!/usr/bin/env python3
"""Local explanations of a latent-binary network: for THIS row, which covariates drove the output, and by how much?

The network and the data of examples/feature_selection_synthetic.py (20 standard-normal covariates, five of them in the true
support, y ~ Bernoulli(sigmoid(x . w)); 20 -> 16 -> 1, sigmoid head).  ``structure_posterior`` answers the global question --
which covariates lie on an active path at all.  The median probability model's posterior-mean forward is a ReLU chain on fixed
weights, so per row its logit is EXACTLY linear in the input,

    res = bnn_amd.evaluate.explain(bnn_amd.evaluate.freeze(net, "mpm"), x)
    res["contributions"][b, 0, i]      # J[b, 0, i] * x[b, i]: what covariate i added to the logit of row b
    res["intercept"][b, 0]             # the bias path;  logits = contributions.sum(-1) + intercept  (res["residual"] checks it)

and ``explain_batches`` / ``ExplanationAccumulator`` average |contribution| over a pass on the device: the global importance
that sits beside ``feature_prob``.

    python examples/explain_synthetic.py
    ROWS=2000 EPOCHS=1000 python examples/explain_synthetic.py
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
fz = bnn_amd.evaluate.freeze(net, "mpm")
batches = [x_all[b * BATCH_SIZE:(b + 1) * BATCH_SIZE] for b in range(NUM_BATCHES)]
imp = bnn_amd.evaluate.explain_batches(fz, batches).result()          # one host read for the whole pass
mean_abs, mean = imp["mean_abs_contribution"][0], imp["mean_contribution"][0]
print("median probability model: density %.4f; %d rows explained" % (fz.density, int(imp["rows"][0])))
print("covariate  in support  true w   P(on an active path)  mean |contribution|  mean contribution")
for i in range(FEATURES):
    print("%9d  %10s  %6.2f  %20.3f  %19.4f  %17.4f" % (i, "yes" if support[i] else "", float(w_true[i]), float(prob[i]), mean_abs[i], mean[i]))
inside, outside = mean_abs[support.numpy()], mean_abs[~support.numpy()]
print("lowest mean |contribution| inside the support %.4f, highest outside %.4f" % (inside.min(), outside.max()))

res = bnn_amd.evaluate.explain(fz, x_all[:2], keep_masks=True)
for b in range(2):
    c = res["contributions"][b, 0].cpu()
    order = torch.argsort(c.abs(), descending=True)[:6].tolist()
    print("row %d: logit %.4f = intercept %.4f + contributions %.4f (residual %.1e); %d of %d hidden units active"
          % (b, float(res["logits"][b, 0]), float(res["intercept"][b, 0]), float(c.sum()), float(res["residual"][b, 0]),
             int(res["active"][b, 0]), HIDDEN))
    print("        largest: " + "  ".join("x%d=%.2f -> %+.4f" % (i, float(x_all[b, i]), float(c[i])) for i in order))
    print("        the data's own terms w_i x_i there: " + "  ".join("%+.4f" % float(w_true[i] * x_all[b, i].cpu()) for i in order))
