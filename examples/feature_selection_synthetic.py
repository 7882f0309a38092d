#!/usr/bin/env python3
"""Feature selection with a DEEP latent-binary network: which covariates lie on an active path to the output?

The simulation study's data-generating process (examples/sim_study_synthetic.py: 20 standard-normal covariates, five of them in
the true support, y ~ Bernoulli(sigmoid(x . w))) on a 20 -> 16 -> 1 network with a sigmoid head.  With a hidden layer the first
layer's alpha no longer answers "does covariate j matter": a weight from j may be kept into a hidden unit that nothing reads.
The answer is a property of the sampled structure,

    res = bnn_amd.evaluate.structure_posterior(net, 1000)
    res["feature_prob"][j]    # P(covariate j lies on an active path to the output)
    res["active_density"]     # per sample: the share of weights on such paths

one kernel launch for the 1000 structures (lbbnn_gate_structure).  Training is the sim study's: the whole step -- forward, head,
fused BCE loss with the training monitor, backward, Adam behind the monitor's guard -- captured once in a HIP graph.  Run on an
LRT network and on an MNF network with this package's planar flows.

ROWS defaults to 50000: sixteen exchangeable hidden units share a covariate's effect, and with the study's 2000 rows the
mean-field posterior keeps every alpha near the prior -- the support then ranks first but is not separated.

    python examples/feature_selection_synthetic.py
    ROWS=2000 EPOCHS=1000 ALPHA_PRIOR=0.05 python examples/feature_selection_synthetic.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd import Priors, lrt, mnf

DEVICE = torch.device("cuda:0")
FEATURES, HIDDEN, BATCH_SIZE = 20, 16, 400
ROWS = int(os.environ.get("ROWS", "50000"))
NUM_BATCHES = ROWS // BATCH_SIZE
EPOCHS = int(os.environ.get("EPOCHS", "100"))
SAMPLES = int(os.environ.get("SAMPLES", "1000"))
LR = float(os.environ.get("LR", "0.01"))
# a sparse prior: a covariate reaches the output through any of 16 hidden units, so a weight the data do not ask for has to be
# rare for the covariate to be off every path
PRIORS = Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=float(os.environ.get("ALPHA_PRIOR", "0.05")), bias_sigma_prior=1.3)
INIT = (1.5, 2.5)                                    # lambdal ~ U(1.5, 2.5): every weight starts included (alpha ~ 0.88)

g = torch.Generator().manual_seed(3)
w_true = torch.zeros(FEATURES)
w_true[[1, 4, 9, 12, 17]] = torch.tensor([2.0, -1.5, 1.0, -2.5, 1.5])
x_all = torch.randn(ROWS, FEATURES, generator=g)
y_all = (torch.rand(ROWS, generator=g) < torch.sigmoid(x_all @ w_true)).float().reshape(ROWS, 1)
x_all, y_all = x_all.to(DEVICE), y_all.to(DEVICE)
support = w_true != 0


def run(name, net):
    net = net.to(DEVICE).train()
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
            print("%s epoch %3d  loss_mean %8.2f  nll_mean %.4f  accuracy %.3f  nonfinite_steps %d"
                  % (name, epoch + 1, m["loss_mean"], m["nll_mean"], m["accuracy"], m["nonfinite_steps"]))
    net.eval()
    res = bnn_amd.evaluate.structure_posterior(net, SAMPLES)
    prob = res["feature_prob"].cpu()
    print("%s P(covariate on an active path), S = %d: %s" % (name, SAMPLES, " ".join("%.2f" % p for p in prob.tolist())))
    chosen = prob > 0.5
    print("%s true support %s | P > 0.5 %s | lowest P inside the support %.3f, highest outside %.3f"
          % (name, support.nonzero().reshape(-1).tolist(), chosen.nonzero().reshape(-1).tolist(),
             float(prob[support].min()), float(prob[~support].max())))
    first = net.inclusion_probabilities()[0].cpu()
    print("%s for comparison, the largest first-layer alpha of each covariate: %s"
          % (name, " ".join("%.2f" % a for a in first.max(0).values.tolist())))
    ad, hidden = res["active_density"].cpu(), res["needed"][:, 1].double().cpu()
    q = torch.quantile(ad, torch.tensor([0.0, 0.05, 0.5, 0.95, 1.0], dtype=torch.float64))
    print("%s active-path density over the samples: min %.4f  5%% %.4f  median %.4f  95%% %.4f  max %.4f  (plain density: mean %.4f)"
          % ((name,) + tuple(q.tolist()) + (float(res["density"].mean()),)))
    print("%s hidden units needed: mean %.2f of %d (min %d, max %d); P(unit needed): %s"
          % (name, float(hidden.mean()), HIDDEN, int(hidden.min()), int(hidden.max()),
             " ".join("%.2f" % p for p in res["unit_prob"][0].cpu().tolist())))


torch.manual_seed(1)
run("LRT", lrt.BayesianNetwork((FEATURES, HIDDEN, 1), head="sigmoid", priors=PRIORS, lambdal_init=INIT))
torch.manual_seed(1)
run("MNF", mnf.BayesianNetwork((FEATURES, HIDDEN, 1), 2, z_flow_type="Planar", r_flow_type="Planar", head="sigmoid",
                               priors=PRIORS, lambdal_init=INIT))
