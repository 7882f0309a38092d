#!/usr/bin/env python3
"""Regression with latent binary weights: a network 8 -> 32 -> 1 with an identity head, a normal likelihood whose log-variance is
learned, and the fused Gaussian ELBO loss.

    net = lrt.BayesianNetwork((8, 32, 1), head="identity")
    log_var = torch.nn.Parameter(torch.zeros(1, device=DEVICE))            # its own Adam group
    monitor = bnn_amd.TrainMonitor(1, DEVICE); optimizer.set_guard(monitor)
    loss = bnn_amd.elbo_gaussian_loss(net(x, sample=True), y, log_var, net.kl(), NUM_BATCHES, stats=stats, monitor=monitor)

The data are synthetic and made here: 2000 rows of 8 standard-normal covariates, y = sin(x0) + 0.5 x1 x2 - x3 + 0.3 * noise (the
last four covariates do nothing).  The whole step -- forward, fused loss with the training monitor, backward, Adam behind the
monitor's guard -- is captured once in a HIP graph; the epoch's mean loss, the one-sigma coverage (the monitor's ``accuracy``) and
the training RMSE (from ``stats``) are read once per epoch.  At the end the network is frozen twice -- the gates as trained, and
the median probability model -- and a graphed evaluation pass over held-out rows prints rmse, mean log density, coverage and the
PIT histogram of each from a ``RegressionAccumulator`` that reads the learned ``log_var`` through its pointer.  Run on an LRT
network and on an MNF network with this package's planar flows.

    python examples/train_regression_synthetic.py
    EPOCHS=400 python examples/train_regression_synthetic.py
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd import Priors, evaluate, lrt, mnf

DEVICE = torch.device("cuda:0")
DIMS, ROWS, TEST_ROWS, BATCH_SIZE, SAMPLES = (8, 32, 1), 2000, 1000, 400, 10
NUM_BATCHES = ROWS // BATCH_SIZE
EPOCHS = int(os.environ.get("EPOCHS", "200"))
NOISE_SD = 0.3
PRIORS = Priors(mu_prior=0.0, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
INIT = (1.5, 2.5)                                    # lambdal ~ U(1.5, 2.5): every weight starts included (alpha ~ 0.88)

g = torch.Generator().manual_seed(3)


def f(x):
    return torch.sin(x[:, 0]) + 0.5 * x[:, 1] * x[:, 2] - x[:, 3]


x_all = torch.randn(ROWS + TEST_ROWS, DIMS[0], generator=g)
y_all = (f(x_all) + NOISE_SD * torch.randn(ROWS + TEST_ROWS, generator=g)).reshape(-1, 1)
x_all, y_all = x_all.to(DEVICE), y_all.to(DEVICE)
x_test, y_test = x_all[ROWS:], y_all[ROWS:]


def run(name, net):
    net = net.to(DEVICE).train()
    log_var = torch.nn.Parameter(torch.zeros(1, device=DEVICE))
    optimizer = bnn_amd.optim.Adam([{"params": list(net.parameters())}, {"params": [log_var], "lr": 0.05}], lr=0.01)
    monitor = bnn_amd.TrainMonitor(1, DEVICE)                        # one output unit; the totals count elements (b, o)
    optimizer.set_guard(monitor)
    stats = torch.zeros(4, dtype=torch.float64, device=DEVICE)      # squared error, absolute error, valid targets, bad targets

    def elbo(net, data, target):
        return bnn_amd.elbo_gaussian_loss(net(data, sample=True), target, log_var, net.kl(), NUM_BATCHES, stats=stats,
                                          monitor=monitor)

    step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, x_all[:BATCH_SIZE], y_all[:BATCH_SIZE])
    for epoch in range(EPOCHS):
        monitor.reset()                                              # (also drops the warm-up steps of the step's factory)
        stats.zero_()
        for b in range(NUM_BATCHES):
            rows = slice(b * BATCH_SIZE, (b + 1) * BATCH_SIZE)
            step(x_all[rows], y_all[rows])
        if epoch % 50 == 49 or epoch == EPOCHS - 1:
            m, s = monitor.result(), stats.tolist()                  # the epoch's two host reads
            print("%s epoch %3d  loss_mean %9.2f  nll_mean %7.4f  one-sigma coverage %.3f  rmse %.4f  mae %.4f  noise sd %.3f  "
                  "nonfinite_steps %d  skipped_steps %d"
                  % (name, epoch + 1, m["loss_mean"], m["nll_mean"], m["accuracy"], math.sqrt(s[0] / s[2]), s[1] / s[2],
                     math.exp(0.5 * float(log_var.detach())), m["nonfinite_steps"], m["skipped_steps"]))
            assert m["nonfinite_rows"] == 0 and s[3] == 0
    # ---- evaluation on the held-out rows: the frozen model with the gates as trained, then the median probability model; one
    # graphed step per batch, one read of the totals at the end of each pass
    net.eval()
    eb = 500
    for gates, what in (("alpha", "gates as trained"), ("mpm", "median probability model")):
        fz = evaluate.freeze(net, gates=gates)
        acc = evaluate.RegressionAccumulator(DIMS[-1], SAMPLES, DEVICE, log_var)
        eval_step = bnn_amd.graphs.make_graphed_eval_step(fz, x_test[:eb], y_test[:eb], SAMPLES, acc)
        for b in range(TEST_ROWS // eb):
            eval_step(x_test[b * eb:(b + 1) * eb], y_test[b * eb:(b + 1) * eb])
        r = acc.result()
        print("%s %s: density %.3f; held-out rmse %.4f (posterior mean %.4f, noise sd %.1f)  mae %.4f  r2 %.3f  mean log density "
              "%.4f" % (name, what, fz.density, r["rmse"], r["rmse_posterior_mean"], NOISE_SD, r["mae"], r["r2"],
                        r["mean_log_density"]))
        print("%s %s: predictive variance epistemic %.4f of total %.4f; coverage of the central 50 / 80 / 90 %% intervals: %.3f "
              "%.3f %.3f" % (name, what, r["mean_epistemic_var"], r["mean_total_var"], r["coverage"](0.5), r["coverage"](0.8),
                             r["coverage"](0.9)))
        print("%s %s: PIT histogram (%d bins, %d elements): %s"
              % (name, what, acc.pit_bins, r["scored_elements"], r["pit_hist"].tolist()))


torch.manual_seed(1)
run("LRT", lrt.BayesianNetwork(DIMS, head="identity", priors=PRIORS, lambdal_init=INIT))
torch.manual_seed(1)
run("MNF", mnf.BayesianNetwork(DIMS, 2, z_flow_type="Planar", r_flow_type="Planar", head="identity", priors=PRIORS,
                               lambdal_init=INIT))
