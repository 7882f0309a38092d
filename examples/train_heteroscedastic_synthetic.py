#!/usr/bin/env python3
"""Heteroscedastic regression with latent binary weights: a network 8 -> 32 -> 2 with an identity head whose second output is the
log-variance of a normal likelihood, trained with the fused Gaussian ELBO loss and scored on the device.

    net = lrt.BayesianNetwork((8, 32, 2), head="identity")
    out = net(x, sample=True)
    loss = bnn_amd.elbo_gaussian_loss(out[:, :1], y, out[:, 1:], net.kl(), NUM_BATCHES, stats=stats)
    acc = evaluate.RegressionScoreAccumulator(1, SAMPLES, DEVICE, "output")        # log-variances: the outputs' upper column

The data are synthetic and made here: 8 standard-normal covariates, y = sin(x0) + 0.5 x1 x2 - x3 + sd(x) * noise with
sd(x) = 0.1 + 0.6 sigmoid(3 x4): the noise level depends on a covariate the mean does not use.  The training step -- forward,
fused loss, backward, Adam -- is one HIP graph.  The trained network is frozen twice (the gates as trained, and the median
probability model) and a second graph -- the ensemble, the posterior-mean forward and lbbnn_eval_regression_scores -- runs over
held-out rows; one read of the totals at the end of each pass prints rmse, mean log density, CRPS and the coverage and mean width of the central 50 % and 90 % intervals.  Next to
each stands a homoscedastic twin: 8 -> 32 -> 1 with one learned log-variance, scored by the same accumulator.  The twin's
intervals have one width everywhere; the heteroscedastic network's follow sd(x), which shows as a better log density and CRPS at
about the same rmse.  ``predict_regression`` then prints the 90 % interval at a quiet and at a noisy input.

    python examples/train_heteroscedastic_synthetic.py
    EPOCHS=400 python examples/train_heteroscedastic_synthetic.py
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd import Priors, evaluate, lrt, mnf

DEVICE = torch.device("cuda:0")
ROWS, TEST_ROWS, BATCH_SIZE, SAMPLES = 2000, 1000, 400, 10
NUM_BATCHES = ROWS // BATCH_SIZE
EPOCHS = int(os.environ.get("EPOCHS", "200"))
LEVELS = (0.5, 0.9)
PRIORS = Priors(mu_prior=0.0, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
INIT = (1.5, 2.5)                                    # lambdal ~ U(1.5, 2.5): every weight starts included (alpha ~ 0.88)

g = torch.Generator().manual_seed(3)


def f(x):
    return torch.sin(x[:, 0]) + 0.5 * x[:, 1] * x[:, 2] - x[:, 3]


def noise_sd(x):
    return 0.1 + 0.6 * torch.sigmoid(3.0 * x[:, 4])


x_all = torch.randn(ROWS + TEST_ROWS, 8, generator=g)
y_all = (f(x_all) + noise_sd(x_all) * torch.randn(ROWS + TEST_ROWS, generator=g)).reshape(-1, 1)
x_all, y_all = x_all.to(DEVICE), y_all.to(DEVICE)
x_test, y_test = x_all[ROWS:], y_all[ROWS:]


def run(name, net, heteroscedastic):
    net = net.to(DEVICE).train()
    groups = [{"params": list(net.parameters())}]
    log_var = None
    if not heteroscedastic:
        log_var = torch.nn.Parameter(torch.zeros(1, device=DEVICE))
        groups.append({"params": [log_var], "lr": 0.05})
    optimizer = bnn_amd.optim.Adam(groups, lr=0.01)
    stats = torch.zeros(4, dtype=torch.float64, device=DEVICE)      # squared error, absolute error, valid targets, bad targets

    def elbo(net, data, target):
        out = net(data, sample=True)
        if heteroscedastic:                                          # column 0: the mean; column 1: its log-variance, per row
            return bnn_amd.elbo_gaussian_loss(out[:, :1], target, out[:, 1:], net.kl(), NUM_BATCHES, stats=stats)
        return bnn_amd.elbo_gaussian_loss(out, target, log_var, net.kl(), NUM_BATCHES, stats=stats)

    step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, x_all[:BATCH_SIZE], y_all[:BATCH_SIZE])
    for epoch in range(EPOCHS):
        stats.zero_()
        total = torch.zeros((), device=DEVICE)
        for b in range(NUM_BATCHES):
            rows = slice(b * BATCH_SIZE, (b + 1) * BATCH_SIZE)
            total += step(x_all[rows], y_all[rows]).detach()
        if epoch % 50 == 49 or epoch == EPOCHS - 1:
            s = stats.tolist()                                       # the epoch's host read
            print("%s epoch %3d  loss_mean %9.2f  rmse %.4f  mae %.4f" % (name, epoch + 1, float(total) / NUM_BATCHES,
                                                                          math.sqrt(s[0] / s[2]), s[1] / s[2]))
    # ---- evaluation on the held-out rows: the frozen median probability model, one graphed step per batch, one read at the end
    net.eval()
    eb = 500
    noise = "output" if heteroscedastic else log_var
    models = {}
    for gates, what in (("alpha", "gates as trained"), ("mpm", "median probability model")):
        fz = models[gates] = evaluate.freeze(net, gates=gates)
        acc = evaluate.RegressionScoreAccumulator(1, SAMPLES, DEVICE, noise, levels=LEVELS)
        eval_step = bnn_amd.graphs.make_graphed_eval_step(fz, x_test[:eb], y_test[:eb], SAMPLES, acc)
        for b in range(TEST_ROWS // eb):
            eval_step(x_test[b * eb:(b + 1) * eb], y_test[b * eb:(b + 1) * eb])
        r = acc.result()
        i50, i90 = r["intervals"]
        print("%s %s: held-out rmse %.4f (posterior mean %.4f)  mean log density %.4f  CRPS %.4f  mean aleatoric variance %.4f, "
              "epistemic %.4f" % (name, what, r["rmse"], r["rmse_posterior_mean"], r["mean_log_density"], r["crps"],
                                  r["mean_aleatoric_var"], r["mean_epistemic_var"]))
        print("%s %s: 50 %% interval coverage %.3f mean width %.3f score %.3f;  90 %% interval coverage %.3f mean width %.3f "
              "score %.3f  (%d elements)" % (name, what, i50["coverage"], i50["mean_width"], i50["mean_interval_score"],
                                             i90["coverage"], i90["mean_width"], i90["mean_interval_score"], r["scored_elements"]))
    # ---- the predictive distribution at a quiet and at a noisy input (true noise sd 0.10 and 0.70), nothing read until the print
    probe = torch.zeros(2, 8, device=DEVICE)
    probe[0, 4], probe[1, 4] = -3.0, 3.0
    p = evaluate.predict_regression(models["alpha"], probe, SAMPLES, noise, levels=(0.9,))
    for i, what in enumerate(("quiet", "noisy")):
        print("%s at the %s input: mean %.3f  total sd %.3f  90 %% interval [%.3f, %.3f]"
              % (name, what, float(p["pred_mean"][i, 0]), float(p["total_std"][i, 0]), float(p["lower"][0, i, 0]),
                 float(p["upper"][0, i, 0])))


for hetero, dims, tag in ((True, (8, 32, 2), "heteroscedastic"), (False, (8, 32, 1), "homoscedastic twin")):
    torch.manual_seed(1)
    run("LRT %s" % tag, lrt.BayesianNetwork(dims, head="identity", priors=PRIORS, lambdal_init=INIT), hetero)
    torch.manual_seed(1)
    run("MNF %s" % tag, mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar", head="identity", priors=PRIORS,
                                            lambdal_init=INIT), hetero)
