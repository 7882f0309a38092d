#!/usr/bin/env python3
"""The MNF simulation study of the latent-binary papers (LBBNN-GP-MF-MNFsim_study.py) as ONE call: 100 replicate networks
20 -> 1 (one MNF layer with two planar transforms per flow, a sigmoid head), seeds 0 .. 99, each trained for EPOCHS epochs of 5
batches on BCELoss(sum) + kl / NUM_BATCHES with Adam in the script's three groups -- the layer's named tensors, the z_flow and
the r_flow parameters, each with its own rate per segment -- the optimizer re-created at epochs 50 / 100 / 450 of 500, all
inside the launches of ``bnn_amd.study.fit_mnf_replicates`` (one workgroup per replicate); then the script's closing numbers
from ``study.selection_summary``.  The script's flows are RNVP; the replicate kernel runs planar flows.

The data are synthetic and made here, as in examples/sim_study_synthetic.py: 2000 rows of 20 standard-normal covariates, a sparse
weight vector of this script's own (five non-zero entries), y ~ Bernoulli(sigmoid(x . w)); every replicate sees the same rows.

    python examples/sim_study_mnf_replicates_synthetic.py
    EPOCHS=100 REPLICATES=20 python examples/sim_study_mnf_replicates_synthetic.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd import Priors, study

DEVICE = torch.device("cuda:0")
FEATURES, ROWS, BATCH_SIZE = 20, 2000, 400
EPOCHS = int(os.environ.get("EPOCHS", "500"))
REPLICATES = int(os.environ.get("REPLICATES", "100"))
PRIORS = Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)

g = torch.Generator().manual_seed(3)
w_true = torch.zeros(FEATURES)
w_true[[1, 4, 9, 12, 17]] = torch.tensor([2.0, -1.5, 1.0, -2.5, 1.5])
x_all = torch.randn(ROWS, FEATURES, generator=g)
y_all = (torch.rand(ROWS, generator=g) < torch.sigmoid(x_all @ w_true)).float().reshape(ROWS, 1)
x_all, y_all = x_all.to(DEVICE), y_all.to(DEVICE)
support = w_true != 0

# the script's schedule, scaled to EPOCHS: four segments that begin at 0, 10 %, 20 % and 90 % of the run, a fresh optimizer at
# the start of the last three, and per segment the rates of the three groups
switch = [EPOCHS // 10, EPOCHS // 5, (9 * EPOCHS) // 10]
BASE = (0.01, 0.01, 0.001, 0.001)
Z_FLOW = (0.004, 0.003, 0.002, 0.0004)
R_FLOW = (0.0035, 0.003, 0.002, 0.0004)
segment = [sum(e >= s for s in switch) for e in range(EPOCHS)]
restarts = sorted({e for e in switch if 0 < e < EPOCHS})

nets = study.make_mnf_replicates(REPLICATES, (FEATURES, 1), num_transforms=2, priors=PRIORS, device=DEVICE)   # seeds 0 .. R - 1
res = study.fit_mnf_replicates(nets, x_all, y_all, EPOCHS, BATCH_SIZE, lr=[BASE[k] for k in segment],
                               lr_z_flow=[Z_FLOW[k] for k in segment], lr_r_flow=[R_FLOW[k] for k in segment],
                               restarts=restarts, seeds=list(range(REPLICATES)))
hist = res.history[:, -1].mean(dim=0).tolist()                                                 # the first host read
print("%d MNF replicates, %d epochs: last epoch, mean over replicates: loss %.2f  nll %.2f  training accuracy %.3f; skipped steps %d"
      % (REPLICATES, EPOCHS, hist[0], hist[1], hist[2], int(res.skipped_steps.sum())))
s = study.selection_summary(res.inclusion_probabilities[:, 0], support.to(DEVICE))
print("RMSE x 100 per covariate:", " ".join("%.1f" % v for v in s["rmse"].tolist()), "| mean %.2f" % float(s["rmse_mean"]))
print("agreement per covariate :", " ".join("%.2f" % v for v in s["agreement_covariate"].tolist()))
print("agreement per replicate : min %.2f mean %.2f" % (float(s["agreement_replicate"].min()), float(s["agreement_replicate"].mean())))
print("true-positive rate %.3f  false-positive rate %.3f (true support %s)"
      % (float(s["true_positive_rate"]), float(s["false_positive_rate"]), support.nonzero().reshape(-1).tolist()))
mpm = bnn_amd.evaluate.freeze(nets[0], gates="mpm")
out = bnn_amd.evaluate.evaluate_batches(mpm, [(x_all, y_all)], samples=10)
print("replicate 0, median probability model: %d of %d weights kept, ensemble accuracy %.3f on the training rows"
      % (mpm.kept[0], FEATURES, out["accuracy_ensemble"]))
