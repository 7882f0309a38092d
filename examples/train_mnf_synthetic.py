#!/usr/bin/env python3
"""How a user of the reference's LBBNN-GP-MF-MNF.py switches to the HIP path: the script's own class definitions are
replaced by one import, its training iteration (:263-275: net(data, sample=True), nll + net.kl()/NUM_BATCHES, backward,
Adam step) and its ensemble test (:277-334: gamma.rsample(), net(data, sample=True) x TEST_SAMPLES, net(data,
sample=False)) run unchanged in meaning.  There is no dataset in this image, so MNIST-shaped synthetic data with learnable
labels stands in for the loaders.

    python examples/train_mnf_synthetic.py            # eager loop, the reference's default RNVP flows
    GRAPH=1 python examples/train_mnf_synthetic.py    # the same step captured once in a HIP graph and replayed
    FLOWS=Planar python examples/train_mnf_synthetic.py   # planar flows
Either way it ends with the median probability model (a frozen snapshot, evaluate.freeze).
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd.mnf import BayesianNetwork            # was: class Gaussian / Bernoulli / BayesianLinear / BayesianNetwork inline
from bnn_amd.evaluate import ensemble_eval

DEVICE = torch.device("cuda:0")
BATCH_SIZE, NUM_BATCHES, EPOCHS, TEST_SAMPLES = 1000, 12, 6, 10
bnn_amd.set_precision("bf16x3")
torch.manual_seed(1)                                # the reference seeds per run (:409); also seeds the in-kernel noise

FLOWS = os.environ.get("FLOWS", "RNVP")
net = BayesianNetwork(z_flow_type=FLOWS, r_flow_type=FLOWS).to(DEVICE)     # 784-400-600-10, RNVP flows, num_transforms=2 (:244-250)
optimizer = bnn_amd.optim.Adam(net.parameters(), lr=1e-3)      # torch.optim.Adam works too (:358)

g = torch.Generator(device=DEVICE).manual_seed(7)
proj = torch.randn(784, 10, device=DEVICE, generator=g)
train_x = torch.rand(NUM_BATCHES, BATCH_SIZE, 1, 28, 28, device=DEVICE, generator=g)
train_y = (train_x.view(NUM_BATCHES, BATCH_SIZE, 784) @ proj).argmax(-1)
test_x = torch.rand(BATCH_SIZE, 1, 28, 28, device=DEVICE, generator=g)
test_y = (test_x.view(BATCH_SIZE, 784) @ proj).argmax(-1)


# The epoch's statistics stay on the device: the fused loss adds every step to the monitor's running totals inside its own
# launch, and the optimizer runs behind the monitor's guard word, so a batch whose loss is not finite changes no parameter and
# is counted instead.  One host read per epoch (monitor.result()) replaces train()'s print(loss) / print(nll) per batch (:272-275).
monitor = bnn_amd.TrainMonitor(10, DEVICE)
optimizer.set_guard(monitor)


def elbo(net, data, target):
    outputs = net(data, sample=True)
    # = F.nll_loss(outputs, target, reduction="sum") + net.kl() / NUM_BATCHES, the reference's spelling, which still works
    return bnn_amd.elbo_loss(outputs, target, net.kl(), NUM_BATCHES, monitor=monitor)


net.train()
if os.environ.get("GRAPH") == "1":
    step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, train_x[0], train_y[0])
else:
    def step(data, target):
        net.zero_grad()
        loss = elbo(net, data, target)
        loss.backward()
        optimizer.step()
        return loss

for epoch in range(EPOCHS):
    monitor.reset()                                 # (also drops the warm-up steps of the graphed step's factory)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for b in range(NUM_BATCHES):
        loss = step(train_x[b], train_y[b])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / NUM_BATCHES * 1e3
    m = monitor.result()                            # the epoch's one host read
    print("epoch %d  nll %.4f per row  loss %.1f per batch (last batch: nll %.1f, loss %.1f)  accuracy %.3f  skipped steps %d  "
          "(%.2f ms/iteration)" % (epoch, m["nll_mean"], m["loss_mean"], m["last_nll"], m["last_loss"], m["accuracy"],
                                   m["skipped_steps"], ms))

res = ensemble_eval(net, test_x, test_y, samples=TEST_SAMPLES)
print("density %.3f | posterior mean %.3f | ensemble %.3f" % (float(res["density"].mean()),
      res["correct_posterior_mean"] / BATCH_SIZE, res["correct_ensemble"] / BATCH_SIZE))

# the median probability model of outofsample(net, loader, medimod=True) (LBBNN-GP-MF-MNF.py:342-366): keep a weight iff its
# inclusion probability exceeds 0.5 -- a frozen snapshot of the trained network, evaluated without touching the parameters
# again.  dense=True also takes the default RNVP / MNF-type z flows (every member's z in one lbbnn_flow_dense_members launch;
# members have the loop's draws and equal it to fp32 rounding); a planar network takes the same path with or without it.
if FLOWS in ("Planar", "RNVP", "MNF"):
    mpm = bnn_amd.evaluate.freeze(net, gates="mpm", dense=True)
    res = ensemble_eval(mpm, test_x, test_y, samples=TEST_SAMPLES)
    print("median probability model: density %.3f (kept per layer %s) | posterior mean %.3f | ensemble %.3f | mean predictive "
          "entropy %.3f" % (mpm.density, mpm.kept, res["correct_posterior_mean"] / BATCH_SIZE,
                            res["correct_ensemble"] / BATCH_SIZE,
                            float(bnn_amd.evaluate.predictive_entropy(res["outputs"]).mean())))
else:
    print("median probability model: evaluate.freeze takes planar, RNVP and MNF-type z flows (FLOWS=%s)" % FLOWS)

# A whole test pass with ONE host read: several test batches through an EvalAccumulator.  Every batch is the ensemble, the
# posterior-mean forward and one lbbnn_eval_metrics call whose running totals (correct counts, per-member corrects, nll sum,
# predictive entropy, confusion matrix) stay on the device; result() reads them when the pass is over -- what test_ensemble
# (:312-323) and outofsample (:370-392) accumulate on the host with an .item() per batch.
test_batches = []
for _ in range(4):
    bx = torch.rand(BATCH_SIZE, 1, 28, 28, device=DEVICE, generator=g)
    test_batches.append((bx, (bx.view(BATCH_SIZE, 784) @ proj).argmax(-1)))
model = mpm if FLOWS in ("Planar", "RNVP", "MNF") else net
tot = bnn_amd.evaluate.evaluate_batches(model, test_batches, samples=TEST_SAMPLES)
print("test pass over %d rows (one host read): ensemble %.3f | posterior mean %.3f | members %s | nll %.3f | mean predictive "
      "entropy %.3f" % (tot["rows"], tot["accuracy_ensemble"], tot["accuracy_posterior_mean"],
                        " ".join("%.3f" % (c / tot["rows_with_target"]) for c in tot["correct_member"]), tot["nll_mean"],
                        tot["entropy_mean"]))
if FLOWS in ("Planar", "RNVP", "MNF"):
    # ... and the same pass replayed from one HIP graph per batch (ensemble + posterior-mean forward + metrics, single stream)
    acc = bnn_amd.evaluate.EvalAccumulator(10, TEST_SAMPLES, DEVICE)
    eval_step = bnn_amd.graphs.make_graphed_eval_step(mpm, test_batches[0][0], test_batches[0][1], TEST_SAMPLES, acc)
    for bx, by in test_batches:
        eval_step(bx, by)
    tot = acc.result()
    print("graphed test pass: ensemble %.3f | posterior mean %.3f | confusion matrix diagonal %s"
          % (tot["accuracy_ensemble"], tot["accuracy_posterior_mean"], tot["confusion"].diagonal().tolist()))

# How good is the uncertainty?  One in-distribution pass and one pass on noise inputs through an UncertaintyAccumulator each
# (lbbnn_eval_uncertainty next to lbbnn_eval_metrics, the totals read once per pass): calibration, the epistemic part of the
# predictive entropy, and the out-of-distribution study of outofsample on FMNIST / KMNIST (LBBNN-GP-MF-LRT.py:283-286) as an AUROC.
ev = bnn_amd.evaluate
noise_batches = [(torch.randn(BATCH_SIZE, 1, 28, 28, device=DEVICE, generator=g), by) for _, by in test_batches]
passes = []
for batches in (test_batches, noise_batches):
    u = ev.UncertaintyAccumulator(10, TEST_SAMPLES, DEVICE)
    passes.append(ev.evaluate_batches(model, batches, samples=TEST_SAMPLES, uncertainty=u))
auroc, half_width = ev.ood_auroc(passes[0], passes[1], score="mutual_information")
print("uncertainty: ECE %.3f | Brier %.3f | log score %.3f | mean mutual information in-distribution %.4f, on noise %.4f | "
      "AUROC noise against test by mutual information %.3f +- %.3f"
      % (passes[0]["ece"], passes[0]["brier_mean"], passes[0]["log_score_mean"], passes[0]["mutual_information_mean"],
         passes[1]["mutual_information_mean"], auroc, half_width))
