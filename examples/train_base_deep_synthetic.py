#!/usr/bin/env python3
"""A five-layer baseline LBBNN (bnn_amd.base.BayesianNetwork of any depth from 1 to 16 layers) trained from ONE HIP graph on
synthetic data (there is no dataset in this image): the step draws its gates and Gamma precisions inside the HIP kernels
(sample_elbo(draws="hip")), log_prior and log_q of the five layers are one lbbnn_fold_rows launch, and bnn_amd.optim.Adam
updates the 55 parameter tensors in one launch.  Then a whole evaluation pass with one host read (evaluate.evaluate_batches):
the sampled gates and the median probability model, with the uncertainty totals.

    python examples/train_base_deep_synthetic.py               # graphed hip-draw step
    EAGER=1 python examples/train_base_deep_synthetic.py       # the same step, eager
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bnn_amd
from bnn_amd.base import BayesianNetwork

DEVICE = torch.device("cuda:0")
DIMS = (64, 128, 96, 64, 32, 10)                       # five layers: the batched evaluation launch goes out in two groups (4 + 1)
BATCH_SIZE, NUM_BATCHES, EPOCHS = 100, 60, 4
torch.manual_seed(0)                                   # also seeds the in-kernel draws

net = BayesianNetwork(DIMS).to(DEVICE)
layers = net._layers()                                 # net.l1 .. net.l5
bnn_amd.base.NUM_BATCHES = NUM_BATCHES
optimizer = bnn_amd.optim.Adam([{"params": [p for n, p in net.named_parameters() if not n.endswith("lambdal")], "lr": 1e-3},
                                {"params": [l.lambdal for l in layers], "lr": 0.1}])

g = torch.Generator(device=DEVICE).manual_seed(7)
proj = torch.randn(DIMS[0], DIMS[-1], device=DEVICE, generator=g)
train_x = torch.rand(NUM_BATCHES, BATCH_SIZE, DIMS[0], device=DEVICE, generator=g)
train_y = ((train_x - 0.5) @ proj).argmax(-1)


def elbo(net, data, target):
    return net.sample_elbo(data, target, draws="hip")[0]


net.train()
if os.environ.get("EAGER") == "1":
    def step(data, target):
        net.zero_grad()
        loss = elbo(net, data, target)
        loss.backward()
        optimizer.step()
        return loss
else:
    step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, train_x[0], train_y[0])

for epoch in range(EPOCHS):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for b in range(NUM_BATCHES):
        loss = step(train_x[b], train_y[b])
    torch.cuda.synchronize()
    print("epoch %d  loss %.1f  (%.3f ms/iteration)" % (epoch, float(loss.detach()), (time.perf_counter() - t0) / NUM_BATCHES * 1e3))
with torch.no_grad():
    print("mean inclusion probability per layer:", ["%.3f" % float(l.alpha.mean()) for l in layers])

# the forward of the reference's scripts takes one gate per layer, by position or as g1= ... gN=
with torch.no_grad():
    gates = [l.gamma.rsample().to(DEVICE) for l in layers]
    out = net(train_x[0], *gates, sample=True)
    assert out.shape == (BATCH_SIZE, DIMS[-1])

# a test pass with ONE host read: hard gates as the reference sets them before its test, ten members per batch
for l in layers:
    l.gamma.exact = True
test_batches = []
for _ in range(5):
    bx = torch.rand(200, DIMS[0], device=DEVICE, generator=g)
    test_batches.append((bx, ((bx - 0.5) @ proj).argmax(-1)))
for gates in ("sample", "mpm"):
    unc = bnn_amd.evaluate.UncertaintyAccumulator(DIMS[-1], 10, DEVICE)
    tot = bnn_amd.evaluate.evaluate_batches(net, test_batches, samples=10, gates=gates, uncertainty=unc)
    print("test pass over %d rows, gates=%s: ensemble %.3f | posterior mean %.3f | nll %.3f | mean predictive entropy %.3f | "
          "model-averaged accuracy %.3f"
          % (tot["rows"], gates, tot["accuracy_ensemble"], tot["accuracy_posterior_mean"], tot["nll_mean"], tot["entropy_mean"],
             tot["correct_bma"] / tot["rows_with_target"]))
