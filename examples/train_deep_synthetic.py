#!/usr/bin/env python3
"""A network of a depth of your own choosing: ``mnf.BayesianNetwork(dims, ...)`` and ``lrt.BayesianNetwork(dims)`` build
l1 .. lN for 1 to 16 layers (ReLU between them, log_softmax after the last).  Here a five-layer MNF network with planar flows
trains on synthetic 64-feature data with the whole step -- forward, backward, Adam -- captured once in a HIP graph
(graphs.make_graphed_train_step), then its median probability model is frozen and evaluated.  Five layers are more than one
batched launch holds (4): the batched C calls go out in two groups of consecutive layers and the network KL is one
lbbnn_kl_total launch; nothing in the script has to know.

    python examples/train_deep_synthetic.py
    DEPTH=9 python examples/train_deep_synthetic.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import bnn_amd
from bnn_amd.mnf import BayesianNetwork

DEVICE = torch.device("cuda:0")
DEPTH = int(os.environ.get("DEPTH", "5"))
FEATURES, CLASSES, WIDTH = 64, 10, 64
BATCH_SIZE, NUM_BATCHES, EPOCHS, TEST_SAMPLES = 1024, 64, 10, 10     # 65536 rows: the likelihood outweighs the prior
torch.manual_seed(1)

dims = (FEATURES,) + (WIDTH,) * (DEPTH - 1) + (CLASSES,)
net = BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar").to(DEVICE)
with torch.no_grad():
    for layer in net._layers():
        # the reference's weight_mu ~ U(+-0.01) is made for 784 inputs and three layers: through more, narrower layers nothing
        # of the input arrives.  A He-style start keeps the signal (and the gradient) alive at any depth.
        layer.weight_mu.normal_(0.0, (2.0 / layer.in_features) ** 0.5)
print("layers:", [name for name, _ in net.named_children()], "dims", net.dims)
optimizer = bnn_amd.optim.Adam(net.parameters(), lr=2e-3)

g = torch.Generator(device=DEVICE).manual_seed(7)
proj = torch.randn(FEATURES, CLASSES, device=DEVICE, generator=g)
train_x = torch.rand(NUM_BATCHES, BATCH_SIZE, FEATURES, device=DEVICE, generator=g)
train_y = ((train_x - 0.5) @ proj).argmax(-1)              # centred: ten classes of similar size
test_x = torch.rand(BATCH_SIZE, FEATURES, device=DEVICE, generator=g)
test_y = ((test_x - 0.5) @ proj).argmax(-1)


def elbo(net, data, target):
    outputs = net(data, sample=True)
    return F.nll_loss(outputs, target, reduction="sum") + net.kl() / NUM_BATCHES


net.train()
step = bnn_amd.graphs.make_graphed_train_step(net, optimizer, elbo, train_x[0], train_y[0])
for epoch in range(EPOCHS):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for b in range(NUM_BATCHES):
        loss = step(train_x[b], train_y[b])
    torch.cuda.synchronize()
    if epoch % 2 == 1:
        print("epoch %d  loss %.1f  (%.2f ms/iteration)" % (epoch, float(loss.detach()), (time.perf_counter() - t0) / NUM_BATCHES * 1e3))

res = bnn_amd.evaluate.ensemble_eval(net, test_x, test_y, samples=TEST_SAMPLES)
print("density %.3f | posterior mean %.3f | ensemble %.3f" % (float(res["density"].mean()),
      res["correct_posterior_mean"] / BATCH_SIZE, res["correct_ensemble"] / BATCH_SIZE))
mpm = bnn_amd.evaluate.freeze(net, gates="mpm")
res = bnn_amd.evaluate.ensemble_eval(mpm, test_x, test_y, samples=TEST_SAMPLES)
print("median probability model: density %.3f (kept per layer %s) | posterior mean %.3f | ensemble %.3f"
      % (mpm.density, mpm.kept, res["correct_posterior_mean"] / BATCH_SIZE, res["correct_ensemble"] / BATCH_SIZE))
