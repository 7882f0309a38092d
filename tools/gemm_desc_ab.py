#!/usr/bin/env python3
"""Byte comparison of whole-network forwards and backwards against a built checkout of the parent commit, for the change that
moved the train and finalize forms of the dual-moment GEMM onto the descriptor: same C calls in the same
order, same bits out.

    python tools/gemm_desc_ab.py --parent DIR [--out profiles/gemm_desc_ab.txt] [--timeout 300]

DIR is a tree of the parent commit with its library built (``git archive <commit> | tar -x -C DIR && make -C
DIR/bayesian-neural-nets_amd/csrc``).  An LRT and a planar-MNF network of 40-48-24-10 and 64-96-80-10 at B = 5 and 64 in fp32,
bf16x3, bf16 and fp16x3f run four passes each -- the train-mode no-grad forward with KL, the eval forward (posterior mean, and
sampled), one forward + backward -- from fixed seeds, once with DIR's package and library and once with this tree's, each in a
fresh child process under its own time limit; this process never touches the device (tools/ab_trees.py).  A child dumps the raw
bytes of the output, every layer's KL and the total, every parameter gradient, the Philox state afterwards, and the names of
the C calls the pass made (``_lib.RECORD``), with the parent's ``lbbnn_lrt_gemm_train`` / ``lbbnn_lrt_gemm_finalize_adv`` read
as ``lbbnn_lrt_gemm_ex``.  Per case: ``identical`` or the first key that differs; exit status 1 unless every case is identical."""
import argparse
import os
import pickle
import sys

import ab_trees

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--out", default=os.path.join(ab_trees.HERE, "profiles", "gemm_desc_ab.txt"))
ap.add_argument("--timeout", type=int, default=300)
ap.add_argument("--worker", default=None, help="(internal) the tree to import, in a child process")
ap.add_argument("--dump", default=None, help="(internal) where the child leaves its bytes")
args = ap.parse_args()

NOW = {"lbbnn_lrt_gemm_train": "lbbnn_lrt_gemm_ex", "lbbnn_lrt_gemm_finalize_adv": "lbbnn_lrt_gemm_ex"}


def worker(tree, dump):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import bnn_amd
    from bnn_amd import _lib, ops
    assert os.path.abspath(bnn_amd.__file__).startswith(os.path.abspath(tree) + os.sep), bnn_amd.__file__
    dev = torch.device("cuda:0")
    out = {}

    def keep(case, calls, **tensors):
        for k, v in tensors.items():
            out["%s/%s" % (case, k)] = v.detach().contiguous().cpu().numpy().tobytes()
        out["%s/calls" % case] = "\n".join(NOW.get(c[0], c[0]) for c in calls).encode()

    def recorded(fn):
        _lib.RECORD = []
        try:
            return fn(), _lib.RECORD
        finally:
            _lib.RECORD = None

    def state(net):
        kls = {"kl%d" % i: l.kl for i, l in enumerate(net._layers()) if torch.is_tensor(l.kl)}
        return dict(kls, rng=ops.RngState.get(dev).t)

    seed = 0
    for kind in ("lrt", "mnf"):
        for dims in ((40, 48, 24, 10), (64, 96, 80, 10)):
            for B in (5, 64):
                seed += 1
                rng = np.random.default_rng(seed)
                x = torch.from_numpy(rng.random((B, dims[0])).astype(np.float32)).to(dev)
                t = torch.from_numpy(rng.integers(0, dims[-1], B).astype(np.int64)).to(dev)
                for precision in ("fp32", "bf16x3", "bf16", "fp16x3f"):
                    torch.manual_seed(0)
                    net = (bnn_amd.lrt.BayesianNetwork(dims) if kind == "lrt" else
                           bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")).to(dev)
                    net.set_precision(precision)
                    case = "%s %s B=%d %s" % (kind, "-".join(map(str, dims)), B, precision)

                    def forward(sample):
                        with torch.no_grad():
                            y = net(x, sample=sample)
                            return y, (net.kl() if net.training else None)

                    net.train()
                    bnn_amd.manual_seed(11, 3)
                    (y, kl), calls = recorded(lambda: forward(True))
                    keep(case + " train no-grad", calls, out=y, kl=kl, **state(net))
                    net.eval()
                    for sample in (False, True):
                        bnn_amd.manual_seed(12, 5)
                        (y, _), calls = recorded(lambda: forward(sample))
                        keep(case + " eval sample=%d" % sample, calls, out=y, rng=ops.RngState.get(dev).t)
                    net.train()
                    bnn_amd.manual_seed(13, 7)

                    def step():
                        y = net(x, sample=True)
                        kl = net.kl()
                        loss = bnn_amd.elbo_loss(y, t, kl, 5.0)
                        loss.backward()
                        return y, kl, loss

                    (y, kl, loss), calls = recorded(step)
                    keep(case + " forward + backward", calls, out=y, kl=kl, loss=loss, **state(net),
                         **{"grad_" + k: p.grad for k, p in net.named_parameters() if p.grad is not None})

    torch.cuda.synchronize()
    with open(dump, "wb") as fh:
        pickle.dump(out, fh)


def main():
    if args.parent is None:
        sys.exit("gemm_desc_ab: --parent DIR (a built checkout of the parent commit) is required")
    sys.exit(ab_trees.report(__file__, ab_trees.child_dumps(__file__, args.parent, args.timeout), args.parent, args.out))


if __name__ == "__main__":
    worker(args.worker, args.dump) if args.worker else main()
