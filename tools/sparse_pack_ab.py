#!/usr/bin/env python3
"""The sparse median-probability models against a built checkout of the parent commit: the bytes of everything they pack and
compute, and the time of their binds.

    python tools/sparse_pack_ab.py --parent DIR [--out profiles/sparse_pack_refactor_ab.txt] [--timeout 600]
    python tools/sparse_pack_ab.py --parent DIR --time        (appends to --out)

DIR is a tree of the parent commit with its library built (``git archive <commit> | tar -x -C DIR && make -C
DIR/bayesian-neural-nets_amd/csrc``).  Every child is a fresh process that imports ONE tree (tools/ab_trees.py); this process
never touches the device.

Bytes: the small cases of tests/frozen_sparse_ref.py, tests/base_sparse_ref.py and tests/threshold_sweep_ref.py (the 784-wide
ones left out; every threshold / threshold set of the tests), inputs seeded on the host.  Per model: every buffer of
``state_dict()``, ``ensemble(x, 3)`` at B = 65 and ``forward(x)``, each from Philox state (1, 0); for the two model families
every tensor of ``explain_ensemble(fz, x, 3, keep_weights=True)`` (``targets="pred"`` where the model has more than 16
outputs).  Per case ``identical`` or the first key that differs; exit status 1 unless every case is identical.

Time (--time): host-clock ms per bind, 5 windows of 10 binds after 3 warm-up binds, a synchronise at each end, of
``freeze(net, "mpm", sparse=True)`` and ``threshold_sweep(net, 8 thresholds)`` on tools/threshold_sweep_time.py's LRT
784-400-400-10 and MNF 784-1200-1200-10 networks and of ``freeze_base(net, "mpm", sparse=True)`` on tools/base_sparse_time.py's
784-400-600-10.  The parent and this tree alternate, each twice.  THE CONDITION, per bind: this tree's median window <= the
parent's median window * (1 + s), s = the parent's slowest window over its fastest, minus 1, over its two runs.  The C calls of
one ``ensemble`` and one ``explain_ensemble`` call of each model are listed for both trees and must be the same."""
import argparse
import math
import os
import pickle
import statistics
import sys
import time

import ab_trees

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sparse_pack_refactor_ab.txt"))
ap.add_argument("--timeout", type=int, default=600)
ap.add_argument("--time", action="store_true", help="the bind times and the call listings instead of the bytes")
ap.add_argument("--worker", default=None, help="(internal) the tree to import, in a child process")
ap.add_argument("--dump", default=None, help="(internal) where the child leaves its result")
args = ap.parse_args()

THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.975, 0.99)
WINDOWS, BINDS, WARMUP = 5, 10, 3


def tensors(prefix, v, out):
    """Every tensor of a result (a tensor, or lists / dicts of them) as bytes under ``prefix``."""
    import torch
    if torch.is_tensor(v):
        out[prefix] = v.contiguous().cpu().numpy().tobytes()
    elif isinstance(v, dict):
        for k, u in v.items():
            tensors("%s.%s" % (prefix, k), u, out)
    elif isinstance(v, (list, tuple)):
        for k, u in enumerate(v):
            tensors("%s.%d" % (prefix, k), u, out)


def load(tree):
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    import torch
    import bnn_amd
    assert os.path.abspath(bnn_amd.__file__).startswith(os.path.abspath(tree) + os.sep), bnn_amd.__file__
    bnn_amd.set_precision("fp32")
    return torch, bnn_amd, torch.device("cuda:0")


def family_net(bnn, dev, family, dims, T, head, lams):
    import frozen_sparse_ref as sr
    if family == "lrt":
        net = bnn.lrt.BayesianNetwork(dims, head=head)
    else:
        net = bnn.mnf.BayesianNetwork(dims, T, z_flow_type="Planar", r_flow_type="Planar", head=head)
    net = net.to(dev).eval()
    sr.apply(net, lams)
    return net


def bytes_worker(tree, dump):
    torch, bnn, dev = load(tree)
    import base_sparse_ref as br
    import frozen_sparse_ref as sr
    import threshold_sweep_ref as tr
    ev = bnn.evaluate
    out = {}

    def model(case, fz, I, explain):
        x = torch.rand(65, I, generator=torch.Generator().manual_seed(66)).to(dev)
        tensors(case + "/state", dict(fz.state_dict()), out)
        bnn.manual_seed(1, 0)
        tensors(case + "/ensemble", fz.ensemble(x, 3), out)
        bnn.manual_seed(1, 0)
        tensors(case + "/forward", fz(x), out)
        if explain:
            bnn.manual_seed(1, 0)
            targets = None if fz.dims[-1] <= 16 else "pred"
            tensors(case + "/explain", ev.explain_ensemble(fz, x, 3, targets=targets, keep_weights=True), out)

    for name, (family, dims, T, head) in zip(sr.IDS, sr.CASES):
        if 784 in dims:
            continue
        for th in sr.THRESHOLDS:
            torch.manual_seed(11)
            net = family_net(bnn, dev, family, dims, T, head, sr.lambdals(dims, th)[0])
            model("freeze %s threshold=%g" % (name, th), ev.freeze(net, "mpm", threshold=th, sparse=True), dims[0], True)
    for name, (dims, head) in zip(br.IDS, br.CASES):
        for th in sr.THRESHOLDS:
            net = br.make_net(bnn, dev, dims, head, th)
            model("freeze_base %s threshold=%g" % (name, th), br.freeze_sparse(ev, net, head, th), dims[0], True)
    for name, (family, dims, T, head) in zip(tr.IDS, tr.CASES):
        for set_name, (thresholds, span, empty_last) in tr.SETS.items():
            torch.manual_seed(11)
            lams = tr.lambdals(dims, thresholds, span=span, empty_last=empty_last)[0]
            net = family_net(bnn, dev, family, dims, T, head, lams)
            model("threshold_sweep %s %s" % (name, set_name), ev.threshold_sweep(net, thresholds), dims[0], False)
    torch.cuda.synchronize()
    with open(dump, "wb") as fh:
        pickle.dump(out, fh)


def time_worker(tree, dump):
    torch, bnn, dev = load(tree)
    from bnn_amd import _lib
    ev = bnn.evaluate
    g = torch.Generator().manual_seed(7)

    def sweep_net(kind, dims):                               # tools/threshold_sweep_time.py's
        torch.manual_seed(0)
        if kind == "mnf":
            net = bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
        else:
            net = bnn.lrt.BayesianNetwork(dims)
        net = net.to(dev).eval()
        scale = math.log(0.99 / 0.01) / math.log(10.0)
        with torch.no_grad():
            for l in net._layers():
                shape = (l.out_features, l.in_features)
                low = torch.empty(shape).uniform_(-6.0, -0.5, generator=g)
                high = torch.empty(shape).exponential_(1.0 / scale, generator=g)
                l.lambdal.copy_(torch.where(torch.rand(shape, generator=g) < 0.1, high, low).to(dev))
        return net

    def base_net(dims):                                      # tools/base_sparse_time.py's
        torch.manual_seed(0)
        net = bnn.base.BayesianNetwork(dims).to(dev).eval()
        with torch.no_grad():
            for l in net._layers():
                l.lambdal.copy_(torch.empty(l.out_features, l.in_features).uniform_(-3, 3, generator=g).to(dev))
        return net

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(BINDS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / BINDS

    def c_calls(fn):
        _lib.RECORD = []
        try:
            fn()
            return " ".join(r[0].replace("lbbnn_", "") for r in _lib.RECORD)
        finally:
            _lib.RECORD = None

    lrt, mnf = sweep_net("lrt", (784, 400, 400, 10)), sweep_net("mnf", (784, 1200, 1200, 10))
    base = base_net((784, 400, 600, 10))
    binds = {"freeze lrt 784-400-400-10": lambda: ev.freeze(lrt, "mpm", sparse=True),
             "freeze mnf 784-1200-1200-10": lambda: ev.freeze(mnf, "mpm", sparse=True),
             "threshold_sweep lrt 784-400-400-10": lambda: ev.threshold_sweep(lrt, THRESHOLDS),
             "threshold_sweep mnf 784-1200-1200-10": lambda: ev.threshold_sweep(mnf, THRESHOLDS),
             "freeze_base 784-400-600-10": lambda: ev.freeze_base(base, "mpm", sparse=True)}
    res = {"windows": {}, "calls": {}}
    x = torch.rand(100, 784, generator=torch.Generator().manual_seed(1)).to(dev)
    for name, bind in binds.items():
        for _ in range(WARMUP):
            bind()
        res["windows"][name] = [window(bind) for _ in range(WINDOWS)]
        fz = bind()
        res["calls"][name + " ensemble"] = c_calls(lambda: fz.ensemble(x, 10))
        if not name.startswith("threshold_sweep"):
            res["calls"][name + " explain_ensemble"] = c_calls(lambda: ev.explain_ensemble(fz, x, 3, targets="pred"))
    with open(dump, "wb") as fh:
        pickle.dump(res, fh)


def time_main():
    runs = {"parent": [], "this tree": []}
    for _ in range(2):                                       # parent, this tree, parent, this tree
        for name, r in ab_trees.child_dumps(__file__, args.parent, args.timeout, extra=("--time",)).items():
            runs[name].append(r)
    lines = ["", "bind times: ms per bind on the host clock, %d windows of %d binds after %d warm-up binds, per run; the parent "
             "and this tree alternate, each twice, a fresh process per run" % (WINDOWS, BINDS, WARMUP)]
    fmt = lambda v: " ".join("%.4f" % u for u in v)
    bad = 0
    for name in runs["parent"][0]["windows"]:
        p = [w for r in runs["parent"] for w in r["windows"][name]]
        t = [w for r in runs["this tree"] for w in r["windows"][name]]
        s = max(p) / min(p) - 1.0
        ok = statistics.median(t) <= statistics.median(p) * (1.0 + s)
        bad += not ok
        lines.append("%-38s parent [%s] median %.4f  s = %.1f %%\n%-38s this   [%s] median %.4f  bound %.4f: %s"
                     % (name, fmt(p), statistics.median(p), 100 * s, "", fmt(t), statistics.median(t),
                        statistics.median(p) * (1.0 + s), "HOLDS" if ok else "DOES NOT HOLD"))
    lines.append("C calls of one call, parent | this tree")
    for name, calls in runs["parent"][0]["calls"].items():
        mine = runs["this tree"][0]["calls"][name]
        bad += mine != calls
        lines.append("%s: %s\n  parent: %s\n  this:   %s" % (name, "the same" if mine == calls else "DIFFERENT", calls, mine))
    lines.append("every condition holds" if not bad else "%d condition(s) DO NOT HOLD" % bad)
    print("\n".join(lines), flush=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if bad else 0


def main():
    if args.parent is None:
        sys.exit("sparse_pack_ab: --parent DIR (a built checkout of the parent commit) is required")
    if args.time:
        sys.exit(time_main())
    sys.exit(ab_trees.report(__file__, ab_trees.child_dumps(__file__, args.parent, args.timeout), args.parent, args.out))


if __name__ == "__main__":
    if args.worker:
        (time_worker if args.time else bytes_worker)(args.worker, args.dump)
    else:
        main()
