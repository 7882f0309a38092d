#!/usr/bin/env python3
"""Byte comparison of the evaluation metrics against a built checkout of the parent commit: a tolerance cannot show that a
refactor kept the order of the additions, equal bytes can.

    python tools/eval_totals_ab.py --parent DIR [--out profiles/eval_totals_refactor_ab.txt] [--timeout 300]

DIR is a tree of the parent commit with its library built (``git archive <commit> | tar -x -C DIR && make -C
DIR/bayesian-neural-nets_amd/csrc``).  A fixed list of small cases -- inputs from seeded numpy on the host -- goes through the
public calls (ensemble_metrics, ensemble_uncertainty, ensemble_regression, ensemble_scores, explain + ExplanationAccumulator),
once with DIR's package and library and once with this tree's, each in a fresh child process under its own time limit; this
process never touches the device.  A child dumps the raw bytes of every per-row / per-element output and of the accumulator's
``_totals`` after TWO updates (the second one exercises the ``+=`` of the sums launch).  Per case the dumps are compared:
``identical`` or the first key that differs.  The run stops at the first child that fails; exit status 1 unless every case is
identical."""
import argparse
import os
import pickle
import sys

import ab_trees

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "eval_totals_refactor_ab.txt"))
ap.add_argument("--timeout", type=int, default=300)
ap.add_argument("--worker", default=None, help="(internal) the tree to import, in a child process")
ap.add_argument("--dump", default=None, help="(internal) where the child leaves its bytes")
args = ap.parse_args()


def lanes(C):
    G = 1
    while G < C:
        G <<= 1
    return G


def worker(tree, dump):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import bnn_amd
    from bnn_amd import evaluate
    assert os.path.abspath(bnn_amd.__file__).startswith(os.path.abspath(tree) + os.sep), bnn_amd.__file__
    dev = torch.device("cuda:0")
    out = {}
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def keep(case, res, acc=None):
        for k, v in res.items():
            if torch.is_tensor(v):
                out["%s/%s" % (case, k)] = v.contiguous().cpu().numpy().tobytes()
        if acc is not None:
            out["%s/_totals" % case] = acc._totals.cpu().numpy().tobytes()

    def twice(case, call, acc):
        """The call's outputs, and with an accumulator the totals after two updates."""
        keep(case + " #1", call())
        if acc is not None:
            keep(case + " #2", call(), acc)

    def log_probs(rng, S, B, C, wide=0):
        z = rng.standard_normal((S, B, C + wide)).astype(np.float32)
        z[..., :C] -= np.log(np.exp(z[..., :C].astype(np.float64)).sum(-1, keepdims=True)).astype(np.float32)
        if C > 1:
            z[0, 0, C - 1] = -np.inf
            z[S - 1, B // 2, 0] = -np.inf
        if B > 1:
            z[S // 2, B - 1, 0] = np.nan
        t = rng.integers(0, C, B)
        t[0] = -1 if B > 1 else t[0]
        t[B // 3] = C if B > 2 else t[B // 3]
        return z, t.astype(np.int64), rng.standard_normal((B, C)).astype(np.float32)

    # ---- metrics and uncertainty: every G, one row / a partial last workgroup of three, the member loop's tail, S = 1
    variants = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0))            # (mean_outputs, target, accumulator)
    seed = 0
    for C in (1, 2, 3, 5, 10, 17, 33, 64):
        for B in (1, 2 * (256 // lanes(C)) + 1):
            for S in (1, 4, 5):
                seed += 1
                z, t, m = log_probs(np.random.default_rng(seed), S, B, C)
                o, tt, mm = up(z), up(t), up(m)
                for wm, wt, wa in variants:
                    case = "C=%d B=%d S=%d mean=%d target=%d acc=%d" % (C, B, S, wm, wt, wa)
                    acc = evaluate.EvalAccumulator(C, S, dev) if wa else None
                    twice("metrics " + case, lambda: evaluate.ensemble_metrics(o, tt if wt else None, mm if wm else None, acc=acc), acc)
                    if not wm:
                        acc = evaluate.UncertaintyAccumulator(C, S, dev) if wa else None
                        twice("uncertainty " + case, lambda: evaluate.ensemble_uncertainty(o, tt if wt else None, acc=acc), acc)
    z, t, m = log_probs(np.random.default_rng(1000), 4, 70, 10, wide=6)                # a strided member block
    o, tt, mm = up(z)[:, :, :10], up(t), up(m)
    acc = evaluate.EvalAccumulator(10, 4, dev)
    twice("metrics strided", lambda: evaluate.ensemble_metrics(o, tt, mm, acc=acc), acc)
    acc = evaluate.UncertaintyAccumulator(10, 4, dev)
    twice("uncertainty strided", lambda: evaluate.ensemble_uncertainty(o, tt, acc=acc), acc)
    z, t, m = log_probs(np.random.default_rng(1001), 1025, 3, 3)                       # crosses the member chunk of 1024
    o, tt, mm = up(z), up(t), up(m)
    acc = evaluate.EvalAccumulator(3, 1025, dev)
    twice("metrics S=1025", lambda: evaluate.ensemble_metrics(o, tt, mm, acc=acc), acc)
    z, t, m = log_probs(np.random.default_rng(1002), 4, 70, 10)
    o, tt = up(z), up(t)
    for M in (1, 20, 100):
        for K in (1, 1024, 4096):
            acc = evaluate.UncertaintyAccumulator(10, 4, dev, conf_bins=M, hist_bins=K)
            twice("uncertainty conf_bins=%d hist_bins=%d" % (M, K), lambda: evaluate.ensemble_uncertainty(o, tt, acc=acc), acc)

    # ---- regression: B * units = 1, 256 exactly, and past two workgroups with a partial third (517 where units divides it)
    def regression_inputs(rng, S, B, O):
        centre = 2.0 * rng.standard_normal((B, O))
        o = (centre[None] + 0.4 * rng.standard_normal((S, B, O))).astype(np.float32)
        y = (centre + rng.standard_normal((B, O))).astype(np.float32)
        if B > 2:
            y[1, 0], y[2, O - 1] = np.nan, np.inf
            o[S - 1, B - 1, 0] = np.inf
        lv = (-0.5 + 0.5 * rng.standard_normal(O)).astype(np.float32)
        if O > 1:
            lv[1] = np.inf
        return o, y, lv, rng.standard_normal((B, O)).astype(np.float32)

    for O, Bs in ((1, (1, 256, 517)), (3, (86, 173)), (16, (16, 33))):
        for B in Bs:
            for S in (1, 4, 5):
                seed += 1
                o, y, lv, m = (up(v) for v in regression_inputs(np.random.default_rng(seed), S, B, O))
                for wm, wt, wa, K in ((1, 1, 1, 20), (0, 1, 1, 1), (0, 1, 1, 1024), (0, 0, 1, 20), (1, 1, 0, 0), (0, 0, 0, 0)):
                    case = "regression units=%d B=%d S=%d mean=%d target=%d pit_bins=%d" % (O, B, S, wm, wt, K)
                    acc = evaluate.RegressionAccumulator(O, S, dev, lv, pit_bins=K) if wa else None
                    twice(case, lambda: evaluate.ensemble_regression(o, y if wt else None, lv, m if wm else None, acc=acc), acc)

    # ---- scores: B * units = 1, 64, 129; the quantiles' split over the waves; every layout of the log-variance
    def scores_case(case, rng, S, B, O, levels, form, wt=1, wa=1, wm=1):
        o, y, _, m = regression_inputs(rng, S, B, O)
        o[~np.isfinite(o)] = 0.25
        lv3 = (-0.5 + 0.5 * rng.standard_normal((S, B, O))).astype(np.float32)
        lv3[S - 1, B - 1, O - 1] = 81.0                                                # beyond +-80: the element is not finite
        per_batch = None
        if form == "number":
            own = -0.75
        elif form == "units":
            own = up(lv3[0, 0])
        elif form == "output":
            own, o, m = "output", np.concatenate([o, lv3], -1), np.concatenate([m, m], -1)
        else:
            own, per_batch = 0.0, up(lv3[0] if form == "element" else lv3)
        o, y, m = up(o), up(y) if wt else None, up(m) if wm else None
        if wa:
            acc = evaluate.RegressionScoreAccumulator(O, S, dev, own, pit_bins=20, levels=levels)
            twice(case, lambda: acc.update(o, y, m, log_var=per_batch), acc)
        else:
            twice(case, lambda: evaluate.ensemble_scores(o, y, own if per_batch is None else per_batch, m, levels=levels), None)

    all_levels = ((), (0.9,), (0.5, 0.9, 0.99), (0.5, 0.8, 0.9, 0.95))
    forms = ("number", "units", "element", "member", "output")
    for S in (1, 2, 5, 64):
        for levels in all_levels:
            for form in forms:
                seed += 1
                scores_case("scores units=3 B=43 S=%d levels=%d log_var=%s" % (S, len(levels), form),
                            np.random.default_rng(seed), S, 43, 3, levels, form)
    for O, B in ((1, 1), (1, 64), (1, 129), (16, 4)):
        for form in ("units", "member"):
            seed += 1
            scores_case("scores units=%d B=%d S=5 levels=3 log_var=%s" % (O, B, form), np.random.default_rng(seed), 5, B, O,
                        all_levels[2], form)
    for wt, wa, wm in ((0, 1, 0), (1, 0, 1), (0, 0, 0)):
        for form in ("units", "member", "output"):
            seed += 1
            scores_case("scores units=3 B=43 S=5 levels=4 log_var=%s target=%d acc=%d mean=%d" % (form, wt, wa, wm),
                        np.random.default_rng(seed), 5, 43, 3, all_levels[3], form, wt, wa, wm)

    # ---- explanation totals (the Python side only: the kernels are not part of the comparison's subject)
    torch.manual_seed(0)
    fz = evaluate.freeze(bnn_amd.lrt.BayesianNetwork((8, 32, 3)).to(dev).eval(), gates="mpm")
    x = up(np.random.default_rng(2000).standard_normal((37, 8)).astype(np.float32))
    for targets in (None, "pred"):
        acc = evaluate.ExplanationAccumulator(3, 8, dev)
        twice("explain targets=%s" % targets, lambda: evaluate.explain(fz, x, targets=targets, acc=acc), acc)

    torch.cuda.synchronize()
    with open(dump, "wb") as fh:
        pickle.dump(out, fh)


def main():
    if args.parent is None:
        sys.exit("eval_totals_ab: --parent DIR (a built checkout of the parent commit) is required")
    sys.exit(ab_trees.report(__file__, ab_trees.child_dumps(__file__, args.parent, args.timeout), args.parent, args.out))


if __name__ == "__main__":
    worker(args.worker, args.dump) if args.worker else main()
