#!/usr/bin/env python3
"""Byte comparison of the three training losses, their monitor and the logits-gradient hand-over against a built checkout of
the parent commit: a tolerance cannot show that a refactor kept the order of the additions, equal bytes can.

    python tools/train_loss_ab.py --parent DIR [--out profiles/train_loss_refactor_ab.txt] [--timeout 300]

DIR is a tree of the parent commit with its library built (``git archive <commit> | tar -x -C DIR && make -C
DIR/bayesian-neural-nets_amd/csrc``).  A fixed list of small cases -- inputs from seeded numpy on the host -- goes through the
public calls (elbo_loss, elbo_bce_loss, elbo_gaussian_loss with and without a TrainMonitor; four small networks for the
hand-over), once with DIR's package and library and once with this tree's, each in a fresh child process under its own time
limit; this process never touches the device (tools/ab_trees.py).  A case is THREE consecutive steps, the middle one
non-finite (kl = inf; without kl an infinite log-probability; a NaN mean for the Gaussian loss): both branches of the
monitor's tail and its ``+=``.  A child dumps the raw bytes of every step's loss and gradients, of ``stats``, and of the
monitor's ``_totals`` and ``_guard``.  The softmax cases and the log_softmax networks run once more in children with
LBBNN_FUSE_LSM_BWD=0.  Per case: ``identical`` or the first key that differs; exit status 1 unless every case is identical."""
import argparse
import os
import pickle
import sys

import ab_trees

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--out", default=os.path.join(ab_trees.HERE, "profiles", "train_loss_refactor_ab.txt"))
ap.add_argument("--timeout", type=int, default=300)
ap.add_argument("--worker", default=None, help="(internal) the tree to import, in a child process")
ap.add_argument("--dump", default=None, help="(internal) where the child leaves its bytes")
ap.add_argument("--only-softmax", action="store_true", help="(internal) the cases that LBBNN_FUSE_LSM_BWD bears on")
args = ap.parse_args()

N_BATCHES = 5.0


def worker(tree, dump, only_softmax):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import bnn_amd
    from bnn_amd import _lib, losses, ops
    assert os.path.abspath(bnn_amd.__file__).startswith(os.path.abspath(tree) + os.sep), bnn_amd.__file__
    dev = torch.device("cuda:0")
    tag = "lsm_bwd=%s " % os.environ.get("LBBNN_FUSE_LSM_BWD", "1")
    out = {}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream

    def keep(case, step, **tensors):
        for k, v in tensors.items():
            if v is not None:
                out["%s #%d/%s" % (case, step, k)] = v.detach().contiguous().cpu().numpy().tobytes()

    def leaf_view(a, wide):
        """``a`` (B, W) on the device as a non-leaf view that keeps its gradient: of a (B, W + wide) leaf when ``wide``."""
        B, W = a.shape
        buf = np.full((B, W + wide), 0.5, np.float32)
        buf[:, :W] = a
        v = up(buf).requires_grad_(True)[:, :W]
        v.retain_grad()
        return v

    def mon_kw(mon):
        return {} if mon is None else {"monitor": mon}

    def mon_state(mon):
        return {} if mon is None else {"_totals": mon._totals, "_guard": mon._guard}

    # ---- softmax: elbo_loss, its two backward launches (the knob picks) and the fused backward's g_logits
    def softmax_case(seed, B, C, wide, with_kl, with_mon):
        case = tag + "softmax B=%d C=%d ld=%d kl=%d monitor=%d" % (B, C, C + wide, with_kl, with_mon)
        rng = np.random.default_rng(seed)
        mon = bnn_amd.TrainMonitor(C, dev) if with_mon else None
        for step in range(3):
            z = rng.standard_normal((B, C)).astype(np.float32)
            z -= np.log(np.exp(z.astype(np.float64)).sum(-1, keepdims=True)).astype(np.float32)
            t = rng.integers(0, C, B).astype(np.int64)
            if B >= 7:                                    # bad targets; a NaN and a -inf beside the target's column
                t[1], t[2] = -1, C
                z[3, (t[3] + 1) % C], z[4, (t[4] + 1) % C] = np.nan, -np.inf
                if C == 1:
                    t[3] = t[4] = -1
            if step == 1 and not with_kl:
                z[0, t[0]] = np.inf
            lp, tt = leaf_view(z, wide), up(t)
            kl = torch.tensor(np.inf if step == 1 else 3.25 + step, device=dev, requires_grad=True) if with_kl else None
            loss = bnn_amd.elbo_loss(lp, tt, kl, N_BATCHES, **mon_kw(mon))
            loss.backward()
            g_logits = torch.empty((B, C), dtype=torch.float32, device=dev)
            g_logp2 = torch.empty((B, C), dtype=torch.float32, device=dev)
            g = torch.ones((), dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().lbbnn_elbo_loss_backward_logits(g.data_ptr(), tt.data_ptr(), lp.data_ptr(), lp.stride(0), B, C,
                                                                  1.0 / N_BATCHES, g_logp2.data_ptr(), g_logits.data_ptr(), None,
                                                                  stream()), "lbbnn_elbo_loss_backward_logits")
            keep(case, step, loss=loss, g_logp=lp.grad, g_kl=None if kl is None else kl.grad, g_logits=g_logits, g_logp2=g_logp2,
                 **mon_state(mon))

    # ---- BCE: elbo_bce_loss with stats, the backward with and without g_logits, the head and its backward
    def bce_case(seed, B, O, wide, with_stats, with_mon):
        case = "bce B=%d O=%d ld=%d stats=%d monitor=%d" % (B, O, O + wide, with_stats, with_mon)
        rng = np.random.default_rng(seed)
        mon = bnn_amd.TrainMonitor(O, dev) if with_mon else None
        stats = torch.zeros(4, dtype=torch.int32, device=dev) if with_stats else None
        for step in range(3):
            x = (2 * rng.standard_normal((B, O))).astype(np.float32)
            p = (1 / (1 + np.exp(-x.astype(np.float64)))).astype(np.float32)
            y = (rng.random((B, O)) > 0.5).astype(np.float32)
            if B * O >= 7:
                y.reshape(-1)[1], y.reshape(-1)[2] = np.nan, 1.5
                p.reshape(-1)[3:7] = (0.0, 1.0, 2e-9, np.nan)
            probs, yy = leaf_view(p, wide), up(y)
            kl = torch.tensor(np.inf if step == 1 else 12.5 + step, device=dev, requires_grad=True)
            loss = bnn_amd.elbo_bce_loss(probs, yy, kl, N_BATCHES, stats=stats, **mon_kw(mon))
            loss.backward()
            g_probs2 = torch.empty((B, O), dtype=torch.float32, device=dev)
            g_logits = torch.empty((B, O), dtype=torch.float32, device=dev)
            g = torch.ones((), dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().lbbnn_elbo_bce_loss_backward(g.data_ptr(), probs.data_ptr(), probs.stride(0) if B > 1 else O,
                                                               yy.data_ptr(), O, B, O, 1.0 / N_BATCHES, g_probs2.data_ptr(),
                                                               g_logits.data_ptr(), None, stream()), "lbbnn_elbo_bce_loss_backward")
            xx = up(x)
            head = ops.binary_head(xx)
            keep(case, step, loss=loss, g_probs=probs.grad, g_kl=kl.grad, g_probs2=g_probs2, g_logits=g_logits, stats=stats,
                 head=head, sigmoid_backward=ops.sigmoid_backward(g_logits, head), **mon_state(mon))

    # ---- Gaussian: elbo_gaussian_loss with a shared (lv_cols through g_lv) and a per-element log-variance
    def gaussian_case(seed, B, O, wide, shared, with_stats, with_mon):
        case = "gaussian B=%d O=%d ld=%d log_var=%s stats=%d monitor=%d" % (B, O, O + wide, "shared" if shared else "element",
                                                                            with_stats, with_mon)
        rng = np.random.default_rng(seed)
        mon = bnn_amd.TrainMonitor(O, dev) if with_mon else None
        stats = torch.zeros(4, dtype=torch.float64, device=dev) if with_stats else None
        for step in range(3):
            m = (2 * rng.standard_normal((B, O))).astype(np.float32)
            y = (m + rng.standard_normal((B, O))).astype(np.float32)
            lv = (-0.5 + 0.5 * rng.standard_normal((O,) if shared else (B, O))).astype(np.float32)
            if B * O >= 7:                                # bad targets; an infinite mean behind one of them
                y.reshape(-1)[1], y.reshape(-1)[2] = np.nan, np.inf
                m.reshape(-1)[1] = np.inf
            if step == 1:
                m.reshape(-1)[0] = np.nan
            mean, yy = leaf_view(m, wide), up(y)
            log_var = up(lv).requires_grad_(True)
            kl = torch.tensor(7.5 + step, device=dev, requires_grad=True)
            loss = bnn_amd.elbo_gaussian_loss(mean, yy, log_var, kl, N_BATCHES, stats=stats, **mon_kw(mon))
            loss.backward()
            keep(case, step, loss=loss, g_mean=mean.grad, g_lv=log_var.grad, g_kl=kl.grad, stats=stats, **mon_state(mon))

    # ---- networks: one seeded forward + backward, every parameter gradient, which way the hand-over went
    def network_case(case, net, loss_of):
        before = dict(losses.HANDOVER)
        bnn_amd.manual_seed(5)
        loss, extra = loss_of(net)
        loss.backward()
        keep(case, 0, loss=loss, handover=torch.tensor([losses.HANDOVER[k] - before[k] for k in sorted(before)]),
             **{"grad_" + k: p.grad for k, p in net.named_parameters()}, **extra)

    seed = 0
    for B in (1, 7, 1023, 1024, 1025, 2500):
        for C in (1, 2, 10, 16, 17, 64):
            for wide in (0, 3):
                for with_kl in (1, 0):
                    for with_mon in (1, 0):
                        seed += 1
                        softmax_case(seed, B, C, wide, with_kl, with_mon)
    rng = np.random.default_rng(5000)
    torch.manual_seed(0)
    net = bnn_amd.lrt.BayesianNetwork((12, 8, 3)).to(dev).train()
    x, t = up(rng.random((70, 12)).astype(np.float32)), up(rng.integers(0, 3, 70).astype(np.int64))
    network_case(tag + "network lrt 12-8-3 log_softmax", net, lambda n: (bnn_amd.elbo_loss(n(x, sample=True), t, n.kl(), N_BATCHES), {}))
    torch.manual_seed(0)
    net = bnn_amd.base.BayesianNetwork((12, 16, 3)).to(dev).train()
    x = up(rng.standard_normal((70, 12)).astype(np.float32))
    mon = bnn_amd.TrainMonitor(3, dev)
    network_case(tag + "network base 12-16-3 sample_elbo(monitor=)", net,
                 lambda n: (n.sample_elbo(x, t, draws="hip", num_batches=N_BATCHES, monitor=mon)[0], mon_state(mon)))
    torch.manual_seed(0)
    net = bnn_amd.vd.BNN((8, 6, 3)).to(dev)
    x, t = up(rng.random((5, 8)).astype(np.float32)), up(rng.integers(0, 3, 5).astype(np.int64))
    mon = bnn_amd.TrainMonitor(3, dev)
    network_case(tag + "network vd 8-6-3 loss_fn(monitor=)", net,
                 lambda n: (bnn_amd.vd.loss_fn(n(x), t, n, num_batches=N_BATCHES, monitor=mon), mon_state(mon)))

    if not only_softmax:
        for B, O in [(B, O) for B in (1, 7, 400) for O in (1, 3, 16)] + [(342, 3)]:          # 342 * 3 = 1026: past the stride
            for wide in (0, 2):
                for with_stats in (1, 0):
                    for with_mon in (1, 0):
                        seed += 1
                        bce_case(seed, B, O, wide, with_stats, with_mon)
        for O in (1, 3, 7, 16):
            for B in (1, 7, 400):
                for wide in (0, 2):
                    for shared in (1, 0):
                        for with_stats in (1, 0):
                            for with_mon in (1, 0):
                                seed += 1
                                gaussian_case(seed, B, O, wide, shared, with_stats, with_mon)
        torch.manual_seed(0)
        net = bnn_amd.lrt.BayesianNetwork((20, 1), head="sigmoid").to(dev).train()
        x, y = up(rng.random((7, 20)).astype(np.float32)), up((rng.random((7, 1)) > 0.5).astype(np.float32))
        network_case("network lrt 20-1 sigmoid", net, lambda n: (bnn_amd.elbo_bce_loss(n(x, sample=True), y, n.kl(), N_BATCHES), {}))
        torch.manual_seed(0)
        net = bnn_amd.base.BayesianNetwork((8, 1), head="sigmoid").to(dev).train()
        x, y = up(rng.standard_normal((5, 8)).astype(np.float32)), up((rng.random((5, 1)) > 0.5).astype(np.float32))
        mon = bnn_amd.TrainMonitor(1, dev)
        network_case("network base 8-1 sigmoid sample_elbo(monitor=)", net,
                     lambda n: (n.sample_elbo(x, y, draws="hip", num_batches=N_BATCHES, monitor=mon)[0], mon_state(mon)))

    torch.cuda.synchronize()
    with open(dump, "wb") as fh:
        pickle.dump(out, fh)


def main():
    if args.parent is None:
        sys.exit("train_loss_ab: --parent DIR (a built checkout of the parent commit) is required")
    dumps = ab_trees.child_dumps(__file__, args.parent, args.timeout)
    knob = ab_trees.child_dumps(__file__, args.parent, args.timeout, extra=("--only-softmax",), env={"LBBNN_FUSE_LSM_BWD": "0"})
    for name in dumps:
        dumps[name].update(knob[name])
    sys.exit(ab_trees.report(__file__, dumps, args.parent, args.out))


if __name__ == "__main__":
    worker(args.worker, args.dump, args.only_softmax) if args.worker else main()
