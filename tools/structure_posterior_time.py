#!/usr/bin/env python3
"""Time of evaluate.structure_posterior (one lbbnn_gate_structure launch for all samples) against the torch spelling of the
same numbers, one process: S in {10, 100, 1000} on 784-1200-1200-10 and 784-400-600-10 (LRT networks as constructed, lambdal ~
U(0, 1)).

  kernel    structure_posterior(net, S, rng=state): the call as a user makes it, its output tensors and fp64 divisions included
  torch     per sample: torch.bernoulli(alpha) of every layer, then the backward `any` sweep of evaluate.live_structure
            and the counts, all on the device, no host read (alpha = sigmoid(lambdal) taken once outside the timed part).  It
            draws from torch's generator, so its numbers are another sample of the same distribution, not the same bits.

The forms alternate; each is timed --repeats times as a window of calls between two device events after a warm-up of all, and
reported as fastest window [slowest window] in ms per call.  The torch spelling at S = 1000 takes --torch-calls calls per window.  The table goes to
stdout and to --out (default profiles/structure_posterior.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bnn_amd
from bnn_amd import evaluate

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20, help="calls per window")
ap.add_argument("--torch-calls", type=int, default=2, help="calls per window of the torch spelling at S = 1000")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_posterior.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("structure_posterior_time: needs a HIP device (no CPU path, no CPU timing)")

dev = torch.device("cuda:0")


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def torch_spelling(alphas, S):
    """kept, needed, active_kept and the feature counts of S structures, spelled in torch on the device."""
    n = len(alphas)
    kept = torch.empty((S, n), dtype=torch.int64, device=dev)
    active = torch.empty((S, n), dtype=torch.int64, device=dev)
    needed = torch.empty((S, n + 1), dtype=torch.int64, device=dev)
    feature_count = torch.zeros(alphas[0].shape[1], dtype=torch.int64, device=dev)
    for s in range(S):
        gates = [torch.bernoulli(a).bool() for a in alphas]
        need = torch.ones(alphas[-1].shape[0], dtype=torch.bool, device=dev)
        needed[s, n] = need.sum()
        for l in range(n - 1, -1, -1):
            live = gates[l] & need[:, None]
            kept[s, l] = gates[l].sum()
            active[s, l] = live.sum()
            need = live.any(0)
            needed[s, l] = need.sum()
        feature_count += need
    return kept, needed, active, feature_count


lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("evaluate.structure_posterior against its torch spelling; per form %d windows (ms per call: fastest [slowest]), the forms "
    "alternating, after %d warm-up calls of each; %d calls per window (torch at S = 1000: %d)"
    % (args.repeats, args.warmup, args.calls, args.torch_calls))
say("device: %s" % torch.cuda.get_device_name(0))
for dims in ((784, 1200, 1200, 10), (784, 400, 600, 10)):
    torch.manual_seed(0)
    net = bnn_amd.lrt.BayesianNetwork(dims).to(dev).eval()
    alphas = [torch.sigmoid(l.lambdal.detach()) for l in net._layers()]
    weights = sum(a.numel() for a in alphas)
    state = torch.tensor([1, 0], dtype=torch.int64, device=dev)
    for S in (10, 100, 1000):
        f_kernel = lambda: evaluate.structure_posterior(net, S, rng=state)
        f_torch = lambda: torch_spelling(alphas, S)
        a = f_kernel()
        t = torch_spelling(alphas, min(S, 100))
        forms = (("kernel", f_kernel, args.calls),
                 ("torch", f_torch, args.torch_calls if S >= 1000 else max(1, args.calls // (1 if S < 100 else 4))))
        for _ in range(args.warmup):
            for name, fn, _ in forms:
                if name != "torch" or S < 1000:
                    fn()
        times = dict((name, []) for name, _, _ in forms)
        for _ in range(args.repeats):
            for name, fn, calls in forms:
                times[name].append(window(fn, calls))
        fmt = lambda v: "%.4f [%.4f]" % (min(v), max(v))
        say("%-16s S=%-5d kernel %s  torch %s  torch/kernel %.1fx"
            % ("-".join(map(str, dims)), S, fmt(times["kernel"]), fmt(times["torch"]), min(times["torch"]) / min(times["kernel"])))
        if S == 1000:
            say("%-16s          %.0f weights: %.2f G gate draws per call, kernel %.1f G draws / s; mean density kernel %.4f, torch "
                "(S = 100) %.4f, mean alpha %.4f" % ("", weights, weights * S / 1e9, weights * S / 1e6 / min(times["kernel"]),
                                                  float(a["density"].mean()), float(t[0].sum(1).double().mean()) / weights,
                                                  float(torch.cat([x.reshape(-1) for x in alphas]).double().mean())))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
