"""Cases of the coupling-flow (RNVP / MNF-type) edge tests, shared by tests/test_dense_flow_edges_gpu.py and
tests/test_dense_flow_edges_host.py: an ``mnf.BayesianLinear`` / ``mnf.BayesianNetwork`` whose flows are swapped for chains
of any length, kind and hidden width H (``flows.RNVP(I, h_sizes=(H,)*4)``, ``flows.MNF(I, hidden=H)`` -- the layer has no
keyword for the width), explicit noise and Bernoulli(0.5) masks from a seeded CPU generator, and the reference: the oracle
(``orc.flow_from_state`` + ``orc.mnf_forward`` / ``orc.mnf_network_forward``) under autograd, in float64 (or float32 for the
rehearsal of the host tier).  Everything here runs on the CPU; only ``to_device`` touches a HIP device."""
import torch
import torch.nn as nn

from oracle import lbbnn_oracle as orc

TOL = 1e-4           # outputs, KL, x.grad (the contract)
PTOL = 5e-4          # parameter gradients (test_dense_flow_hip_backward_vs_oracle_autograd)
HIDDEN_SWEEP = (1, 2, 17, 63, 64, 65, 76, 78, 79, 110, 111, 128)


def make_flow(bnn, kind, I, H, T):
    """PropagateFlow(kind, I, ·) with T transforms of hidden width H."""
    flow = bnn.flows.PropagateFlow(kind, I, 0)
    make = (lambda: bnn.flows.RNVP(I, h_sizes=(H,) * 4)) if kind == "RNVP" else (lambda: bnn.flows.MNF(I, hidden=H))
    flow.transforms = nn.ModuleList([make() for _ in range(T)])
    return flow


def make_layer(bnn, I, O, H, zk, rk, Tz, Tr, seed=21):
    """CPU layer as test_dense_flow_hip_backward_vs_oracle_autograd conditions it: q0_mean around 1, weight_mu x 10."""
    torch.manual_seed(seed)
    layer = bnn.mnf.BayesianLinear(I, O, 0, z_flow_type=zk, r_flow_type=rk)
    layer.z_flow.transforms = make_flow(bnn, zk, I, H, Tz).transforms
    layer.r_flow.transforms = make_flow(bnn, rk, I, H, Tr).transforms
    with torch.no_grad():
        layer.q0_mean.add_(1.0)
        layer.weight_mu.mul_(10)
    return layer


def make_network(bnn, dims, H, kinds, T, seed=41):
    """mnf.BayesianNetwork(dims) whose layer k has flows of kind kinds[k] and width H[k] (T transforms each)."""
    torch.manual_seed(seed)
    net = bnn.mnf.BayesianNetwork(dims, 0, z_flow_type="RNVP", r_flow_type="RNVP")
    for l, h, kind in zip(net._layers(), H, kinds):
        l.z_flow = make_flow(bnn, kind, l.in_features, h, T)
        l.r_flow = make_flow(bnn, kind, l.in_features, h, T)
        with torch.no_grad():
            l.q0_mean.add_(1.0)
            l.weight_mu.mul_(10)
    return net


def draw_masks(g, I, T):
    """T Bernoulli(0.5) masks (I,).  For I <= 2 a list is drawn again until it holds both a 0 and a 1 (where its T * I
    elements allow that): a mask list of all ones never moves z, one of all zeros never feeds the coupling network."""
    while True:
        ms = [torch.bernoulli(torch.full((I,), 0.5), generator=g) for _ in range(T)]
        if I > 2 or T * I < 2:
            return ms
        flat = torch.cat(ms)
        if bool((flat == 0).any()) and bool((flat == 1).any()):
            return ms


def make_noise(g, B, I, O, Tz, Tr):
    """Every draw of one training forward, in the shapes layer.noise takes (the draw order of the existing test)."""
    n = {"eps_z": torch.randn(1, I, generator=g), "eps_out": torch.randn(B, O, generator=g),
         "eps_z2": torch.randn(1, I, generator=g), "eps_act": torch.randn(O, generator=g)}
    n["zmask"] = draw_masks(g, I, Tz)
    n["zmask2"] = draw_masks(g, I, Tz)
    n["rmask"] = draw_masks(g, I, Tr)
    return n


def to_device(noise, dev):
    return {k: ([m.to(dev) for m in v] if isinstance(v, list) else v.to(dev)) for k, v in noise.items()}


def _cast(noise, dtype):
    return {k: ([m.to(dtype) for m in v] if isinstance(v, list) else v.to(dtype)) for k, v in noise.items()}


def layer_loss(out, kl):
    return out.pow(2).sum() + kl / 60


def reference_layer(state, x, noise, zk, rk, Tz, Tr, *, train=True, dtype=torch.float64):
    """The oracle layer under autograd in ``dtype``: {'out', 'kl', 'x', name: gradient or None}.  ``train=False`` is the
    eval-mode forward with sample=True: no KL branch, loss = out^2 summed."""
    pc = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in state.items()}
    xc = x.detach().clone().to(dtype).requires_grad_(True)
    zf = orc.flow_from_state("z_flow", zk, pc, Tz)
    rf = orc.flow_from_state("r_flow", rk, pc, Tr)
    o, kl, _ = orc.mnf_forward(xc, pc, zf, rf, _cast(noise, dtype), compute_kl=train)
    (layer_loss(o, kl) if train else o.pow(2).sum()).backward()
    res = {"out": o.detach(), "kl": kl.detach() if train else None, "x": xc.grad}
    res.update({k: v.grad for k, v in pc.items()})
    return res


def reference_network(states, x, noises, kinds, T, *, dtype=torch.float64):
    """The oracle network (ReLU between the layers, log_softmax after the last) under autograd; loss as layer_loss.
    Returns {'out', 'kl', 'x', 'l<k>.<name>': gradient or None}."""
    P = [{k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()} for sd in states]
    xc = x.detach().clone().to(dtype).requires_grad_(True)
    zf = [orc.flow_from_state("z_flow", kind, p, T) for kind, p in zip(kinds, P)]
    rf = [orc.flow_from_state("r_flow", kind, p, T) for kind, p in zip(kinds, P)]
    o, kl = orc.mnf_network_forward(xc, P, zf, rf, [_cast(n, dtype) for n in noises])
    layer_loss(o, kl).backward()
    res = {"out": o.detach(), "kl": kl.detach(), "x": xc.grad}
    for i, p in enumerate(P):
        res.update({"l%d.%s" % (i + 1, k): v.grad for k, v in p.items()})
    return res


def rel(a, b):
    """max|a-b| / max|b| (conftest.rel_err) without importing conftest from a helper."""
    a = torch.as_tensor(a, dtype=torch.float64).cpu()
    b = torch.as_tensor(b, dtype=torch.float64).cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def compare(got, ref, worst=None, tol=TOL, ptol=PTOL):
    """``got`` / ``ref``: dicts as reference_layer returns them.  Asserts the bars; a reference gradient that is None or
    exactly zero wants ours None or zero.  ``worst``: a dict that collects the largest error per class of quantity."""
    errs = {"out": rel(got["out"], ref["out"]), "x": rel(got["x"], ref["x"])}
    if ref.get("kl") is not None:
        errs["kl"] = abs(float(got["kl"]) - float(ref["kl"])) / abs(float(ref["kl"]))
    perr = {}
    for name, r in ref.items():
        if name in ("out", "kl", "x"):
            continue
        g = got.get(name)
        if r is None or float(r.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) < 1e-12, name
            continue
        assert g is not None, name
        perr[name] = rel(g, r)
    if worst is not None:
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if perr:
            k = max(perr, key=perr.get)
            if perr[k] >= worst.get("param", (0.0, ""))[0]:
                worst["param"] = (perr[k], k)
    print("errors:", {k: "%.3g" % v for k, v in errs.items()},
          "param worst: %s" % (max(perr.items(), key=lambda kv: kv[1]),) if perr else "")
    for k, v in errs.items():
        assert v < tol, (k, v)
    for k, v in perr.items():
        assert v < ptol, (k, v)
    return errs, perr
