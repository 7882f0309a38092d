"""GPU tier: the coupling-flow (RNVP / MNF-type) kernels away from the hidden widths 75 and 100 of the reference.

The five HIP files that carry these flows branch on the hidden width H, the vector length I and the chain lengths
(DESIGN.md 7.16): H <= 64 | > 64 (column halves), odd / even k split and the four tails of the 4-unrolled middle dot, a
second LDS copy round from H = 79, the dynamic-LDS opt-in from H = 65, the global-memory walk from H = 111, H = 128 = HMAX;
workgroup tails of 64 / 16 / 64 elements of I, the 16-at-a-time partial sum (nwg = 16, 17); the ping-pong of the partial
buffers across the z and r phases (odd Tz), mixed kinds in one layer, Tz or Tr = 0, eight mask bits per Philox word.  Every
case compares outputs, KL, x.grad and every parameter gradient with the fp64 oracle under autograd (tests/dense_flow_cases.py;
loss = out^2 summed + KL / 60) on explicit noise and masks:

  a  hidden-width sweep, one layer, forward + lbbnn_mnf_flow_dense_backward (the default mode)
  b  the same, lbbnn_flow_dense_apply[_backward] (single workgroup)
  c  vector-length sweep
  d  chain lengths and kinds, both modes, one case in eval mode with sample=True
  e  two networks in one batched launch each: per-layer H = (17, 128, 64) and (17, 64, 64), kinds (RNVP, MNF, RNVP)
  f  in-kernel draws at Tz = Tr = 8: the HIP backward against the torch chain on the same seeds
  g  the MFMA row kernel lbbnn_flow_dense_rows on explicit masks
  h  the members kernel through freeze(dense=True).ensemble

Bars (the project's own for these kernels, unchanged): 1e-4 on outputs, KL and x.grad, 5e-4 on parameter gradients (a-f);
g: 2e-5 on z and 5e-5 on the log-determinant (test_flow_dense_rows_in_kernel_masks_vs_oracle); h: 5e-6 on z
(test_member_z_against_fp64, layers of at most 784 inputs).  The fp32 rounding of the reference itself is 40 times below the
bars of a-f (tests/test_dense_flow_edges_host.py).  A reference gradient that is None or exactly zero wants ours None or
zero.

What the Python boundary refuses instead of computing (asserted here): a row-kernel chain of 9 transforms (RuntimeError,
LBBNN_E_SHAPE from lbbnn_flow_dense_rows, nothing launched), a row length above lbbnn_flow_dense_rows_max_dim()
(RuntimeError before the call) and H = 129 (ValueError of flows.dense_hidden: from freeze(dense=True) AND from the loop form
-- no forward of this library takes a coupling network wider than LBBNN_MAX_HIDDEN, so there is no fallback that could be
compared with the oracle).  Every combination of d, Tz = 0 and Tr = 0 included, is computed.

Worst errors measured on an MI355X (profiles/dense_flow_edges.txt; outputs / KL / x.grad / worst parameter gradient):
  a  1.7e-7 / 7.4e-8 / 2.1e-7 / 3.2e-6        b  1.7e-7 / 7.2e-8 / 2.1e-7 / 7.0e-6        c  1.6e-7 / 1.3e-7 / 3.5e-7 / 6.8e-6
  d  1.4e-7 / 4.0e-8 / 2.6e-7 / 7.1e-6        e  1.0e-7 / 9.3e-9 / 1.9e-6 / 1.6e-6        f  0 / 0 / 9.5e-8 / 1.9e-5
  g  z 3.0e-7, log-det 1.0e-7                 h  z 1.4e-7
All sit at the rounding of the fp32 arithmetic, far under the bars; the bars are kept.  Before its fix in flow_dense.hip the
case (RNVP, RNVP, Tz = 0, Tr = 2) of d missed them in the single-workgroup mode: KL 1.2e-4, r0_b1 gradient 0.85."""
import pytest
import torch

import dense_flow_cases as dfc
import philox_ref
from conftest import rel_err
from dense_flow_cases import PTOL, TOL
from oracle import lbbnn_oracle as orc
from philox_bits_ref import mask_bits

pytestmark = pytest.mark.gpu

ROWS_Z, ROWS_LD = 2e-5, 5e-5        # group g
MEMBER_Z = 5e-6                     # group h

_REF = {}                           # fp64 references, computed once per case and shared by the modes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _set_mode(monkeypatch, mode):
    from bnn_amd import _grad, layers
    monkeypatch.setattr(layers, "_DENSE_HIP_BWD", mode == "layer_hip")
    monkeypatch.setattr(_grad, "_DENSE_HIP", mode == "single_wg")


def _layer_case(bnn, dev, group, I, O, B, H, zk, rk, Tz, Tr, train=True):
    """One layer on explicit noise: forward, KL and backward on the device against the fp64 oracle."""
    layer = dfc.make_layer(bnn, I, O, H, zk, rk, Tz, Tr)
    key = (I, O, B, H, zk, rk, Tz, Tr, train)
    if key not in _REF:
        g = torch.Generator().manual_seed(22)
        noise = dfc.make_noise(g, B, I, O, Tz, Tr)
        x = torch.rand(B, I, generator=g)
        state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
        _REF[key] = (noise, x, dfc.reference_layer(state, x, noise, zk, rk, Tz, Tr, train=train))
    noise, x, ref = _REF[key]
    layer = layer.to(dev).train(train)
    layer.noise = dfc.to_device(noise, dev)
    xg = x.to(dev).requires_grad_(True)
    out = layer(xg, sample=True)
    (dfc.layer_loss(out, layer.kl) if train else out.pow(2).sum()).backward()
    got = {"out": out.detach(), "kl": layer.kl.detach() if train else None, "x": xg.grad}
    got.update({n: p.grad for n, p in layer.named_parameters()})
    print("dense-edges group %s case %s" % (group, key))
    return dfc.compare(got, ref)


# ----------------------------------------------------------------------------------------- a / b: hidden-width sweeps
@pytest.mark.parametrize("kind", ["RNVP", "MNF"])
@pytest.mark.parametrize("H", dfc.HIDDEN_SWEEP)
def test_a_hidden_width_sweep_layer_backward(bnn, dev, monkeypatch, H, kind):
    _set_mode(monkeypatch, "layer_hip")
    _layer_case(bnn, dev, "a", 65, 5, 4, H, kind, kind, 2, 2)


@pytest.mark.parametrize("kind", ["RNVP", "MNF"])
@pytest.mark.parametrize("H", [1, 17, 64, 65, 111, 128])
def test_b_hidden_width_sweep_single_workgroup(bnn, dev, monkeypatch, H, kind):
    _set_mode(monkeypatch, "single_wg")
    _layer_case(bnn, dev, "b", 65, 5, 4, H, kind, kind, 2, 2)


# ----------------------------------------------------------------------------------------- c: vector lengths
@pytest.mark.parametrize("kind", ["RNVP", "MNF"])
@pytest.mark.parametrize("I", [1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 1024, 1025])
def test_c_vector_length_sweep(bnn, dev, monkeypatch, I, kind):
    _set_mode(monkeypatch, "layer_hip")
    _layer_case(bnn, dev, "c", I, 3, 3, 17, kind, kind, 2, 2)


# ----------------------------------------------------------------------------------------- d: chain lengths and kinds
CHAINS = [("RNVP", "MNF", 3, 1, True), ("MNF", "RNVP", 1, 3, True), ("RNVP", "RNVP", 8, 8, True), ("MNF", "MNF", 8, 8, True),
          ("RNVP", "RNVP", 0, 2, True), ("RNVP", "RNVP", 2, 0, True), ("RNVP", "MNF", 3, 1, False)]


@pytest.mark.parametrize("mode", ["layer_hip", "single_wg"])
@pytest.mark.parametrize("zk,rk,Tz,Tr,train", CHAINS, ids=["%s%d-%s%d-%s" % (c[0], c[2], c[1], c[3], "train" if c[4] else "eval")
                                                         for c in CHAINS])
def test_d_chain_lengths_and_kinds(bnn, dev, monkeypatch, zk, rk, Tz, Tr, train, mode):
    """train=False: eval mode with sample=True -- no KL branch, every r-flow / r0 gradient zero or None."""
    _set_mode(monkeypatch, mode)
    _layer_case(bnn, dev, "d", 65, 5, 4, 17, zk, rk, Tz, Tr, train=train)


# ----------------------------------------------------------------------------------------- e: heterogeneous batched launch
NET_DIMS, NET_KINDS, NET_T, NET_B = (129, 16, 65, 10), ("RNVP", "MNF", "RNVP"), 2, 4


def _net_grads(net, xg, out, kl):
    dfc.layer_loss(out, kl).backward()
    got = {"out": out.detach().clone(), "kl": kl.detach().clone(), "x": xg.grad.clone()}
    got.update({n: (p.grad.clone() if p.grad is not None else None) for n, p in net.named_parameters()})
    return got


@pytest.mark.parametrize("H", [(17, 128, 64), (17, 64, 64)], ids=["wide-neighbour", "all-le-64"])
def test_e_network_of_mixed_widths_and_kinds_in_one_batched_launch(bnn, dev, monkeypatch, H):
    """maxH of the batched launch decides the branch for every layer: with (17, 128, 64) the H = 17 RNVP layer walks global
    memory beside its wide neighbour, with (17, 64, 64) the three matrices take exactly 48 KB of LDS and nothing is opted in.
    The network path (all layers' flows in one launch sequence) against the oracle network, and against the same layers
    called one by one on the same noise: the two agree to TOL / PTOL, and when run on an MI355X they were NOT bitwise equal
    (see profiles/dense_flow_edges.txt), so that is what is asserted."""
    _set_mode(monkeypatch, "layer_hip")
    net = dfc.make_network(bnn, NET_DIMS, H, NET_KINDS, NET_T)
    layers = net._layers()
    key = ("net", H)
    if key not in _REF:
        g = torch.Generator().manual_seed(42)
        x = torch.rand(NET_B, NET_DIMS[0], generator=g)
        noises = [dfc.make_noise(g, NET_B, l.in_features, l.out_features, NET_T, NET_T) for l in layers]
        states = [{k: v.detach().clone() for k, v in l.state_dict().items()} for l in layers]
        _REF[key] = (x, noises, dfc.reference_network(states, x, noises, NET_KINDS, NET_T))
    x, noises, ref = _REF[key]
    net = net.to(dev).train()
    for l, n in zip(layers, noises):
        l.noise = dfc.to_device(n, dev)
    xg = x.to(dev).requires_grad_(True)
    out = net(xg, sample=True)
    got = _net_grads(net, xg, out, net.kl())
    print("dense-edges group e case network %s against the oracle" % (H,))
    dfc.compare(got, ref)
    # the same layers one by one
    net.zero_grad(set_to_none=True)
    xg = x.to(dev).requires_grad_(True)
    h, kl = xg, 0
    for i, l in enumerate(layers):
        h = l(h, sample=True)
        kl = kl + l.kl
        if i < len(layers) - 1:
            h = torch.relu(h)
    one = _net_grads(net, xg, torch.log_softmax(h, dim=1), kl)
    bitwise = all((got[k] is None) == (one[k] is None) and (got[k] is None or torch.equal(got[k], one[k])) for k in got)
    print("dense-edges group e case network %s against its layers one by one (bitwise equal: %s)" % (H, bitwise))
    dfc.compare(got, one)


# ----------------------------------------------------------------------------------------- f: in-kernel draws
def test_f_in_kernel_draws_eight_transforms(bnn, dev, monkeypatch):
    """Eight mask bits per Philox word are the most the row kernels allow; here the training path draws eight per flow.
    lbbnn_mnf_flow_dense_backward (draws re-created in the kernel) against the torch chain on the same seeds."""
    from bnn_amd import _grad, layers
    monkeypatch.setattr(_grad, "_DENSE_HIP", False)
    B, I, O, H, T = 4, 65, 5, 17, 8
    layer = dfc.make_layer(bnn, I, O, H, "RNVP", "RNVP", T, T).to(dev).train()
    x = torch.rand(B, I, generator=torch.Generator().manual_seed(5)).to(dev)
    res = {}
    for mode in ("hip", "torch"):
        monkeypatch.setattr(layers, "_DENSE_HIP_BWD", mode == "hip")
        bnn.manual_seed(77, 3)
        layer.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        out = layer(xg, sample=True)
        dfc.layer_loss(out, layer.kl).backward()
        res[mode] = {"out": out.detach().clone(), "kl": layer.kl.detach().clone(), "x": xg.grad.clone(),
                     **{n: (p.grad.clone() if p.grad is not None else None) for n, p in layer.named_parameters()}}
    print("dense-edges group f case in-kernel T=8")
    dfc.compare(res["hip"], res["torch"])


# ----------------------------------------------------------------------------------------- g: the row kernel
def _row_masks(g, T, R, I):
    while True:
        ms = [torch.bernoulli(torch.full((R, I), 0.5), generator=g) for _ in range(T)]
        if R * I > 2:
            return ms
        if T * R * I == 1:
            return [torch.zeros(R, I)]                    # the one element moves: the transform is exercised
        flat = torch.cat([m.reshape(-1) for m in ms])
        if bool((flat == 0).any()) and bool((flat == 1).any()):
            return ms


def _rows_case(bnn, dev, kind, R, I, H, T):
    torch.manual_seed(3)
    flow = dfc.make_flow(bnn, kind, I, H, T)
    with torch.no_grad():
        for p in flow.parameters():
            p.requires_grad_(False)                       # evaluation: the one-launch row kernel
            if p.dim() == 2:
                p.mul_(1.5)                               # gates away from 0.5, log-dets of useful size
    g = torch.Generator().manual_seed(4)
    z = torch.randn(R, I, generator=g)
    masks = _row_masks(g, T, R, I)
    sd = {"x." + k: v.detach().double() for k, v in flow.state_dict().items()}
    flow = flow.to(dev)
    flow.masks = [m.to(dev) for m in masks]
    return flow, z, masks, sd


@pytest.mark.parametrize("kind", ["RNVP", "MNF"])
@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("R,I,H", [(1, 1, 1), (17, 65, 17), (16, 64, 76), (33, 130, 128), (5, 7, 111)])
def test_g_row_kernel_explicit_masks_vs_oracle(bnn, dev, R, I, H, T, kind):
    flow, z, masks, sd = _rows_case(bnn, dev, kind, R, I, H, T)
    out, ld = flow(z.to(dev))
    ref_z, ref_ld = orc.flow_from_state("x", kind, sd, T).run(z.double(), [m.double() for m in masks])
    ez, el = rel_err(out, ref_z), rel_err(ld, ref_ld)
    print("dense-edges group g case %s errors: z %.3g logdet %.3g" % ((kind, R, I, H, T), ez, el))
    assert not out.requires_grad and out.shape == (R, I) and ld.shape == ref_ld.shape
    assert ez < ROWS_Z and el < ROWS_LD


@pytest.mark.parametrize("kind", ["RNVP", "MNF"])
def test_g_row_kernel_at_the_longest_row(bnn, dev, kind):
    from bnn_amd import _lib
    I = int(_lib.lib().lbbnn_flow_dense_rows_max_dim())
    R, H, T = 17, 128, 1
    flow, z, masks, sd = _rows_case(bnn, dev, kind, R, I, H, T)
    out, ld = flow(z.to(dev))
    ref_z, ref_ld = orc.flow_from_state("x", kind, sd, T).run(z.double(), [m.double() for m in masks])
    ez, el = rel_err(out, ref_z), rel_err(ld, ref_ld)
    print("dense-edges group g case %s errors: z %.3g logdet %.3g" % ((kind, R, I, H, T), ez, el))
    assert ez < ROWS_Z and el < ROWS_LD


def test_g_row_kernel_refuses_nine_transforms_and_longer_rows(bnn, dev):
    """Pinned: both are clear exceptions before a launch -- never numbers that could disagree with the oracle."""
    from bnn_amd import _lib
    flow, z, _, _ = _rows_case(bnn, dev, "RNVP", 3, 65, 17, _lib.MAX_DENSE_T + 1)
    with pytest.raises(RuntimeError, match=r"lbbnn_flow_dense_rows failed \(-2\)"):
        flow(z.to(dev))
    I = int(_lib.lib().lbbnn_flow_dense_rows_max_dim()) + 1
    flow, z, _, _ = _rows_case(bnn, dev, "MNF", 2, I, 4, 1)
    with pytest.raises(RuntimeError, match=r"dim %d exceeds the limit %d" % (I, I - 1)):
        flow(z.to(dev))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------- h: the members kernel
SEED, OFF, MEMBERS = 3, 5, 5


def _members_net(bnn, dims, kind, H, T=2):
    torch.manual_seed(11)
    net = bnn.mnf.BayesianNetwork(dims, 0, z_flow_type=kind, r_flow_type=kind)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for l in net._layers():
            O, I = l.out_features, l.in_features
            l.z_flow = dfc.make_flow(bnn, kind, I, H, T)
            l.r_flow = dfc.make_flow(bnn, kind, I, H, T)
            l.lambdal.copy_(2.0 * torch.randn(O, I, generator=g))
            l.q0_mean.copy_(1.0 + 0.1 * torch.randn(I, generator=g))          # z around 1 with a visible draw, as
            l.q0_log_var.copy_(-6.0 + 0.5 * torch.randn(I, generator=g))      # tests/test_frozen_dense_gpu.py
    return net


@pytest.mark.parametrize("kind", ["RNVP", "MNF"])
@pytest.mark.parametrize("H", [16, 17, 128])
@pytest.mark.parametrize("dims", [(64, 16, 10), (132, 68, 10)], ids=["64-16-10", "132-68-10"])
def test_h_member_z_against_fp64(bnn, dev, dims, H, kind):
    T = 2
    net = _members_net(bnn, dims, kind, H, T)
    P = [{k: v.detach().double() for k, v in l.state_dict().items()} for l in net._layers()]
    net = net.to(dev).eval()
    fz = bnn.evaluate.freeze(net, "alpha", dense=True)
    x = torch.rand(1, dims[0], generator=torch.Generator().manual_seed(1)).to(dev)
    bnn.manual_seed(SEED, OFF)
    out = fz.ensemble(x, MEMBERS, keep_z=True)
    assert out.shape == (MEMBERS, 1, dims[-1]) and int(bnn.ops.RngState.get(dev).t[1]) == OFF + MEMBERS
    worst = 0.0
    for m in range(MEMBERS):
        for i, (l, p) in enumerate(zip(net._layers(), P)):
            I = l.in_features
            eps = torch.from_numpy(philox_ref.normal_vector(SEED, OFF + m, bnn.ops.STREAM_EPS_Z * 64 + l._layer_id, I))
            mk = torch.from_numpy(mask_bits(SEED, OFF + m, l._layer_id, I, T))
            z, _, _ = orc.mnf_sample_z(p, eps.double().reshape(1, I), orc.flow_from_state("z_flow", kind, p, T),
                                       [r.double().reshape(1, I) for r in mk])
            e = rel_err(fz.last_z[i][m], z)
            worst = max(worst, e)
            assert e < MEMBER_Z, (m, i, e)
    print("dense-edges group h case %s errors: z %.3g" % ((kind, dims, H), worst))


@pytest.mark.parametrize("kind", ["RNVP", "MNF"])
def test_h_hidden_129_is_refused_by_the_frozen_model_and_by_the_loop(bnn, dev, kind):
    """No forward takes H = 129 (the single forward's kernels hold HMAX = 128 units as the member kernel does), so the loop
    form that freeze() names for other refusals refuses it too: a ValueError before any launch, the Philox offset unmoved."""
    net = _members_net(bnn, (64, 16, 10), kind, 129).to(dev).eval()
    x = torch.rand(1, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    bnn.manual_seed(SEED, OFF)
    with pytest.raises(ValueError, match=r"layer 1: z_flow.*129"):
        bnn.evaluate.freeze(net, "alpha", dense=True)
    with pytest.raises(ValueError, match=r"layer 1: z_flow.*129"):
        bnn.evaluate.ensemble_forward(net, x, MEMBERS, batched=True)
    with pytest.raises(ValueError, match="129"):
        bnn.evaluate.ensemble_forward(net, x, MEMBERS)
    assert int(bnn.ops.RngState.get(dev).t[1]) == OFF
    torch.cuda.synchronize()
