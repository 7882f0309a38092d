"""CPU tier of the coupling-flow edge tests (tests/test_dense_flow_edges_gpu.py).

1. Widths the HIP kernels cannot take are refused with a ValueError that names them (``flows.dense_hidden``): an RNVP
   whose four hidden layers differ (``h_sizes=(75, 50, 60, 75)``: the kernels read ONE width and three "H x H" matrices),
   a list of another length than 4, and widths above ``_lib.MAX_HIDDEN`` (RNVP ``h_sizes`` and MNF ``hidden``).  The paths
   that refuse, each before anything is launched: ``PropagateFlow.dense_descs`` (through it the layer's training forward
   and backward in layers.py, the stand-alone row-kernel forward and ``sample_z``), ``_grad._dense_hip`` /
   ``_grad._dense_descs`` (lbbnn_flow_dense_apply[_backward]) and ``evaluate.freeze(dense=True)`` (through it the batched
   ensemble).  The torch formulas of ``_grad._dense`` (the chain's backward under LBBNN_DENSE_TORCH_BWD=1 with
   ``_grad._DENSE_HIP`` off) have no such restriction and keep accepting any widths; the forward in front of them is a HIP
   kernel and refuses.  ``dense_descs`` only takes ``data_ptr()``, so all of this runs on CPU modules.
2. ``dense_descs`` reports ``hidden == H`` and kind 0 / 1 for the widths of the GPU sweep and for a layer of mixed kinds.
3. The reference itself at three shapes of the GPU tier: the oracle in float32 against the oracle in float64.  Measured
   on a CPU beforehand (worst of five shapes): outputs 1.3e-7, KL 1e-7, x.grad 2.9e-7, parameter gradients 1.2e-5; the
   bars here are four times that.  They guard the GPU bars (1e-4 / 5e-4) against a reference that is itself badly
   conditioned at a shape."""
import pytest
import torch

import dense_flow_cases as dfc


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _flow_of(bnn, transforms, kind, I=6):
    flow = bnn.flows.PropagateFlow(kind, I, 0)
    flow.transforms = torch.nn.ModuleList(transforms)
    return flow


BAD = [("RNVP", dict(h_sizes=(75, 50, 60, 75)), r"\(75, 50, 60, 75\)"),
       ("RNVP", dict(h_sizes=(75, 75, 75, 74)), r"\(75, 75, 75, 74\)"),
       ("RNVP", dict(h_sizes=(16, 32, 32, 32)), r"\(16, 32, 32, 32\)"),
       ("RNVP", dict(h_sizes=(75, 75, 75)), r"\(75, 75, 75\)"),
       ("RNVP", dict(h_sizes=(20, 20, 20, 20, 20)), r"\(20, 20, 20, 20, 20\)"),
       ("RNVP", dict(h_sizes=(129,) * 4), r"\(129, 129, 129, 129\)"),
       ("MNF", dict(hidden=129), r"hidden = 129"),
       ("MNF", dict(hidden=1000), r"hidden = 1000")]


@pytest.mark.parametrize("kind,kw,names", BAD, ids=[str(list(k[1].values())[0]) for k in BAD])
def test_widths_the_kernels_cannot_take_are_refused_on_every_descriptor_path(bnn, kind, kw, names):
    from bnn_amd import _grad, _lib, evaluate as ev
    assert _lib.MAX_HIDDEN == 128
    I = 8
    torch.manual_seed(0)
    cls = bnn.flows.RNVP if kind == "RNVP" else bnn.flows.MNF
    good = cls(I, **({"h_sizes": (5,) * 4} if kind == "RNVP" else {"hidden": 5}))
    bad = cls(I, **kw)
    masks = [torch.ones(I), torch.ones(I)]
    # the helper itself, and dense_descs with the bad transform first or second (every transform is checked before one is built)
    with pytest.raises(ValueError, match=names):
        bnn.flows.dense_hidden(kind, dict(bad.named_parameters()))
    for trs in ([bad, good], [good, bad]):
        with pytest.raises(ValueError, match=names):
            _flow_of(bnn, trs, kind, I).dense_descs(masks, masks)
        with pytest.raises(ValueError, match=names):
            _flow_of(bnn, trs, kind, I).dense_descs(None, None)
    # the layer: what its training forward and its backward call (layers.py) -- z flow and r flow
    for which in ("z_flow", "r_flow"):
        layer = bnn.mnf.BayesianLinear(I, 3, 0, z_flow_type=kind, r_flow_type=kind)
        layer.z_flow.transforms = torch.nn.ModuleList([cls(I, **(kw if which == "z_flow" else
                                                                   ({"h_sizes": (5,) * 4} if kind == "RNVP" else {"hidden": 5})))])
        layer.r_flow.transforms = torch.nn.ModuleList([cls(I, **(kw if which == "r_flow" else
                                                                   ({"h_sizes": (5,) * 4} if kind == "RNVP" else {"hidden": 5})))])
        layer.noise = {"zmask": [torch.ones(I)], "zmask2": [torch.ones(I)], "rmask": [torch.ones(I)]}
        dl = (_lib.DenseLayer * 1)()
        with pytest.raises(ValueError, match=names):
            layer._dense_layer_desc(dl[0], (True, True, False), [])
    # the single-workgroup route (lbbnn_flow_dense_apply[_backward]): refused before the autograd function is entered
    with pytest.raises(ValueError, match=names):
        _grad._dense_hip(torch.zeros(I), kind, [dict(bad.named_parameters())], masks[:1])
    # the frozen model / the batched ensemble: refused with the layer's number, before the device is looked at
    torch.manual_seed(1)
    net = bnn.mnf.BayesianNetwork((I, 4, 3), 1, z_flow_type=kind, r_flow_type=kind)
    net.l2.z_flow.transforms = torch.nn.ModuleList([cls(4, **kw)])
    with pytest.raises(ValueError, match=r"layer 2: z_flow.*" + names):
        ev.freeze(net, dense=True)
    with pytest.raises(ValueError, match=r"layer 2: z_flow.*" + names):
        ev.ensemble_forward(net, torch.zeros(2, I), 3, batched=True)


def test_torch_formulas_keep_taking_any_widths(bnn):
    """What does NOT refuse: the torch chain of _grad._dense (the fallback backward) on a CPU vector."""
    from bnn_amd import _grad
    torch.manual_seed(2)
    I = 8
    tr = bnn.flows.RNVP(I, h_sizes=(7, 5, 6, 7))
    z, ld = _grad._dense(torch.randn(I), "RNVP", [dict(tr.named_parameters())], [torch.bernoulli(torch.full((I,), 0.5))])
    assert z.shape == (I,) and bool(torch.isfinite(z).all()) and bool(torch.isfinite(ld))
    tr = bnn.flows.MNF(I, hidden=300)
    z, ld = _grad._dense(torch.randn(I), "MNF", [dict(tr.named_parameters())], [torch.bernoulli(torch.full((I,), 0.5))])
    assert z.shape == (I,) and bool(torch.isfinite(z).all()) and bool(torch.isfinite(ld))


@pytest.mark.parametrize("H", dfc.HIDDEN_SWEEP)
def test_dense_descs_reports_the_width_and_the_kind(bnn, H):
    I, T = 65, 2
    for kind, kid in (("RNVP", 0), ("MNF", 1)):
        flow = dfc.make_flow(bnn, kind, I, H, T)
        m = [torch.ones(I) for _ in range(T)]
        arr, n, keep = flow.dense_descs(m, None)
        assert n == T
        for t, tr in enumerate(flow.transforms):
            assert (arr[t].kind, arr[t].hidden) == (kid, H)
            first = tr.network[0] if kind == "RNVP" else tr.f
            assert arr[t].w_in == first.weight.data_ptr() and arr[t].b_in == first.bias.data_ptr()
            assert arr[t].mask_fwd == keep[t].data_ptr() and not arr[t].mask_kl
            assert bnn.flows.dense_hidden(kind, dict(tr.named_parameters())) == H


def test_dense_descs_of_a_layer_with_mixed_kinds_and_chain_lengths(bnn):
    layer = dfc.make_layer(bnn, 65, 5, 17, "RNVP", "MNF", 3, 1)
    assert layer._check_flows() == "dense"
    za, Tz, _ = layer.z_flow.dense_descs(None, None)
    ra, Tr, _ = layer.r_flow.dense_descs(None, None)
    assert (Tz, Tr) == (3, 1)
    assert [(za[t].kind, za[t].hidden) for t in range(Tz)] == [(0, 17)] * 3
    assert [(ra[t].kind, ra[t].hidden) for t in range(Tr)] == [(1, 17)]
    assert all(za[t].w_mid[l] and za[t].b_mid[l] for t in range(Tz) for l in range(3))
    assert not any(ra[0].w_mid[l] for l in range(3))                   # the MNF type has no middle layers
    empty = dfc.make_flow(bnn, "RNVP", 65, 17, 0)
    arr, T0, keep = empty.dense_descs([], [])
    assert T0 == 0 and keep == [] and len(arr) == 1 and not arr[0].w_in


# (I, O, B, H, zk, rk, Tz, Tr): the narrowest and the widest coupling network of the GPU sweep, and the longest chains
REHEARSAL = [(65, 5, 4, 1, "RNVP", "RNVP", 2, 2), (65, 5, 4, 128, "RNVP", "RNVP", 2, 2), (65, 5, 4, 17, "MNF", "MNF", 8, 8)]
FLOORS = {"out": 1.3e-7, "kl": 1e-7, "x": 2.9e-7, "param": 1.2e-5}


@pytest.mark.parametrize("I,O,B,H,zk,rk,Tz,Tr", REHEARSAL)
def test_reference_in_float32_against_itself_in_float64(bnn, I, O, B, H, zk, rk, Tz, Tr):
    layer = dfc.make_layer(bnn, I, O, H, zk, rk, Tz, Tr)
    g = torch.Generator().manual_seed(22)
    noise = dfc.make_noise(g, B, I, O, Tz, Tr)
    x = torch.rand(B, I, generator=g)
    state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    r64 = dfc.reference_layer(state, x, noise, zk, rk, Tz, Tr)
    r32 = dfc.reference_layer(state, x, noise, zk, rk, Tz, Tr, dtype=torch.float32)
    errs, perr = dfc.compare(r32, r64, tol=1.0, ptol=1.0)              # (the zero / None rule; the bars follow)
    for k in ("out", "kl", "x"):
        assert errs[k] <= 4 * FLOORS[k], (k, errs[k])
    for k, v in perr.items():
        assert v <= 4 * FLOORS["param"], (k, v)
