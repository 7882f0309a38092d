"""GPU tier: the first layer's x as fp16 planes, formatted by workgroups behind the rows of the weight-pass launch (the default
of the fused "fp16x3f" forward), against the fp32-x form (LBBNN_F16_FIRST=f32: the split in the GEMM's registers).  Both forms
feed the same hi | lo values into the same products, so log_probs and kl are BYTE-equal -- eager, through a LaunchPlan replay
and through a captured graph, from the same Philox {seed, offset}.  Under "fp16x3" the GEMM's three variance products square the
fp32 x itself where it has it (the planes form differs in the last bits), so there the default keeps fp32 x; a first layer the
format job does not take (I % 8 != 0) keeps fp32 x too, silently."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _forward_all_ways(bnn, net, x):
    """(log_probs, kl) of one forward at Philox {7, 3}: eager, LaunchPlan replay, graph replay."""
    from bnn_amd import graphs
    res = []
    with torch.no_grad():
        bnn.manual_seed(7, 3)
        out = net(x, sample=True).clone()
        res.append((out, net.kl().clone()))
        plan = graphs.LaunchPlan(net, x, sample=True)
        bnn.manual_seed(7, 3)
        o, k = plan()
        res.append((o.clone(), k.clone()))
        net(x, sample=True)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            og = net(x, sample=True)
            kg = net.kl()
        bnn.manual_seed(7, 3)
        gr.replay()
        torch.cuda.synchronize()
        res.append((og.clone(), kg.clone()))
    return res


def _bytes_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("prec", ["fp16x3", "fp16x3f"])
@pytest.mark.parametrize("B", [1, 129])
@pytest.mark.parametrize("dims", [(264, 96, 10), (784, 96, 10)])
def test_first_planes_equal_fp32_x_bytes(bnn, dev, monkeypatch, dims, B, prec):
    from bnn_amd import layers as L
    torch.manual_seed(dims[0] + B)
    net = bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
    net.set_precision(prec)
    x = torch.rand(B, dims[0], device=dev)
    assert L._F16_FIRST_PLANES is None                           # no override in the environment: the default rule
    monkeypatch.setattr(L, "_F16_FIRST_PLANES", False)           # LBBNN_F16_FIRST=f32
    ref = _forward_all_ways(bnn, net, x)
    assert net._layers()[0]._split_now == (3 if prec == "fp16x3f" else 2)
    assert not any(k[0] == "planes" and k[1] == "in" for k in net._plane_cache)
    monkeypatch.setattr(L, "_F16_FIRST_PLANES", None)
    new = _forward_all_ways(bnn, net, x)
    # the planes form really ran where it is the default: the single-variance-product first layer of "fp16x3f"; the three
    # products of "fp16x3" square the fp32 x itself, which planes cannot reproduce bit for bit, so that layer keeps fp32 x
    assert any(k[0] == "planes" and k[1] == "in" for k in net._plane_cache) == (prec == "fp16x3f")
    assert torch.isfinite(ref[0][0]).all() and float(ref[0][0].abs().max()) > 0
    for how, (o, k) in zip(("eager", "plan", "graph"), new):
        assert _bytes_equal(o, ref[0][0]) and _bytes_equal(k, ref[0][1]), (how, "planes against eager fp32 x")
    for how, (o, k) in zip(("eager", "plan", "graph"), ref):
        assert _bytes_equal(o, ref[0][0]) and _bytes_equal(k, ref[0][1]), (how, "fp32 x against eager fp32 x")


@pytest.mark.parametrize("B", [1, 129])
def test_first_layer_the_format_job_does_not_take_keeps_fp32_x(bnn, dev, monkeypatch, B):
    """I = 260 (I % 8 != 0): the first layer keeps fp32 operands and fp32 x under both settings, silently, with equal bytes;
    the second layer still takes a 16-bit format."""
    from bnn_amd import layers as L
    torch.manual_seed(260 + B)
    net = bnn.mnf.BayesianNetwork((260, 96, 96, 10), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
    net.set_precision("fp16x3f")
    x = torch.rand(B, 260, device=dev)
    monkeypatch.setattr(L, "_F16_FIRST_PLANES", False)
    ref = _forward_all_ways(bnn, net, x)
    monkeypatch.setattr(L, "_F16_FIRST_PLANES", None)
    new = _forward_all_ways(bnn, net, x)
    assert net._layers()[0]._split_now == 0 and net._layers()[1]._split_now >= 1
    assert not any(k[0] == "planes" and k[1] == "in" for k in net._plane_cache)
    for how, (o, k) in zip(("eager", "plan", "graph"), new):
        assert _bytes_equal(o, ref[0][0]) and _bytes_equal(k, ref[0][1]), how
