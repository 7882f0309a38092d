"""GPU tier of variational dropout's batched ensemble evaluation (evaluate.vd_ensemble / ensemble_forward / ensemble_eval on
a vd.BNN; include/lbbnn.h lbbnn_vd_gemm_members): the batched form is bitwise the loop of single forwards from the same Philox
state in every precision, matches the fp64 oracle on the regenerated noise, every fan-out member is bitwise its own single
launch in every kernel family the dispatch can pick, and the ensemble replays from a captured graph."""
import pytest
import torch

import philox_ref
from conftest import rel_err
from gemm_variant_cases import FAMILIES
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TIGHT = 5e-6
# the bars of the existing variational-dropout parity tests (fp16x3 / fp16x3f take the bf16x3 kernels in this layer)
BARS = {"fp32": TIGHT, "bf16x3": 2e-5, "fp16x3": 2e-5, "fp16x3f": 2e-5, "fp16": 2e-3, "bf16": 2e-2}
PRECISIONS = ("fp32", "bf16x3", "fp16x3", "fp16x3f", "bf16", "fp16")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture
def prec(bnn):
    def set_(p):
        bnn.set_precision(p)
    yield set_
    bnn.set_precision("fp32")


def _net(bnn, dev, dims, seed=0):
    torch.manual_seed(seed)
    return bnn.vd.BNN(dims).to(dev)


def _loop_vs_batched(bnn, net, x, S, **kw):
    """S consecutive net(x) and the batched ensemble from the same Philox state: (loop, batched, offsets) with the live
    offset before and after each."""
    st = bnn.ops.RngState.get(x.device)
    start = st.t.clone()
    with torch.no_grad():
        ref = torch.stack([net(x) for _ in range(S)])
    end_loop = st.t.clone()
    st.t.copy_(start)
    got = bnn.evaluate.ensemble_forward(net, x, S, **kw)
    end_batched = st.t.clone()
    return ref, got, int(start[1]), int(end_loop[1]), int(end_batched[1])


SHAPES = [((784, 1200, 1200, 1200, 10), 100, 10),      # the reference's VD network, its validation ensemble
          ((3072, 4096, 4096, 10), 512, 4),             # BASELINE configs[4]
          ((50, 37, 29, 3), 33, 5),                     # O % 4 != 0 (fp32 kernels after the first layer), ragged B
          ((64, 8), 40, 6)]                             # one layer: the O <= 16 head fans out


@pytest.mark.parametrize("p", PRECISIONS)
@pytest.mark.parametrize("dims,B,S", SHAPES)
def test_batched_equals_loop_bitwise(bnn, dev, prec, p, dims, B, S):
    net = _net(bnn, dev, dims, seed=len(dims))
    x = torch.rand(B, dims[0], device=dev, generator=torch.Generator(device=dev).manual_seed(B))
    prec(p)
    ref, got, live, end_loop, end_batched = _loop_vs_batched(bnn, net, x, S)
    L = len(dims) - 1
    assert got.shape == (S, B, dims[-1])
    assert torch.equal(got, ref), (p, float((got - ref).abs().max()))
    assert end_batched == end_loop == live + L * S
    assert not torch.equal(got[0], got[-1])                   # every member its own draw


def test_batched_single_member_and_chunks(bnn, dev, prec):
    dims, B = (784, 1200, 1200, 1200, 10), 100
    net = _net(bnn, dev, dims)
    x = torch.rand(B, 1, 28, 28, device=dev)
    for p in ("fp32", "bf16x3"):
        prec(p)
        ref, got, live, end_loop, end_batched = _loop_vs_batched(bnn, net, x, 1)
        assert torch.equal(got, ref) and end_batched == end_loop == live + 4
        st = bnn.ops.RngState.get(dev)
        start = st.t.clone()
        whole = bnn.evaluate.vd_ensemble(net, x, 10)
        end_whole = st.t.clone()
        st.t.copy_(start)
        chunked = bnn.evaluate.ensemble_forward(net, x, 10, max_members=3)
        assert torch.equal(chunked, whole)
        assert torch.equal(st.t[:2], end_whole[:2]) and int(end_whole[1]) == int(start[1]) + 40
        # batched=None took the batched form; batched=False is the loop
        st.t.copy_(start)
        loop = bnn.evaluate.ensemble_forward(net, x, 10, batched=False)
        assert torch.equal(loop, whole)


def test_misaligned_and_strided_input(bnn, dev, prec):
    """A first-layer input whose rows the split kernels cannot take (misaligned base, odd row stride) takes the kernel the
    loop takes, in the fan-out form too."""
    dims, B, S = (96, 80, 40, 10), 37, 4
    net = _net(bnn, dev, dims)
    b97, b100 = torch.rand(B, 97, device=dev), torch.rand(B, 100, device=dev)
    for p in ("fp32", "bf16x3"):
        prec(p)
        for x in (b97[:, 1:], b100[:, 1:97], b100[:, 4:]):
            ref, got, live, end_loop, end_batched = _loop_vs_batched(bnn, net, x, S)
            assert torch.equal(got, ref) and end_batched == end_loop


@pytest.mark.parametrize("p", PRECISIONS)
@pytest.mark.parametrize("dims,B,S", [((96, 64, 48, 10), 33, 4), ((784, 1200, 1200, 1200, 10), 100, 3)])
def test_against_fp64_oracle(bnn, dev, prec, p, dims, B, S):
    """Member m's zeta regenerated with tests/philox_ref.py at offset live + L*m + i, the oracle's vd_forward in fp64."""
    net = _net(bnn, dev, dims, seed=3)
    x = torch.rand(B, dims[0], device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    bnn.manual_seed(1234, 77)
    st = bnn.ops.RngState.get(dev)
    seed, live = int(st.t[0]), int(st.t[1])
    prec(p)
    got = bnn.evaluate.vd_ensemble(net, x, S).cpu()
    L = len(dims) - 1
    layers = net._layers()
    for m in range(S):
        h = x.double().cpu()
        for i, l in enumerate(layers):
            zeta = philox_ref.normal_matrix(seed, live + L * m + i, bnn.ops.STREAM_EPS_OUT * 64 + l._layer_id, B, l.m)
            h = orc.vd_forward(h, l.theta.detach().double().cpu(), l.alpha.double().cpu(), torch.from_numpy(zeta))
            if i < L - 1:
                h = torch.relu(h)
        ref = torch.log_softmax(h, dim=1)
        assert rel_err(got[m], ref) < BARS[p], (p, m, rel_err(got[m], ref))
    assert int(st.t[1]) == live + L * S


# kernel families of the dispatch (lrt_gemm_dispatch): (name, B, I, O, flags-name, relu), one or more rows per fan-out
# instantiation; the table and the host-side check that it is complete live in tests/gemm_variant_cases.py


@pytest.mark.parametrize("name,B,I,O,mode,relu", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_entry_point_fanout_and_members_equal_single_launches(bnn, dev, name, B, I, O, mode, relu):
    """Fan-out member m, and members-mode member m, equal bitwise the single lbbnn_lrt_gemm launch with var_scale at offset
    rng[1] + m * member_advance; NaN-poisoned outputs: every member's B x O block is written, the padding is not."""
    ops = bnn.ops
    torch.manual_seed(9)
    layer = bnn.vd.BayesianLayer(I, O).to(dev)
    layer.alpha.uniform_(0.05, 0.5)
    x = torch.rand(B, I, device=dev)
    split = mode != "fp32"
    half = mode == "fp16"
    single = mode in ("bf16", "fp16")
    e_w, var_w = layer._operands(split, half)
    S, adv, stream, row0 = 5, 3, ops.STREAM_EPS_OUT * 64 + 50, 7
    bnn.manual_seed(321, 1000)
    rng = ops.RngState.get(dev).t[:2].clone()
    o_ms = -(-(B * O) // 4) * 4 + 4                                   # padding past every member's block
    kw = dict(I=I, O=O, members=S, rng_stream=stream, row_offset=row0, member_advance=adv, relu=relu, split=split,
              single=single, half=half)

    def poisoned():
        return torch.full((S, o_ms), float("nan"), device=dev)

    buf_f = poisoned()
    ops.vd_gemm_members(x, e_w, var_w, layer.alpha, rng, fanout=True, out=buf_f[:, :B * O].view(S, B, O), **kw)
    xs = torch.empty((S, -(-(B * I) // 4) * 4 + 4), device=dev)[:, :B * I].view(S, B, I)
    xs.copy_(x.expand(S, B, I))
    buf_m = poisoned()
    ops.vd_gemm_members(xs, e_w, var_w, layer.alpha, rng, fanout=False, out=buf_m[:, :B * O].view(S, B, O), **kw)
    torch.cuda.synchronize()
    for m in range(S):
        r = rng.clone()
        r[1] += m * adv
        one = ops.lrt_gemm(x, e_w, var_w, I=I, O=O, var_scale=layer.alpha, rng=r, rng_stream=stream, row_offset=row0,
                           relu=relu, split=split, half=half, single=single)
        assert torch.equal(buf_f[m, :B * O].view(B, O), one), (name, m)
        assert torch.equal(buf_m[m, :B * O].view(B, O), one), (name, m)
    assert torch.isnan(buf_f[:, B * O:]).all() and torch.isnan(buf_m[:, B * O:]).all()
    assert not torch.equal(buf_f[0], buf_f[1])


def test_ensemble_eval_on_a_vd_net(bnn, dev):
    net = _net(bnn, dev, (784, 1200, 1200, 1200, 10))
    B = 100
    x = torch.rand(B, 1, 28, 28, device=dev)
    target = torch.randint(0, 10, (B,), device=dev)
    st = bnn.ops.RngState.get(dev)
    start = st.t.clone()
    r = bnn.evaluate.ensemble_eval(net, x, target, samples=10)
    assert not net.training
    st.t.copy_(start)
    outputs = bnn.evaluate.vd_ensemble(net, x, 10)
    assert torch.equal(r["outputs"], outputs)
    mean = outputs.mean(0)
    assert torch.equal(r["pred_ensemble"], mean.argmax(1))
    with torch.no_grad():
        loss = bnn.vd.loss_fn(mean, target, net)
    net.eval()
    assert torch.equal(r["loss"], loss)
    assert r["correct_ensemble"] == int(mean.argmax(1).eq(target).sum())
    assert "pred_posterior_mean" not in r and "density" not in r
    ent = bnn.evaluate.predictive_entropy(r["outputs"])
    assert ent.shape == (B,) and torch.isfinite(ent).all()
    r2 = bnn.evaluate.ensemble_eval(net, x, samples=3)
    assert set(r2) == {"outputs", "pred_ensemble"}


@pytest.mark.parametrize("p", ["fp32", "bf16x3"])
def test_graph_capture_replays_the_eager_ensemble(bnn, dev, prec, p):
    prec(p)
    net = _net(bnn, dev, (784, 1200, 1200, 1200, 10))
    x = torch.rand(100, 784, device=dev)
    st = bnn.ops.RngState.get(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bnn.evaluate.vd_ensemble(net, x, 10, max_members=4)          # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    start = st.t.clone()
    eager = bnn.evaluate.vd_ensemble(net, x, 10, max_members=4).clone()
    end = st.t.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = bnn.evaluate.vd_ensemble(net, x, 10, max_members=4)
    st.t.copy_(start)
    g.replay()
    assert torch.equal(out, eager)
    assert torch.equal(st.t[:2], end[:2])
    g.replay()                                                       # from the advanced state: fresh draws
    assert not torch.equal(out, eager)
    assert int(st.t[1]) == int(end[1]) + 40
