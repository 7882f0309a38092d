"""GPU tier of the baseline LBBNN's batched ensemble evaluation (evaluate.base_ensemble / ensemble_forward / ensemble_eval,
BayesianNetwork.sample_predict; include/lbbnn.h lbbnn_gate_members + lbbnn_gemm_members_mean): member m is bitwise the
training kernels' chain at Philox offset (live + m) in every precision, chunking and the loop form change no bit, the gates
are the documented draws, the outputs match the fp64 oracle on the regenerated noise, and the statistics come out right."""
import pytest
import torch

from base_draw_ref import _chain, _relaxed, _rng
from conftest import rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TIGHT = 5e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture
def temper(bnn):
    old = bnn.distributions.TEMPER_PRIOR

    def set_(t):
        bnn.distributions.TEMPER_PRIOR = t
    yield set_
    bnn.distributions.TEMPER_PRIOR = old


def _net(bnn, dev, dims, hard, seed=0):
    torch.manual_seed(seed)
    net = bnn.base.BayesianNetwork(dims).to(dev)
    with torch.no_grad():
        for l in (net.l1, net.l2, net.l3):
            l.lambdal.uniform_(-2.5, 2.5)          # gates that vary (the default init puts every alpha in (0.5, 0.73))
            l.gamma.exact = hard
    return net


SHAPES = [((784, 400, 600, 10), 1000, 10), ((50, 37, 29, 3), 33, 3)]


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "fp16x3f"])
@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=["784-400-600-10", "50-37-29-3"])
def test_ensemble_members_equal_the_training_chain_bitwise(bnn, dev, temper, prec, hard, shape):
    dims, B, S = shape
    temper(0.5)
    net = _net(bnn, dev, dims, hard)
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(1)).to(dev)
    ops, ev = bnn.ops, bnn.evaluate
    bnn.set_precision(prec)
    try:
        ops.manual_seed(7, 100)
        st = ops.RngState.get(dev)
        off = int(st.t[1])
        out = ev.ensemble_forward(net, x, S)
        assert int(st.t[1]) == off + S
        assert out.shape == (S, B, dims[-1])
        with torch.no_grad():
            for m in range(S):
                ref = _chain(net, x, _rng(dev, 7, off + m))
                assert torch.equal(out[m], ref), (prec, hard, m, float((out[m] - ref).abs().max()))
        assert not torch.equal(out[0], out[1])
        ops.manual_seed(7, 100)
        out3 = ev.ensemble_forward(net, x, S, max_members=3)
        assert torch.equal(out3, out) and int(st.t[1]) == off + S
        ops.manual_seed(7, 100)
        loop = ev.ensemble_forward(net, x, S, batched=False)
        assert torch.equal(loop, out) and int(st.t[1]) == off + S
    finally:
        bnn.set_precision("fp32")


def test_sample_predict_is_member_zero_and_advances_once(bnn, dev):
    net = _net(bnn, dev, (784, 400, 600, 10), True)
    x = torch.rand(64, 1, 28, 28, device=dev)
    ops = bnn.ops
    ops.manual_seed(11, 5)
    st = ops.RngState.get(dev)
    out = net.sample_predict(x)
    assert int(st.t[1]) == 6 and out.shape == (64, 10)
    assert torch.equal(out, net.sample_predict(x, rng=_rng(dev, 11, 5)))      # an explicit snapshot does not advance
    assert int(st.t[1]) == 6
    ops.manual_seed(11, 5)
    ens = bnn.evaluate.ensemble_forward(net, x, 2)
    assert torch.equal(ens[0], out)
    assert torch.allclose(out.exp().sum(1), torch.ones(64, device=dev), atol=1e-5)


@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_gates_and_outputs_against_the_oracle(bnn, dev, temper, hard, prec):
    temper(0.5)
    dims, B, S = (784, 400, 600, 10), 64, 3
    net = _net(bnn, dev, dims, hard, seed=2)
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(3)).to(dev)
    ops = bnn.ops
    layers = (net.l1, net.l2, net.l3)
    bnn.set_precision(prec)
    try:
        ops.manual_seed(21, 9)
        r = bnn.evaluate.base_ensemble(net, x, S, keep_gates=True)
        for m in range(S):
            rng = _rng(dev, 21, 9 + m)
            h64 = x.double().cpu()
            for k, l in enumerate(layers):
                O, I, L = l.out_features, l.in_features, l._layer_id
                g = r["gates"][k][m]
                u = ops.philox_uniform(rng, ops.STREAM_GATE * 64 + L, O, I)
                with torch.no_grad():
                    l.sample_forward(h64.float().to(dev), rng=rng)       # the training kernel's alpha of the same lambdal
                alpha = l.alpha
                assert float((alpha - torch.sigmoid(l.lambdal.detach())).abs().max()) < 1e-6
                if hard:
                    assert torch.equal(g, (u < alpha).float())
                else:
                    assert float((g - _relaxed(alpha, u, 0.5)).abs().max()) < 1e-4
                assert float((r["gate_rows"][k][m].double() - g.double().sum(1)).abs().max()) < 1e-3
                P64 = {n: getattr(l, n).detach().double().cpu() for n in l._names}
                noise = {"eps_w": ops.philox_normal(rng, ops.STREAM_EPS_W * 64 + L, O, I).double().cpu(),
                         "eps_b": ops.philox_normal(rng, ops.STREAM_EPS_B * 64 + L, 0, O).double().cpu()}
                h64, _, _ = orc.base_forward(h64, P64, g.double().cpu(), noise, mode="sample", compute_lp=False)
                h64 = torch.relu(h64) if k < 2 else torch.log_softmax(h64, dim=1)
            assert rel_err(r["outputs"][m], h64) < (TIGHT if prec == "fp32" else 2e-5), m
    finally:
        bnn.set_precision("fp32")


def test_mpm_gates_and_outputs(bnn, dev):
    dims, B, S = (784, 400, 600, 10), 64, 3
    net = _net(bnn, dev, dims, True, seed=4)
    x = torch.rand(B, dims[0], generator=torch.Generator().manual_seed(5)).to(dev)
    ops = bnn.ops
    ops.manual_seed(3, 0)
    st = ops.RngState.get(dev)
    r = bnn.evaluate.base_ensemble(net, x, S, gates="mpm", keep_gates=True)
    assert int(st.t[1]) == S
    h64 = [x.double().cpu() for _ in range(S)]
    for k, l in enumerate((net.l1, net.l2, net.l3)):
        O, I, L = l.out_features, l.in_features, l._layer_id
        mpm = ((1 / (1 + torch.exp(-l.lambdal.detach()))) > 0.5).float()       # LBBNN-GP-MF.py:469-473
        assert 0 < float(mpm.mean()) < 1
        P64 = {n: getattr(l, n).detach().double().cpu() for n in l._names}
        far = l.lambdal.detach().abs() > 1e-5          # (alpha within an ulp of 0.5 may round either way)
        for m in range(S):
            g = r["gates"][k][m]
            assert torch.equal(g[far], mpm[far])
            assert torch.equal(r["gate_rows"][k][m], g.sum(1))
            rng = _rng(dev, 3, m)
            noise = {"eps_w": ops.philox_normal(rng, ops.STREAM_EPS_W * 64 + L, O, I).double().cpu(),
                     "eps_b": ops.philox_normal(rng, ops.STREAM_EPS_B * 64 + L, 0, O).double().cpu()}
            o, _, _ = orc.base_forward(h64[m], P64, g.double().cpu(), noise, mode="sample", compute_lp=False)
            h64[m] = torch.relu(o) if k < 2 else torch.log_softmax(o, dim=1)
    for m in range(S):
        assert rel_err(r["outputs"][m], h64[m]) < TIGHT
    assert not torch.equal(r["outputs"][0], r["outputs"][1])      # same gates, different weight noise
    ops.manual_seed(3, 0)
    assert torch.equal(bnn.evaluate.ensemble_forward(net, x, S, gates="mpm", batched=False), r["outputs"])


def test_hard_gate_density_statistics(bnn, dev):
    S = 200
    net = _net(bnn, dev, (784, 400, 600, 10), True, seed=6)
    x = torch.rand(8, 784, device=dev)
    bnn.ops.manual_seed(99, 0)
    r = bnn.evaluate.base_ensemble(net, x, S, max_members=64)
    for k, l in enumerate((net.l1, net.l2, net.l3)):
        alpha = torch.sigmoid(l.lambdal.detach().double())
        n = alpha.numel()
        dens = r["gate_rows"][k].double().sum(1) / n                 # (S,)
        sigma = float(torch.sqrt((alpha * (1 - alpha)).sum())) / n / S ** 0.5
        assert abs(float(dens.mean()) - float(alpha.mean())) < 4 * sigma, (k, float(dens.mean()), float(alpha.mean()), sigma)
        assert float(dens.std()) > 0


def test_ensemble_eval_on_a_baseline_network(bnn, dev):
    dims, B, S = (784, 400, 600, 10), 200, 10
    net = _net(bnn, dev, dims, True, seed=8)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(B, 1, 28, 28, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    res = bnn.evaluate.ensemble_eval(net, x, y, S)
    assert set(res) == {"outputs", "pred_ensemble", "pred_posterior_mean", "density", "correct_ensemble",
                        "correct_posterior_mean"}
    assert res["outputs"].shape == (S, B, 10)
    assert res["pred_ensemble"].shape == (B,) and res["pred_posterior_mean"].shape == (B,)
    assert res["density"].shape == (S,)
    assert isinstance(res["correct_ensemble"], int) and isinstance(res["correct_posterior_mean"], int)
    layers = (net.l1, net.l2, net.l3)
    alpha_mean = sum(float(torch.sigmoid(l.lambdal.detach()).sum()) for l in layers) / sum(l.lambdal.numel() for l in layers)
    assert float((res["density"] - alpha_mean).abs().max()) < 0.01
    assert torch.equal(res["pred_ensemble"], res["outputs"].mean(0).argmax(1))
    # the posterior mean: the oracle's mode-2 forward with alpha = sigmoid(lambdal) (LBBNN-GP-MF.py:369-374, :413)
    h = x.view(B, -1).double().cpu()
    for k, l in enumerate(layers):
        P64 = {n: getattr(l, n).detach().double().cpu() for n in l._names}
        alpha = 1 / (1 + torch.exp(-P64["lambdal"]))
        h, _, _ = orc.base_forward(h, P64, None, {}, mode="mean", compute_lp=False, alpha_attr=alpha)
        h = torch.relu(h) if k < 2 else torch.log_softmax(h, dim=1)
    top2 = h.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert int(clear.sum()) > B // 2
    assert torch.equal(res["pred_posterior_mean"].cpu()[clear], h.argmax(1)[clear])


def test_injected_noise_and_bad_gates_raise(bnn, dev):
    net = _net(bnn, dev, (50, 37, 29, 3), False)
    x = torch.rand(5, 50, device=dev)
    with pytest.raises(ValueError):
        bnn.evaluate.ensemble_forward(net, x, 2, gates="hard")
    net.l2.noise = {"eps_w": torch.zeros(29, 37, device=dev)}
    for batched in (True, False):
        with pytest.raises(ValueError, match="noise"):
            bnn.evaluate.ensemble_forward(net, x, 2, batched=batched)
    with pytest.raises(ValueError, match="noise"):
        net.sample_predict(x)
