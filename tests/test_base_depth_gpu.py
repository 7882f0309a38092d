"""GPU tier of the baseline LBBNN at depth (base.BayesianNetwork of 1 to 16 layers): the draws="hip" training step against the
fp64 oracle composed per layer on regenerated draws, the log-probability totals (lbbnn_fold_rows), the ensemble contract with the
gate launch in groups, the evaluation stack, a captured nine-layer training step, and the three-layer network's unchanged calls.

Bars: the three-layer ones of tests/test_base_hip_draws_gpu.py and tests/test_base_draws_edges_gpu.py (TIGHT, SPLIT, GRAD below),
at every depth.  Worst errors measured on an MI355X, relaxed and hard gates, B = 5 and 70, fp32 and bf16x3 (these widths are
below the split kernels' shapes, so both precisions run the fp32 kernels: the two columns agree):

    layers   loss      log_prior  log_q     nll       worst parameter gradient
    1        1.6e-07   4.4e-08    2.1e-07   1.4e-07   8.7e-06
    2        4.4e-08   9.0e-08    8.2e-07   6.6e-08   2.7e-05
    3        6.4e-08   2.0e-07    1.7e-07   7.8e-08   6.8e-06
    4        9.1e-08   1.3e-07    2.7e-07   6.1e-08   9.9e-06
    5        5.3e-08   1.1e-07    3.6e-07   6.5e-08   1.4e-05
    9        1.4e-07   1.9e-07    3.7e-07   6.5e-08   1.6e-05
    16       9.3e-08   3.6e-08    5.2e-08   8.1e-08   2.7e-05
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from base_depth_ref import (NETS, _CACHE, _relaxed, _rng, chain, data, elbo_oracle, eval_oracle, eval_sensitivity, fold32,
                            make_net, mean_oracle, sensitivity)
from conftest import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 5e-6          # fp32 outputs
SPLIT = 2e-5          # bf16x3 outputs; loss, lp, lq, nll in both precisions
GRAD = {"fp32": 2e-4, "bf16x3": 5e-4}
T = 0.5
NB = 600
KEYS = list(NETS)
# Seeds of the networks' parameters, per check: 100 unless listed.  Chosen on the CPU to meet two conditions.
#
# 1. Every layer reaches the output.  With the gates of the check's own Philox state (the uniforms are the documented words,
#    tests/philox_ref.py), a 1 % change of any single layer's weight_mu moves the fp64 output by at least 2e-4: five times the
#    floor asserted below, which is twice SPLIT = 2e-5, the widest bar applied to what is formed from the output (loss, nll,
#    ensemble outputs).  The gradient bars (GRAD) are relative to each gradient's own largest entry, not to the output.
#    (Width 8 over 16 layers with half the gates shut lets the signal die for most seeds: the output of seed 101, hard gates,
#    does not depend on x at all.)
#
# 2. The scalar gradients d / d pa and d / d pb of every layer are conditioned.  Both are differences that can cancel
#    (base_depth_ref.pa_condition, pb_condition):
#      d loss / d pb sums +0.47 per shut gate and -0.48 per open one.  A 12 x 16 layer with hard gates that keeps 0.1 % of its
#        terms (nine layers, seed 100) comes out at 2.7e-4: 2.7e-7 of the terms, at a bar of 2e-4;
#      d loss / d pa is N (-1 / (pa + pb) - psi(pa)), zero at pa = 1.064, inside the U(1, 1.1) that pa is created from.  A layer
#        with pa = 1.0633, pb = 1.0332 (sixteen layers, seed 359) keeps 0.07 % and comes out at 7.5e-4: 4.7e-7 of the terms.
#    Every other number of such a step agrees to 1e-7.  That is the conditioning of one reference value on one small layer, at
#    any depth: the kernel's fp32 digamma is good to 1e-6, and three evaluations of it against a bar of 2e-4 need 1.5 % of the
#    terms to survive.  The seeds keep at least 2 % in every layer, which is asserted before the comparison.
PRIOR_COND = 0.02
SEEDS = {("elbo", "n1", False): 106, ("elbo", "n1", True): 106, ("elbo", "n2", False): 106, ("elbo", "n2", True): 112,
         ("elbo", "n4", True): 103, ("elbo", "n5", False): 107, ("elbo", "n5", True): 114, ("elbo", "n5c20", True): 114,
         ("elbo", "n9", False): 353, ("elbo", "n9", True): 206, ("elbo", "n16", False): 3970, ("elbo", "n16", True): 9444,
         ("ens", "n5", True): 101, ("ens", "n16", False): 104, ("ens", "n16", True): 103}
WORST = {}


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
    bnn.distributions.TEMPER_PRIOR = T
    yield
    bnn.distributions.TEMPER_PRIOR = old


@pytest.fixture
def prec(bnn):
    def set_(p):
        bnn.set_precision(p)
    yield set_
    bnn.set_precision("fp32")


def _case(bnn, dev, key, B, hard, check="elbo"):
    dims = NETS[key]
    seed = SEEDS.get((check, key, hard), 100)
    net = make_net(bnn, dims, hard, seed).to(dev)
    x, y = data(dims, B, seed + B)
    return net, x.to(dev), y.to(dev)


# ============================================================================================== 1 + 2. training step vs fp64
@pytest.mark.parametrize("hard", [False, True], ids=["relaxed", "hard"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("key", KEYS)
def test_elbo_step_vs_fp64_oracle(bnn, dev, temper, prec, key, B, precision, hard):
    ops = bnn.ops
    net, x, y = _case(bnn, dev, key, B, hard)
    net.train()
    layers = net._layers()
    n = len(layers)
    seed, off = 700 + n, 9
    rng = _rng(dev, seed, off)
    c = _CACHE.setdefault(("elbo", key, B, hard), {})
    # 1. a test that cannot see a wrong layer proves nothing: a 1 % change of ANY single layer's weight_mu moves the fp64 oracle's
    # output by at least twice SPLIT, the widest bar applied below to what is formed from the output (see SEEDS)
    if "shift" not in c:
        c["shift"], c["moves"] = sensitivity(ops, net, x, y, rng, T, NB)
    assert c["shift"] >= 2 * SPLIT, (c["shift"], c["moves"])
    # 2. the step
    prec(precision)
    ops.manual_seed(seed, off)
    st = ops.RngState.get(dev)
    loss, lp, lq, nll = net.sample_elbo(x, y, draws="hip", num_batches=NB)
    loss.backward()
    prec("fp32")
    assert int(st.t[1]) == off + 1
    if "ref" not in c:
        r = elbo_oracle(ops, net, x, y, rng, T, NB, alphas=[l.alpha for l in layers])
        r["loss"].backward()
        c["prior_cond"] = min(r["prior_cond"])
        c["ref"] = {"loss": r["loss"].detach(), "lp": r["lp"].detach(), "lq": r["lq"].detach(), "nll": r["nll"].detach(),
                    "grads": [{name: P[name].grad.clone() for name in layers[0]._names} for P in r["P"]]}
    ref = c["ref"]
    assert c["prior_cond"] >= PRIOR_COND, c["prior_cond"]    # d / d pa, d / d pb keep 2 % of their terms in every layer (SEEDS)
    errs = {"loss": rel_err(loss.detach(), ref["loss"]), "lp": rel_err(lp.detach(), ref["lp"]),
            "lq": rel_err(lq.detach(), ref["lq"]), "nll": rel_err(nll.detach(), ref["nll"])}
    g_err, g_who = 0.0, None
    for k, l in enumerate(layers):
        for name in l._names:
            assert getattr(l, name).grad is not None, (k, name)
            e = rel_err(getattr(l, name).grad, ref["grads"][k][name])
            if e > g_err:
                g_err, g_who = e, (k, name)
    w = WORST.setdefault((n, key, precision), dict(loss=0.0, lp=0.0, lq=0.0, nll=0.0, grad=0.0))
    for q in errs:
        w[q] = max(w[q], errs[q])
    w["grad"] = max(w["grad"], g_err)
    print("\nbase depth %-6s n=%2d B=%2d %-6s %-7s loss %.1e lp %.1e lq %.1e nll %.1e grad %.1e %s | worst so far: %s"
          % (key, n, B, precision, "hard" if hard else "relaxed", errs["loss"], errs["lp"], errs["lq"], errs["nll"], g_err, g_who,
             " ".join("%s %.1e" % kv for kv in w.items())))
    for q in errs:
        assert errs[q] < SPLIT, (q, errs[q])
    assert g_err < GRAD[precision], (g_who, g_err)


# ============================================================================================== 3. totals
@pytest.mark.parametrize("samples", [1, 2])
@pytest.mark.parametrize("key", [k for k in KEYS if len(NETS[k]) > 4])
def test_totals_are_the_left_fold_and_backward_matches_torch_adds(bnn, dev, temper, key, samples):
    ops = bnn.ops
    net, x, y = _case(bnn, dev, key, 5, False)
    net.train()
    layers = net._layers()
    assert len(layers) > 3 and net._fold_totals

    def step(record=False):
        net.zero_grad()
        ops.manual_seed(31, 4)
        calls = None
        if record:
            bnn._lib.RECORD = calls = []
        try:
            r = net.sample_elbo(x, y, samples, draws="hip", num_batches=NB)
            r[0].backward()
        finally:
            bnn._lib.RECORD = None
        return [t.detach().clone() for t in r], {name: p.grad.clone() for name, p in net.named_parameters()}, calls
    r1, g1, calls = step(record=True)
    assert [c[0] for c in calls].count("lbbnn_fold_rows") == samples          # one launch per sample
    if samples == 1:
        # the layers' published values are the last (only) sample's
        for got, attr in ((r1[1], "log_prior"), (r1[2], "log_variational_posterior")):
            want = fold32([getattr(l, attr) for l in layers])
            assert np.float32(got.item()).view(np.uint32) == want.view(np.uint32), (attr, got.item(), float(want))
    net._fold_totals = False
    r2, g2, _ = step()
    for a, b, what in zip(r1, r2, ("loss", "log_prior", "log_q", "nll")):
        assert torch.equal(a, b) if samples == 1 else rel_err(a, b) < 1e-6, what     # the same fp32 left fold
    for name in g1:
        assert rel_err(g1[name], g2[name]) < 1e-6, name


def test_fold_rows_is_the_fp32_left_fold(bnn, dev):
    g = torch.Generator().manual_seed(5)
    for rows, n, ld in ((1, 1, 1), (2, 16, 16), (3, 5, 9), (64, 7, 7), (2, 64, 64)):
        v = (torch.randn(rows, ld, generator=g) * 1000).to(dev)
        got = bnn.ops.fold_rows(v, rows, n).cpu().numpy()
        want = np.array([fold32(v[r, :n].cpu().numpy()) for r in range(rows)], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rows, n, ld)


# ============================================================================================== 4. ensemble contract
ENS = [(k, h, "fp32") for k in KEYS for h in (False, True)] + [(k, False, "bf16x3") for k in ("n5", "n9")]


@pytest.mark.parametrize("key,hard,precision", ENS, ids=["%s-%s-%s" % (k, "hard" if h else "relaxed", p) for k, h, p in ENS])
def test_ensemble_members_are_the_chain_at_consecutive_offsets(bnn, dev, temper, prec, key, hard, precision):
    ops, ev = bnn.ops, bnn.evaluate
    net, x, _ = _case(bnn, dev, key, 5, hard, "ens")
    layers = net._layers()
    n, S = len(layers), 3
    prec(precision)
    ops.manual_seed(41, 20)
    st = ops.RngState.get(dev)
    r = ev.base_ensemble(net, x, S, keep_gates=True)
    assert int(st.t[1]) == 20 + S
    assert r["outputs"].shape == (S, 5, NETS[key][-1])
    assert len(r["gate_rows"]) == n and len(r["gates"]) == n
    ops.manual_seed(41, 20)
    r2 = ev.base_ensemble(net, x, S, max_members=2, keep_gates=True)
    assert int(st.t[1]) == 20 + S
    assert torch.equal(r2["outputs"], r["outputs"])
    for k in range(n):
        assert torch.equal(r2["gate_rows"][k], r["gate_rows"][k]) and torch.equal(r2["gates"][k], r["gates"][k]), k
    for m in range(S):
        rng = _rng(dev, 41, 20 + m)
        with torch.no_grad():
            ref = chain(net, x, rng)
        assert torch.equal(r["outputs"][m], ref), (m, float((r["outputs"][m] - ref).abs().max()))
        for k, l in enumerate(layers):
            gk = r["gates"][k][m]
            assert gk.shape == (l.out_features, l.in_features)
            assert torch.equal(gk, l.gammas), (m, k)                # the chain just drew them at this offset
            u = ops.philox_uniform(rng, ops.STREAM_GATE * 64 + l._layer_id, l.out_features, l.in_features)
            if hard:
                assert torch.equal(gk, (u < l.alpha).float())
            else:
                assert float((gk - _relaxed(l.alpha, u, T)).abs().max()) < 1e-4
            assert float((r["gate_rows"][k][m].double() - gk.double().sum(1)).abs().max()) < 1e-3
    g0 = [r["gates"][k][0] for k in range(n)]
    h64 = eval_oracle(ops, net, x, _rng(dev, 41, 20), g0)
    bar = TIGHT if precision == "fp32" else SPLIT
    shift = eval_sensitivity(ops, net, x, _rng(dev, 41, 20), g0, h64)
    assert shift >= 2 * bar, shift                           # every layer reaches the output
    assert rel_err(r["outputs"][0], h64) < bar
    assert torch.equal(net.sample_predict(x, rng=_rng(dev, 41, 21)), r["outputs"][1])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("key", ["n5", "n9"])
def test_median_probability_model_at_depth(bnn, dev, temper, prec, key, precision):
    ops = bnn.ops
    net, x, _ = _case(bnn, dev, key, 5, True, "mpm")
    layers = net._layers()
    n, S = len(layers), 2
    prec(precision)
    ops.manual_seed(43, 0)
    r = bnn.evaluate.base_ensemble(net, x, S, gates="mpm", keep_gates=True)
    assert int(ops.RngState.get(dev).t[1]) == S
    for k, l in enumerate(layers):
        mpm = ((1 / (1 + torch.exp(-l.lambdal.detach()))) > 0.5).float()       # LBBNN-GP-MF.py:469-473
        far = l.lambdal.detach().abs() > 1e-5          # (alpha within an ulp of 0.5 may round either way)
        for m in range(S):
            assert torch.equal(r["gates"][k][m][far], mpm[far]), (k, m)
    for m in range(S):
        gm = [r["gates"][k][m] for k in range(n)]
        h64 = eval_oracle(ops, net, x, _rng(dev, 43, m), gm)
        bar = TIGHT if precision == "fp32" else SPLIT
        assert eval_sensitivity(ops, net, x, _rng(dev, 43, m), gm, h64) >= 2 * bar, m
        assert rel_err(r["outputs"][m], h64) < bar, m


# ============================================================================================== 5. evaluation stack
def test_evaluation_stack_on_five_layers(bnn, dev, temper):
    ops, ev = bnn.ops, bnn.evaluate
    key, B, S = "n5", 70, 4
    net, x, y = _case(bnn, dev, key, B, True)
    layers = net._layers()
    C = NETS[key][-1]
    ops.manual_seed(47, 0)
    full = ev.base_ensemble(net, x, S, keep_gates=True)
    ops.manual_seed(47, 0)
    res = ev.ensemble_eval(net, x, y, S)
    assert torch.equal(res["outputs"], full["outputs"]) and res["density"].shape == (S,)
    # density: the mean gate of the member over the weights of ALL five layers.  fp32 row sums of at most 20 gates in [0, 1]
    # and one fp32 rounding of the quotient: within (20 + 1) * 2^-24 of the fp64 mean, relative
    n_w = sum(l.lambdal.numel() for l in layers)
    for m in range(S):
        want = sum(float(full["gates"][k][m].double().sum()) for k in range(len(layers))) / n_w
        assert abs(float(res["density"][m]) - want) <= 21 * 2.0 ** -24 * want, m
    # the posterior-mean forward takes five None gates; against the fp64 joint-mean forward where its top two are apart
    h = mean_oracle(net, x)
    top2 = h.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert int(clear.sum()) > B // 2
    assert torch.equal(res["pred_posterior_mean"].cpu()[clear], h.argmax(1)[clear])
    assert torch.equal(res["pred_ensemble"], res["outputs"].mean(0).argmax(1))
    # evaluate_batches with both accumulators: two batches, one synchronisation
    batches = [(x[:30], y[:30]), (x[30:], y[30:])]
    ops.manual_seed(47, 0)
    unc = ev.UncertaintyAccumulator(C, S, dev)
    out = ev.evaluate_batches(net, batches, S, acc=ev.EvalAccumulator(C, S, dev), uncertainty=unc)
    assert int(ops.RngState.get(dev).t[1]) == 2 * S
    assert out["rows"] == B and out["rows_with_target"] == B and out["bad_targets"] == 0
    ops.manual_seed(47, 0)
    c_ens = c_mean = 0
    for xb, yb in batches:
        o = ev.base_ensemble(net, xb, S)["outputs"]
        acc = o[0].clone()
        for m in range(1, S):
            acc += o[m]
        c_ens += int((acc / S).argmax(1).eq(yb).sum())
        c_mean += int(net(xb, *[None] * len(layers), sample=False).argmax(1).eq(yb).sum())
    assert out["correct_ensemble"] == c_ens and out["correct_posterior_mean"] == c_mean
    assert "correct_bma" in out and 0 <= out["correct_bma"] <= B
    with pytest.raises(TypeError, match="baseline"):
        ev.freeze(net)                                      # a frozen baseline model is not built


# ============================================================================================== 6. graphed training
def test_graphed_nine_layer_step_equals_eager_subprocess():
    """A captured nine-layer draws="hip" training step (make_graphed_train_step + optim.Adam): three replays are bitwise three
    eager steps from the same seed and parameters -- losses and every parameter, as the three-layer test of
    tests/test_base_hip_draws_gpu.py asserts.  The optimizer holds 99 tensors in two lists.  Own process (capture wants a clean
    autograd state)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, copy, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import bnn_amd
from base_depth_ref import NETS, make_net, data
dev = torch.device("cuda:0")
dims = NETS["n9"]
net = make_net(bnn_amd, dims, False, 3).to(dev).train()
assert len(net._layers()) == 9 and len(list(net.parameters())) == 99
init = copy.deepcopy(net.state_dict())
opt = bnn_amd.optim.Adam(net.parameters(), lr=3e-2)
x, y = data(dims, 70, 4)
x, y = x.to(dev), y.to(dev)
lf = lambda n, a, b: n.sample_elbo(a, b, draws="hip")[0]
step = bnn_amd.graphs.make_graphed_train_step(net, opt, lf, x, y)

def reset():
    net.load_state_dict(init)
    for s in opt.state.values():
        s["exp_avg"].zero_(); s["exp_avg_sq"].zero_()
    for gr in opt.param_groups:
        gr["step_dev"].zero_()
    bnn_amd.manual_seed(7)

reset()
gl = [float(step(x, y)) for _ in range(3)]
gp = {k: v.detach().clone() for k, v in net.named_parameters()}
assert any(not torch.equal(gp[k], init[k]) for k in gp)
reset()
el = []
for _ in range(3):
    opt.zero_grad(set_to_none=True)
    loss = lf(net, x, y)
    loss.backward()
    opt.step()
    el.append(float(loss.detach()))
del loss
torch.cuda.synchronize()
assert gl == el, (gl, el)
for k, v in net.named_parameters():
    assert torch.equal(v.detach(), gp[k]), k
lists = opt.__dict__["_lists"]
assert len(lists) == 2 and sum(l[1].n for l in lists.values()) == 99, [l[1].n for l in lists.values()]
print("BASEDEPTHGRAPH_OK", gl)
""" % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BASEDEPTHGRAPH_OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])


# ============================================================================================== 7. compatibility
# C calls of a three-layer network as the commit before depth made them (recorded there with _lib.RECORD on the same three
# pieces of code): the torch-draw forward, the draws="hip" step with its backward, and a three-member ensemble
_FWD = ["lbbnn_gate_sample", "lbbnn_lrt_gemm", "lbbnn_rng_advance"]
_BWD = ["lbbnn_output_grad", "lbbnn_transpose_operand", "lbbnn_lrt_gemm", "lbbnn_gate_backward_draw"]
_DX = ["lbbnn_transpose_operand", "lbbnn_lrt_gemm"]
PARENT_CALLS = {
    "forward": _FWD * 3,
    "step": (["lbbnn_rng_advance"] + ["lbbnn_gate_sample_draw", "lbbnn_lrt_gemm"] * 3
             + ["lbbnn_elbo_loss", "lbbnn_elbo_loss_backward_logits"] + _BWD + _DX + _BWD + _DX + _BWD),
    "ensemble": ["lbbnn_gate_members"] + ["lbbnn_gemm_members_mean"] * 3 + ["lbbnn_rng_advance"],
}


def test_three_layer_network_calls_are_unchanged(bnn, dev, temper):
    ops = bnn.ops
    net, x, y = _case(bnn, dev, "n3", 5, False)
    net.eval()
    gs = [torch.rand(l.out_features, l.in_features, generator=torch.Generator().manual_seed(k)).to(dev)
          for k, l in enumerate(net._layers())]
    with torch.no_grad():
        ops.manual_seed(51, 0)
        a = net(x, gs[0], gs[1], gs[2], sample=True)
        ops.manual_seed(51, 0)
        b = net(x, g1=gs[0], g2=gs[1], g3=gs[2], sample=True)
        ops.manual_seed(51, 0)
        c = net(x, gs[0], gs[1], gs[2], True, False)
    assert torch.equal(a, b) and torch.equal(a, c)
    got = {}
    try:
        bnn._lib.RECORD = rec = []
        with torch.no_grad():
            net(x, gs[0], gs[1], gs[2], sample=True)
        got["forward"] = [r[0] for r in rec]
        net.train()
        bnn._lib.RECORD = rec = []
        net.sample_elbo(x, y, draws="hip")[0].backward()
        got["step"] = [r[0] for r in rec]
        bnn._lib.RECORD = rec = []
        bnn.evaluate.base_ensemble(net, x, 3)
        got["ensemble"] = [r[0] for r in rec]
    finally:
        bnn._lib.RECORD = None
    print("\nthree-layer C calls:", got)
    assert "lbbnn_fold_rows" not in got["step"]
    assert got == PARENT_CALLS
