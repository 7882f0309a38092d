"""GPU tier of the frozen baseline model (evaluate.freeze_base / FrozenBaseNetwork; include/lbbnn.h
lbbnn_base_frozen_operands, lbbnn_base_frozen_members).

1. A full model is base_ensemble, bit for bit: outputs, member weights and biases (a stored +0.0 where the loop stores -0.0 is
   the one allowed difference), chunked or not, and the Philox offset advances by the member count.
2. A compact median-probability model: member weight (o', j') and every bias are the full frozen model's at (rows[o'],
   cols[j']), bit for bit.
3. Its outputs, and the full model's, equal an fp64 forward composed on the CPU from the full model's member weights read back.
4. The posterior-mean forward equals the fp64 mean forward, and in sample mode _base_mean_forward to 1e-6.
5. Every buffer is fully written: with NaN-filled allocations all results are finite and every tail is zero.
6. A graphed evaluation step replays the eager results bitwise, and its totals are evaluate_batches'.

Bars: those of tests/test_frozen_compact_gpu.py, 5e-6 of max|out| with fp32 operands and 2e-5 under "bf16x3" (rel_err).
Shapes: (13, 9, 3) has in_features % 4 != 0 and a partial last Philox quad; (40, 24, 24, 10) under "bf16x3" takes the split
layout with ld - I = 24; five layers make two launch groups; (20, 1) is the sigmoid head as two classes."""
import ctypes

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

BAR = {"fp32": 5e-6, "bf16x3": 2e-5}
SEED, OFF, S = 7, 11, 3
CASES = [((13, 9, 3), "fp32", "log_softmax"), ((40, 24, 24, 10), "bf16x3", "log_softmax"),
         ((16, 16, 16, 16, 16, 4), "fp32", "log_softmax"), ((20, 1), "fp32", "sigmoid")]
IDS = ["13-9-3", "40-24-24-10-bf16x3", "five-layers", "20-1-sigmoid"]
GATES = ["sample", "sample-hard", "mpm"]
# the member-GEMM chain's head cases no case above reaches: log_softmax by torch (C > 16) and the sigmoid head's probabilities
# (log_probs off, the 4th field); B * C = 90 / 5 at B = 5, so the member stride pad4(B * C) is padded
HEAD_CASES = [((8, 12, 20, 18), p, "log_softmax", False) for p in ("fp32", "bf16x3")] + \
             [((8, 12, 20, 1), p, "sigmoid", False) for p in ("fp32", "bf16x3")]
HEAD_IDS = ["8-12-20-18", "8-12-20-18-bf16x3", "8-12-20-1-probs", "8-12-20-1-probs-bf16x3"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture
def precision(bnn):
    def set_(p):
        bnn.set_precision(p)
    yield set_
    bnn.set_precision("fp32")


_NETS = {}


def _net(bnn, dev, dims, head):
    """The network of a case (built once per module, never changed): lambdal on both sides of 0, so the median model prunes."""
    if (dims, head) not in _NETS:
        torch.manual_seed(21)
        _NETS[(dims, head)] = bnn.base.BayesianNetwork(dims, head=head, lambdal_init=(-2.0, 2.0)).to(dev).eval()
    return _NETS[(dims, head)]


def _x(dev, B, I, seed=1):
    return torch.rand(B, I, generator=torch.Generator().manual_seed(seed + B)).to(dev)


def _set_hard(net, hard):
    for l in net._layers():
        l.gamma.exact = bool(hard)


def _loop_members(bnn, net, x, members, gates):
    """Member weights and biases as base_ensemble's own draw call makes them (lbbnn_gate_members on the layers' parameters,
    the operand formats of BayesianNetwork._predict_members) from the live Philox state, which is left where it was."""
    from bnn_amd import _lib, distributions
    ops = bnn.ops
    layers = net._layers()
    n = len(layers)
    splits = []
    for k, l in enumerate(layers):
        in_ok = (x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0) if k == 0 else layers[k - 1].out_features % 4 == 0
        splits.append(bool(ops.split_precision() and ops.split_eligible(l.in_features, l.out_features) and in_ok))
    descs = (_lib.GateMemberDesc * n)()
    bufs = [l._fill_member_desc(descs[k], members, splits[k]) for k, l in enumerate(layers)]
    st = ops.RngState.get(x.device)
    mode = ops.GATES_MPM if gates == "mpm" else ops.GATES_SAMPLE
    for k, cnt in _lib.layer_groups(n):
        _lib.check(_lib.lib().lbbnn_gate_members(_lib.group_slice(descs, k, cnt), cnt, members, mode,
                                                 float(distributions.TEMPER_PRIOR), st.t.data_ptr(), 1, ops._stream()),
                   "lbbnn_gate_members")
    return [b["w"] for b in bufs], [b["bias"] for b in bufs], splits


def _same_bits(a, b, split):
    """Bitwise equality of two operand buffers, a zero of either sign equal to a zero of the other (fp32 values, or the bf16
    halves of the split layout)."""
    ia, ib = (a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)) if split else \
             (a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    mag = 0x7FFF if split else 0x7FFFFFFF
    return bool(((ia == ib) | (((ia & mag) == 0) & ((ib & mag) == 0))).all())


def _head64(h, head):
    if head == "sigmoid":
        return torch.cat([torch.nn.functional.logsigmoid(-h), torch.nn.functional.logsigmoid(h)], dim=-1)
    return torch.log_softmax(h, dim=-1)


def _forward64(x, ws, bs, head):
    """fp64 forward on the CPU: relu(x W^T + b) per hidden layer, then the head's log-probabilities."""
    h = x.double().cpu()
    for k, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.double().cpu().t() + b.double().cpu()
        if k < len(ws) - 1:
            h = torch.relu(h)
    return _head64(h, head)


def _mean_weights64(net, gates, threshold=0.5):
    """The posterior-mean weights in fp64 from the parameters: alpha * mu, or the medimean's mu * [alpha > threshold]."""
    ws = []
    for l in net._layers():
        lam, mu = l.lambdal.detach().double().cpu(), l.weight_mu.detach().double().cpu()
        alpha = torch.sigmoid(lam)
        ws.append(alpha * mu if gates == "sample" else mu * (alpha > threshold))
    return ws, [l.bias_mu.detach() for l in net._layers()]


# ------------------------------------------------------------------------------------------- 1. the full model
@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("gates", GATES)
@pytest.mark.parametrize("case", CASES + HEAD_CASES, ids=IDS + HEAD_IDS)
def test_full_model_is_base_ensemble(bnn, dev, precision, case, gates, B):
    ev, ops = bnn.evaluate, bnn.ops
    dims, prec, head = case[:3]
    net = _net(bnn, dev, dims, head)
    precision(prec)
    mode = "mpm" if gates == "mpm" else "sample"
    _set_hard(net, gates == "sample-hard")
    try:
        binary = head == "sigmoid" if len(case) == 3 else case[3]       # (log_probs: the sigmoid head's 2-class form)
        x = _x(dev, B, dims[0])
        st = ops.RngState.get(dev)
        bnn.manual_seed(SEED, OFF)
        want = ev.base_ensemble(net, x, S, gates=mode, log_probs=binary)["outputs"]
        assert want.shape == (S, B, 2 if binary else dims[-1])
        bnn.manual_seed(SEED, OFF)
        w_loop, b_loop, splits = _loop_members(bnn, net, x, S, mode)
        fz = ev.freeze_base(net, mode)
        assert fz.gates == mode and fz.head == head and fz.dims == dims and fz.full_dims == dims and list(fz.parameters()) == []
        assert fz._split == splits
        if prec == "bf16x3" and case in CASES:
            assert splits == [True, True, False]                 # the split layout really is in play
        bnn.manual_seed(SEED, OFF)
        got = fz.ensemble(x, S, log_probs=binary, keep_weights=True)
        assert st.t[:2].tolist() == [SEED, OFF + S]              # the live offset advanced by the member count
        assert got.shape == want.shape and torch.equal(got, want)
        for k in range(len(dims) - 1):
            assert _same_bits(fz.last_weights[k], w_loop[k], splits[k]), k
            assert torch.equal(fz.last_biases[k], b_loop[k]), k
        bnn.manual_seed(SEED, OFF)
        chunked = fz.ensemble(x, S, max_members=2, log_probs=binary, keep_weights=True)
        assert torch.equal(chunked, want) and st.t[:2].tolist() == [SEED, OFF + S]
        for k in range(len(dims) - 1):
            assert _same_bits(fz.last_weights[k], w_loop[k], splits[k]), k
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(fz(x, sample=True, log_probs=binary), want[0])
        assert torch.equal(ev.ensemble_forward(fz, x, 2, log_probs=binary), want[1:3])      # offsets OFF + 1, OFF + 2
    finally:
        _set_hard(net, False)


@pytest.mark.parametrize("gates", ["sample", "mpm"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_posterior_mean_and_statistics(bnn, dev, precision, case, gates):
    ev, ops = bnn.evaluate, bnn.ops
    dims, prec, head = case
    net = _net(bnn, dev, dims, head)
    precision(prec)
    binary = head == "sigmoid"
    x = _x(dev, 70, dims[0])
    fz = ev.freeze_base(net, gates)
    st = ops.RngState.get(dev)
    bnn.manual_seed(SEED, OFF)
    got = fz(x, log_probs=binary)
    assert st.t[:2].tolist() == [SEED, OFF]                      # the mean forward draws nothing
    ws, bs = _mean_weights64(net, gates)
    ref = _forward64(x, ws, bs, head)
    err = rel_err(got, ref)
    print("posterior mean %s %s: rel_err %.3g (bar %.1g)" % (dims, gates, err, BAR[prec]))
    assert err < BAR[prec]
    if gates == "sample":
        loop = ev._base_mean_forward(net, x, binary)
        e2 = rel_err(got, loop)
        print("against _base_mean_forward: %.3g" % e2)
        assert e2 < 1e-6
    # statistics: the kernel's counts against the parameters
    n_w = sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
    alphas = [torch.sigmoid(l.lambdal.detach().double()) for l in net._layers()]
    kept = [int((a > 0.5).sum()) for a in alphas]
    assert fz.kept == kept and [int(k.numel()) for k in fz.kept_rows] == list(dims[1:])
    if gates == "mpm":
        assert fz.density == sum(kept) / n_w
    else:
        expected = float(sum(a.sum() for a in alphas)) / n_w
        assert abs(fz.density - expected) < 1e-6 * expected      # the EXPECTED density sum(alpha) / weights
    r = ev.ensemble_eval(fz, x, None, 2)
    assert bool((r["density"] == torch.tensor(fz.density, dtype=torch.float32)).all())


def test_refresh_equals_a_fresh_freeze(bnn, dev):
    ev = bnn.evaluate
    torch.manual_seed(5)
    net = bnn.base.BayesianNetwork((13, 9, 3), lambdal_init=(-2.0, 2.0)).to(dev).eval()
    x = _x(dev, 5, 13)
    for gates in ("sample", "mpm"):
        fz = ev.freeze_base(net, gates)
        ptrs = dict((k, v.data_ptr()) for k, v in fz.named_buffers())
        with torch.no_grad():
            for l in net._layers():
                for p in (l.weight_mu, l.weight_rho, l.lambdal, l.bias_mu, l.bias_rho):
                    p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(3)).to(dev) * 0.3)
        assert fz.refresh() is fz
        fresh = ev.freeze_base(net, gates)
        bufs, want = dict(fz.named_buffers()), dict(fresh.named_buffers())
        assert sorted(bufs) == sorted(want)
        for k in want:
            assert torch.equal(bufs[k], want[k]) and bufs[k].data_ptr() == ptrs[k], k          # the same buffers, re-taken
        bnn.manual_seed(SEED, OFF)
        a = fz.ensemble(x, S)
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(a, fresh.ensemble(x, S))
        bnn.manual_seed(SEED, OFF)
        assert torch.equal(a, ev.base_ensemble(net, x, S, gates=gates)["outputs"])


def test_a_copied_or_moved_model_addresses_its_own_buffers(bnn, dev):
    """The descriptors hold device addresses: a deep copy, or a model moved with .to(), must not go on addressing the buffers it
    was built with."""
    import copy
    ev = bnn.evaluate
    net = _net(bnn, dev, (13, 9, 3), "log_softmax")
    x = _x(dev, 5, 13)
    fz = ev.freeze_base(net, "mpm")
    bnn.manual_seed(SEED, OFF)
    want = fz.ensemble(x, S)
    twin = copy.deepcopy(fz)
    for i in range(2):
        getattr(fz, "w_mu_%d" % i).fill_(float("nan"))           # the original's planes are no longer usable
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(twin.ensemble(x, S), want)
    old = dict(twin.named_buffers())
    moved = twin.double().float()                                # every float buffer replaced (a cast leaves int32 ones in place)
    for k, b in moved.named_buffers():
        if b.is_floating_point():
            assert b.data_ptr() != old[k].data_ptr(), k
            old[k].fill_(float("nan"))                           # still alive: a stale address reads NaN, not freed memory
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(moved.ensemble(x, S), want)
    with pytest.raises(RuntimeError, match="data is on"):
        moved.cpu().ensemble(x, S)


# ------------------------------------------------------------------------------------------- 2-6. the compact model
FULL = (24, 16, 16, 5)
F0 = [1, 2, 7, 9, 10, 14, 17, 22]          # live input features: they straddle and partly fill the Philox quads 0 .. 5
N1 = [0, 1, 2, 4, 6, 7, 8, 10]             # needed units of hidden layer 1; unit 8 has no kept input
N2 = [0, 2, 4, 6, 11]                      # needed units of hidden layer 2: five, topped up to eight with dead units 1, 3, 5
LIVE = [F0, N1, [0, 1, 2, 3, 4, 5, 6, 11], [0, 1, 2, 3, 4]]
MU_SEED = 24                               # chosen on the CPU: of seeds 0 .. 59 the largest floor of _sensitivity on the
                                           # posterior-mean weights, 2.6e-4 at B = 70 and 3.1e-4 at B = 5 (most seeds
                                           # leave a hidden unit off for every row: floor 0)


def _fixture_masks():
    """The kept weights of the compact fixture, set by hand:
    - hidden-1 unit 3 has kept inputs but every consumer pruned; input feature 4 is kept by that unit alone;
    - hidden-1 unit 5 is consumed only by hidden-2 unit 9, which no output keeps (a dead unit's dead input);
    - hidden-1 unit 8 is needed (hidden-2 units 2 and 6 keep it) and has no kept input: it emits relu(bias);
    - hidden-2 units 1 and 3 are dead but keep inputs: they ride along as the top-up of the five needed units to eight."""
    k0, k1, k2 = torch.zeros(16, 24, dtype=torch.bool), torch.zeros(16, 16, dtype=torch.bool), torch.zeros(5, 16, dtype=torch.bool)
    rows0 = [u for u in N1 if u != 8]
    for i, u in enumerate(rows0):
        for f in (F0[i % 8], F0[(i + 3) % 8], F0[(i + 5) % 8]):
            k0[u, f] = True
    k0[7, F0[7]] = True                                           # (the seven rows above leave feature 22 to this one)
    k0[3, 4] = k0[3, 1] = True
    k0[5, 2] = k0[5, 20] = True
    for i, q in enumerate(N2):
        for c in (N1[(2 * i) % 8], N1[(2 * i + 1) % 8], N1[(i + 5) % 8]):
            k1[q, c] = True
    k1[9, 5] = k1[9, 0] = True
    k1[1, 0] = k1[3, 12] = True
    for c in range(5):
        for q in (N2[c], N2[(c + 1) % 5], N2[(c + 3) % 5]):
            k2[c, q] = True
    return [k0, k1, k2]


def _fixture_net(bnn, dev, seed=MU_SEED):
    """(24, 16, 16, 5) with the masks above as lambdal = +-3, weights of size 0.5 .. 1.5 with random signs and biases of
    0.1 .. 0.5, so that every kept weight on a path to an output moves the output (asserted by _sensitivity)."""
    if ("fixture", seed) not in _NETS:
        torch.manual_seed(31)
        net = bnn.base.BayesianNetwork(FULL)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for l, k in zip(net._layers(), _fixture_masks()):
                l.lambdal.copy_(torch.where(k, torch.tensor(3.0), torch.tensor(-3.0)))
                mag = 0.5 + torch.rand(l.weight_mu.shape, generator=g)
                l.weight_mu.copy_(mag * torch.where(torch.rand(l.weight_mu.shape, generator=g) < 0.35, -1.0, 1.0))
                l.bias_mu.copy_(0.1 + 0.4 * torch.rand(l.bias_mu.shape, generator=g))
        _NETS[("fixture", seed)] = net.to(dev).eval()
    return _NETS[("fixture", seed)]


def _active(masks):
    """Kept weights whose row and column are both needed: the ones an output depends on."""
    need = [torch.zeros(d, dtype=torch.bool) for d in FULL]
    for b, idx in enumerate([F0, N1, N2, list(range(5))]):
        need[b][idx] = True
    return [k & need[i + 1][:, None] & need[i][None, :] for i, k in enumerate(masks)]


def _sensitivity(x, ws, bs, ref):
    """The smallest movement of the fp64 output, as rel_err, when ONE active kept weight is scaled by 1 %."""
    moves = []
    for i, act in enumerate(_active(_fixture_masks())):
        for o, j in act.nonzero().tolist():
            w2 = [w.double().cpu().clone() for w in ws]
            w2[i][o, j] *= 1.01
            moves.append(rel_err(_forward64(x, w2, bs, "log_softmax"), ref))
    return min(moves), len(moves)


def _compact_pair(bnn, dev, x, **kw):
    ev = bnn.evaluate
    net = _fixture_net(bnn, dev)
    full, cp = ev.freeze_base(net, "mpm"), ev.freeze_base(net, "mpm", compact=True)
    bnn.manual_seed(SEED, OFF)
    out_f = full.ensemble(x, S, keep_weights=True, **kw)
    bnn.manual_seed(SEED, OFF)
    out_c = cp.ensemble(x, S, keep_weights=True, **kw)
    return net, full, cp, out_f, out_c


def test_compact_structure_comes_from_the_kernel_masks(bnn, dev):
    ev = bnn.evaluate
    net = _fixture_net(bnn, dev)
    masks = ev._base_keep_masks(net._layers(), 0.5)
    want = _fixture_masks()
    for k, w in zip(masks, want):
        assert k.dtype == torch.bool and torch.equal(k.cpu(), w)
    need, live = ev.live_structure(masks, 8)
    cp = ev.freeze_base(net, "mpm", compact=True)
    assert cp.compact and cp.full_dims == FULL and cp.dims == (8, 8, 8, 5) and cp.needed == [8, 8, 5, 5]
    for b in range(4):
        assert torch.equal(cp.live[b], live[b]) and cp.live[b].tolist() == LIVE[b], b
    act = _active(want)
    assert cp.active_kept == sum(int(a.sum()) for a in act)
    n_w = sum(FULL[i] * FULL[i + 1] for i in range(3))
    assert cp.active_density == cp.active_kept / n_w
    full = ev.freeze_base(net, "mpm")
    assert cp.density == full.density == sum(int(k.sum()) for k in want) / n_w
    for i in range(3):
        rows, cols = torch.tensor(LIVE[i + 1]), torch.tensor(LIVE[i])
        assert torch.equal(cp.kept_rows[i].cpu(), want[i][rows][:, cols].sum(1).int()), i
        assert torch.equal(full.kept_rows[i].cpu(), want[i].sum(1).int()), i
    with pytest.raises(NotImplementedError, match="freeze again"):
        cp.refresh()


@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_compact_members_are_the_full_models(bnn, dev, precision, prec, B):
    precision(prec)
    x = _x(dev, B, FULL[0])
    net, full, cp, out_f, out_c = _compact_pair(bnn, dev, x)
    assert not any(full._split) and not any(cp._split)            # (no layer of this fixture has more than 16 rows)
    # 2. weights and biases, bit for bit, at the full coordinates
    for i in range(3):
        rows, cols = torch.tensor(LIVE[i + 1], device=dev), torch.tensor(LIVE[i], device=dev)
        I = len(LIVE[i])
        wf, wc = full.last_weights[i], cp.last_weights[i]
        assert wc.shape == (S, len(LIVE[i + 1]), bnn.ops.operand_ld(I))
        assert torch.equal(wc[:, :, :I].contiguous().view(torch.int32), wf[:, rows][:, :, cols].contiguous().view(torch.int32)), i
        assert bool((wc[:, :, I:] == 0).all()) and bool((wf[:, :, FULL[i]:] == 0).all())
        assert torch.equal(cp.last_biases[i].view(torch.int32), full.last_biases[i][:, rows].contiguous().view(torch.int32)), i
        assert int((wc[:, :, :I] != 0).sum()) > 0
    # 3. both against the fp64 forward composed from the full model's member weights
    bar = BAR[prec]
    for m in range(S):
        ws = [full.last_weights[i][m][:, :FULL[i]] for i in range(3)]
        bs = [full.last_biases[i][m] for i in range(3)]
        ref = _forward64(x, ws, bs, "log_softmax")
        if m == 0:
            shift, n_act = _sensitivity(x, ws, bs, ref)
            print("sensitivity: %d active kept weights, smallest move %.3g (floor %.1g)" % (n_act, shift, 2 * bar))
            assert shift >= 2 * bar, shift                        # a test that cannot see a wrong weight proves nothing
        ef, ec = rel_err(out_f[m], ref), rel_err(out_c[m], ref)
        print("member %d: full %.3g compact %.3g (bar %.1g)" % (m, ef, ec, bar))
        assert ef < bar and ec < bar, (m, ef, ec)
    # chunks give the same bits
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(cp.ensemble(x, S, max_members=2), out_c)
    # 4. the medimean forward of both
    wm, bm = _mean_weights64(net, "mpm")
    ref = _forward64(x, wm, bm, "log_softmax")
    ef, ec = rel_err(full(x), ref), rel_err(cp(x), ref)
    print("medimean: full %.3g compact %.3g" % (ef, ec))
    assert ef < bar and ec < bar


def test_nan_filled_buffers(bnn, dev, monkeypatch):
    """5. Every buffer (planes, keep masks, member weights and biases, the gathered input, activations, outputs) is handed out
    full of NaN (integers: all ones): anything read without having been written would surface."""
    ev = bnn.evaluate
    x = _x(dev, 70, FULL[0])
    net, full0, cp0, clean_f, clean_c = _compact_pair(bnn, dev, x)
    clean_mean = cp0(x)
    small = _net(bnn, dev, (13, 9, 3), "log_softmax")
    xs = _x(dev, 5, 13)
    bnn.manual_seed(SEED, OFF)
    clean_s = ev.freeze_base(small, "sample").ensemble(xs, S)

    def nan_empty(*size, **kw):
        fill = float("nan") if kw.get("dtype", torch.float32).is_floating_point else 255
        return torch.full(*size, fill, **kw) if len(size) == 1 else torch.full(size, fill, **kw)
    monkeypatch.setattr(ev, "_empty", nan_empty)
    _, full, cp, out_f, out_c = _compact_pair(bnn, dev, x)
    for fz in (full, cp):
        for name, buf in fz.named_buffers():
            assert bool(torch.isfinite(buf.float()).all()), name
        for i in range(3):
            I = fz.dims[i]
            for plane in ("w_mu", "w_sigma", "e_w"):
                assert bool((getattr(fz, "%s_%d" % (plane, i))[:, I:] == 0).all()), (plane, i)
            assert bool(torch.isfinite(fz.last_weights[i]).all()) and bool((fz.last_weights[i][:, :, I:] == 0).all())
            assert bool(torch.isfinite(fz.last_biases[i]).all())
    assert bool(torch.isfinite(out_c).all()) and torch.equal(out_f, clean_f) and torch.equal(out_c, clean_c)
    assert torch.equal(cp(x), clean_mean)
    fs = ev.freeze_base(small, "sample")
    for i, I in enumerate((13, 9)):
        for plane in ("w_mu", "w_sigma", "alpha", "e_w"):
            p = getattr(fs, "%s_%d" % (plane, i))
            assert bool(torch.isfinite(p).all()) and bool((p[:, I:] == 0).all()), (plane, i)
    bnn.manual_seed(SEED, OFF)
    assert torch.equal(fs.ensemble(xs, S), clean_s)


@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
def test_graphed_eval_step(bnn, dev, compact):
    """6. Replays of make_graphed_eval_step give the eager results bitwise from the same offset, and the accumulator's totals are
    those of evaluate_batches over the same batches."""
    ev = bnn.evaluate
    net = _fixture_net(bnn, dev)
    fz = ev.freeze_base(net, "mpm", compact=compact)
    B, C, members = 40, FULL[-1], 4
    g = torch.Generator().manual_seed(4)
    data = [(torch.rand(B, FULL[0], generator=g).to(dev), torch.randint(0, C, (B,), generator=g).to(dev)) for _ in range(3)]
    acc_g = ev.EvalAccumulator(C, members, dev)
    step = bnn.graphs.make_graphed_eval_step(fz, data[0][0], data[0][1], members, acc_g)
    bnn.manual_seed(SEED, OFF)
    got = [{k: v.clone() for k, v in step(xb, yb).items()} for xb, yb in data]
    assert bnn.ops.RngState.get(dev).t[:2].tolist() == [SEED, OFF + 3 * members]
    acc_e = ev.EvalAccumulator(C, members, dev)
    bnn.manual_seed(SEED, OFF)
    for (xb, yb), rows_g in zip(data, got):
        rows_e = acc_e.update(fz.ensemble(xb, members), yb, fz(xb, sample=False))
        assert sorted(rows_e) == sorted(rows_g)
        for k in rows_e:
            assert torch.equal(rows_e[k], rows_g[k]), k
    assert torch.equal(acc_g._totals, acc_e._totals) and acc_g.updates == 3
    acc_b = ev.EvalAccumulator(C, members, dev)
    bnn.manual_seed(SEED, OFF)
    res = ev.evaluate_batches(fz, data, members, acc=acc_b)
    assert torch.equal(acc_b._totals, acc_g._totals) and res["rows"] == 3 * B


def test_members_entry_point_gate_rows_and_member_split(bnn, dev):
    """lbbnn_base_frozen_members called directly: gate_rows of hard gates are the exact counts of the member's nonzero gates, and
    a member count beyond what one launch spreads over gridDim.y (the in-kernel member loop) gives the bits of single calls."""
    from bnn_amd import _lib
    ev, ops = bnn.evaluate, bnn.ops
    net = _net(bnn, dev, (13, 9, 3), "log_softmax")
    _set_hard(net, True)
    try:
        fz = ev.freeze_base(net, "sample")
    finally:
        _set_hard(net, False)
    members, n = 5, 2
    f = dict(dtype=torch.float32, device=dev)
    w = [torch.full((members, fz.dims[i + 1], 32), float("nan"), **f) for i in range(n)]
    b = [torch.full((members, fz.dims[i + 1]), float("nan"), **f) for i in range(n)]
    gr = [torch.full((members, fz.dims[i + 1]), float("nan"), **f) for i in range(n)]
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    bnn.manual_seed(SEED, OFF)
    st = ops.RngState.get(dev)
    _lib.check(_lib.lib().lbbnn_base_frozen_members(fz._layer_descs, None, n, members, ops.GATES_SAMPLE, 0.5, arr(w), arr(b), arr(gr),
                                                    st.t.data_ptr(), 1, ops._stream()), "lbbnn_base_frozen_members")
    for i in range(n):
        I = fz.dims[i]
        mu = getattr(fz, "w_mu_%d" % i)[:, :I]
        assert bool(torch.isfinite(w[i]).all()) and bool((w[i][:, :, I:] == 0).all())
        open_gates = (w[i][:, :, :I] != 0).float().sum(2)                    # a hard gate is 0 or 1, and mu + sigma eps != 0
        assert bool((mu != 0).all()) and torch.equal(gr[i], open_gates), i
    # 700 members of the (3, 9) layer's rows: more than gridDim.y takes, so every wave loops over several members
    many = 700
    w2 = [torch.empty((many, fz.dims[i + 1], 32), **f) for i in range(n)]
    b2 = [torch.empty((many, fz.dims[i + 1]), **f) for i in range(n)]
    _lib.check(_lib.lib().lbbnn_base_frozen_members(fz._layer_descs, None, n, many, ops.GATES_SAMPLE, 0.5, arr(w2), arr(b2), None,
                                                    st.t.data_ptr(), 1, ops._stream()), "lbbnn_base_frozen_members")
    for i in range(n):
        assert torch.equal(w2[i][:members], w[i]) and torch.equal(b2[i][:members], b[i]), i
    assert st.t[:2].tolist() == [SEED, OFF]                                  # the entry point does not advance the state
