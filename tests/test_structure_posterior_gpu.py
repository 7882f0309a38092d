"""GPU tier of the posterior over network structures (evaluate.structure_posterior, include/lbbnn.h lbbnn_gate_structure): every
output against the numpy reference (tests/structure_ref.py) on the kernels' own uniforms, exact integer equality throughout --
edge shapes with decided gates, the all-pruned and all-kept networks, the baseline family against the gates its ensemble
members really used, general alpha on LRT and planar-MNF networks, the RNG contract, graph capture, and the binomial bound on
the mean density."""
import numpy as np
import pytest
import torch

import structure_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _state(dev, seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


def _uniforms(bnn, dev, net, seed, offset, S):
    """Per layer the (S, O, I) uniforms of the gate draw, sample s at Philox offset + s (ops.philox_uniform)."""
    ops = bnn.ops
    return [torch.stack([ops.philox_uniform(_state(dev, seed, offset + s), ops.STREAM_GATE * 64 + l._layer_id,
                                            l.out_features, l.in_features) for s in range(S)]) for l in net._layers()]


def _decided_net(bnn, dev, dims, seed):
    """An LRT network whose lambdal is a random pattern of -40 / 0 / +40: alpha below every uniform, exactly 0.5 (a uniform
    (k + 0.5) 2^-24 never is), or exactly 1 -- every gate is decided without a rounding question."""
    net = bnn.lrt.BayesianNetwork(dims)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.copy_((torch.randint(0, 3, l.lambdal.shape, generator=g).float() - 1.0) * 40.0)
    return net.to(dev)


def _decided_gates(net, us):
    return [((l.lambdal.detach() > 20) | ((l.lambdal.detach() == 0) & (u < 0.5))).cpu().numpy() for l, u in zip(net._layers(), us)]


def _check(res, ref, S, keep_need=True):
    """Every output of structure_posterior against structure_ref's, exactly."""
    n = ref["kept"].shape[1]
    np_ = lambda t: t.cpu().numpy()
    assert res["kept"].dtype == res["needed"].dtype == res["active_kept"].dtype == res["feature_count"].dtype == torch.int32
    assert res["kept"].shape == (S, n) and res["needed"].shape == (S, n + 1) and res["active_kept"].shape == (S, n)
    assert np.array_equal(np_(res["kept"]), ref["kept"])
    assert np.array_equal(np_(res["needed"]), ref["needed"])
    assert np.array_equal(np_(res["active_kept"]), ref["active_kept"])
    assert np.array_equal(np_(res["feature_count"]), ref["feature_count"])
    assert len(res["unit_count"]) == len(res["unit_prob"]) == n - 1
    for b in range(n - 1):
        assert np.array_equal(np_(res["unit_count"][b]), ref["unit_count"][b]), b
        assert np.array_equal(np_(res["unit_prob"][b]), ref["unit_count"][b] / float(S))
    weights = float(sum(nd.shape[1] * ref["need"][b + 1].shape[1] for b, nd in enumerate(ref["need"][:-1])))
    assert res["density"].dtype == res["active_density"].dtype == res["feature_prob"].dtype == torch.float64
    assert np.array_equal(np_(res["density"]), ref["kept"].sum(1) / weights)
    assert np.array_equal(np_(res["active_density"]), ref["active_kept"].sum(1) / weights)
    assert np.array_equal(np_(res["feature_prob"]), ref["feature_count"] / float(S))
    if keep_need:
        assert len(res["need"]) == n + 1
        for b in range(n + 1):
            assert res["need"][b].dtype == torch.bool and np.array_equal(np_(res["need"][b]), ref["need"][b]), b
    else:
        assert "need" not in res


def _prefix(gates, S):
    return [g[:S] for g in gates]


SINGLE = [(I, O) for I in (1, 3, 4, 5, 63, 64, 65, 1025) for O in (1, 2, 17)]
MULTI = [(5, 3, 2), (65, 17, 4, 3), (4,) * 17, (4096, 2)]
EDGE_DIMS = [(I, O) for I, O in SINGLE] + MULTI


@pytest.mark.parametrize("dims", EDGE_DIMS, ids=lambda d: "-".join(map(str, d)) if len(d) < 8 else "%dx%d" % (len(d), d[0]))
def test_edge_shapes_decided_gates(bnn, dev, dims):
    net = _decided_net(bnn, dev, dims, seed=len(dims) * 1000 + dims[0])
    seed, off = 11, 1 << 33                                   # an offset past 32 bits: both key words carry it
    gates = _decided_gates(net, _uniforms(bnn, dev, net, seed, off, 8))
    for S in (1, 3, 8):
        ref = sr.structure_ref(_prefix(gates, S))
        _check(bnn.evaluate.structure_posterior(net, S, rng=_state(dev, seed, off), keep_need=True), ref, S)
    _check(bnn.evaluate.structure_posterior(net, 8, rng=_state(dev, seed, off)), sr.structure_ref(gates), 8, keep_need=False)


@pytest.mark.parametrize("dims", [(9, 5, 3), (6, 2)])
def test_all_pruned_and_all_kept(bnn, dev, dims):
    n, S = len(dims) - 1, 5
    weights = [dims[l] * dims[l + 1] for l in range(n)]
    net = bnn.lrt.BayesianNetwork(dims).to(dev)
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.fill_(-40.0)
    res = bnn.evaluate.structure_posterior(net, S, rng=_state(dev, 3, 0), keep_need=True)
    assert (res["kept"] == 0).all() and (res["active_kept"] == 0).all()
    assert (res["needed"][:, :n] == 0).all() and (res["needed"][:, n] == dims[-1]).all()
    assert (res["feature_prob"] == 0).all() and all((p == 0).all() for p in res["unit_prob"])
    assert res["need"][n].all() and not any(nd.any() for nd in res["need"][:n])
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.fill_(40.0)
    res = bnn.evaluate.structure_posterior(net, S, rng=_state(dev, 3, 0), keep_need=True)
    want = torch.tensor([weights] * S, dtype=torch.int32, device=dev)
    assert torch.equal(res["kept"], want) and torch.equal(res["active_kept"], want)
    assert torch.equal(res["needed"], torch.tensor([list(dims)] * S, dtype=torch.int32, device=dev))
    assert (res["feature_prob"] == 1).all() and (res["density"] == 1).all() and (res["active_density"] == 1).all()
    assert all(nd.all() for nd in res["need"])


def test_baseline_family_against_its_real_members(bnn, dev):
    """The structures are those of the very members base_ensemble draws from the same Philox state."""
    ops, ev = bnn.ops, bnn.evaluate
    dims, S = (24, 16, 16, 3), 6
    torch.manual_seed(5)
    net = bnn.base.BayesianNetwork(dims).to(dev)
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.uniform_(-2.5, 2.5)
            l.gamma.exact = True
    x = torch.rand(7, dims[0], generator=torch.Generator().manual_seed(1)).to(dev)
    ops.manual_seed(7, 100)
    members = ev.base_ensemble(net, x, S, keep_gates=True)
    gates = [g.cpu().numpy() for g in members["gates"]]
    assert all(((g == 0) | (g == 1)).all() for g in gates)
    ops.manual_seed(7, 100)
    res = ev.structure_posterior(net, S, keep_need=True)
    for l in range(len(dims) - 1):
        assert np.array_equal(res["kept"][:, l].cpu().numpy(), gates[l].sum(axis=(1, 2)).astype(np.int64)), l
        assert np.array_equal(res["kept"][:, l].cpu().numpy(), members["gate_rows"][l].sum(1).cpu().numpy().astype(np.int64)), l
    ref = sr.structure_ref([g > 0.5 for g in gates])
    _check(res, ref, S)
    assert 0 < ref["needed"][:, 0].min() and ref["needed"][:, 2].min() < dims[2]        # the case prunes something


# seeds of the general-alpha cases: with them no draw lies within 4 ulp of its alpha (found with tests/philox_ref.py on the
# CPU, asserted again below on the device's uniforms)
GENERAL = {"lrt": (21, 9, 500), "mnf": (22, 9, 500)}


def _general_net(bnn, family, dims, seed):
    torch.manual_seed(seed)
    if family == "lrt":
        net = bnn.lrt.BayesianNetwork(dims)
    else:
        net = bnn.mnf.BayesianNetwork(dims, 2, z_flow_type="Planar", r_flow_type="Planar")
    with torch.no_grad():
        for l in net._layers():
            l.lambdal.uniform_(-3.0, 3.0)
    return net


def _ambiguous(us, alphas):
    """Draws with |u - alpha| <= 4 ulp(alpha): a reference in another precision could decide them either way."""
    return sum(int((np.abs(u.astype(np.float64) - a[None]) <= 4.0 * np.spacing(a.astype(np.float32)).astype(np.float64)[None]).sum())
               for u, a in zip(us, alphas))


@pytest.mark.parametrize("family", sorted(GENERAL))
def test_general_alpha_against_fp64_sigmoid(bnn, dev, family):
    dims, S = (20, 8, 3), 8
    net_seed, seed, off = GENERAL[family]
    net = _general_net(bnn, family, dims, net_seed)
    alphas = [1.0 / (1.0 + np.exp(-l.lambdal.detach().numpy().astype(np.float64))) for l in net._layers()]
    # the CPU restatement of the draws agrees with the device's, and the seed leaves no draw ambiguous
    cpu_gates, _ = sr.gates_ref(alphas, [l._layer_id for l in net._layers()], seed, off, S)
    net = net.to(dev)
    us = [u.cpu().numpy() for u in _uniforms(bnn, dev, net, seed, off, S)]
    assert _ambiguous(us, alphas) == 0
    gates = [u.astype(np.float64) < a[None] for u, a in zip(us, alphas)]
    assert all(np.array_equal(g, c) for g, c in zip(gates, cpu_gates))
    ref = sr.structure_ref(gates)
    _check(bnn.evaluate.structure_posterior(net, S, rng=_state(dev, seed, off), keep_need=True), ref, S)
    assert ref["needed"][:, 1].min() < dims[1] or ref["kept"].min() < ref["kept"].max()


def _same(a, b):
    for k in ("kept", "needed", "active_kept", "feature_count", "density", "active_density", "feature_prob"):
        assert torch.equal(a[k], b[k]), k
    for k in ("unit_count", "unit_prob") + (("need",) if "need" in a else ()):
        assert len(a[k]) == len(b[k]) and all(torch.equal(p, q) for p, q in zip(a[k], b[k])), k


def test_reproducibility_and_rng_contract(bnn, dev):
    ops, ev = bnn.ops, bnn.evaluate
    net = _general_net(bnn, "lrt", (20, 8, 3), 21).to(dev)
    S, k = 7, 40
    ops.manual_seed(9, k)
    st = ops.RngState.get(dev)
    one = ev.structure_posterior(net, S, keep_need=True)
    assert st.t[:2].tolist() == [9, k + S]                    # the live offset advances by exactly S
    ops.manual_seed(9, k)
    _same(ev.structure_posterior(net, S, keep_need=True), one)             # the same state, the same bits
    for chunk in (1, 3):
        ops.manual_seed(9, k)
        _same(ev.structure_posterior(net, S, keep_need=True, max_members=chunk), one)
        assert st.t[:2].tolist() == [9, k + S]
    # an explicit state advances nothing, neither itself nor the live state; chunks walk a copy
    rng = _state(dev, 9, k)
    for chunk in (None, 1, 3):
        _same(ev.structure_posterior(net, S, rng=rng, keep_need=True, max_members=chunk), one)
        assert rng.tolist() == [9, k] and st.t[:2].tolist() == [9, k + S]
    # sample s of a call at offset k is sample 0 of a call at offset k + s
    for s in range(S):
        single = ev.structure_posterior(net, 1, rng=_state(dev, 9, k + s), keep_need=True)
        for key in ("kept", "needed", "active_kept"):
            assert torch.equal(single[key][0], one[key][s]), (key, s)
        assert all(torch.equal(p[0], q[s]) for p, q in zip(single["need"], one["need"]))
    assert not torch.equal(one["kept"][0], one["kept"][1])


def test_graph_capture(bnn, dev):
    ev = bnn.evaluate
    net = _general_net(bnn, "lrt", (20, 8, 3), 21).to(dev)
    rng = _state(dev, 9, 40)
    eager = ev.structure_posterior(net, 5, rng=rng, keep_need=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.structure_posterior(net, 5, rng=rng, keep_need=True)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ev.structure_posterior(net, 5, rng=rng, keep_need=True)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _same(out, eager)                                     # the totals are zeroed inside the graph: no accumulation


def test_statistics_are_sane(bnn, dev):
    dims, S = (64, 32, 4), 64
    net = bnn.lrt.BayesianNetwork(dims)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for l in net._layers():
            a = torch.rand(l.lambdal.shape, generator=g) * 0.96 + 0.02
            l.lambdal.copy_(torch.log(a / (1 - a)))
    net = net.to(dev)
    alpha = torch.cat([torch.sigmoid(l.lambdal.detach().double()).reshape(-1) for l in net._layers()])
    N = alpha.numel()
    res = bnn.evaluate.structure_posterior(net, S, rng=_state(dev, 2, 0))
    bound = 5.0 * float((alpha * (1 - alpha)).sum().sqrt()) / (N * S ** 0.5)               # the binomial bound; nothing is tuned
    diff = abs(float(res["density"].mean()) - float(alpha.mean()))
    print("mean density %.6f, mean alpha %.6f, |diff| %.3e, bound %.3e" % (float(res["density"].mean()), float(alpha.mean()), diff, bound))
    assert diff <= bound
    assert (res["feature_prob"] >= 0).all() and (res["feature_prob"] <= 1).all()
    assert (res["needed"][:, len(dims) - 1] == dims[-1]).all()
    assert (res["active_kept"] <= res["kept"]).all() and (res["active_density"] <= res["density"]).all()
