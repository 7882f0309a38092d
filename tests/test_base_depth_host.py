"""CPU tier of the baseline LBBNN at depth (base.BayesianNetwork of 1 to 16 layers): construction, seeded values, the calling
convention of ``forward``, the grouping of the batched evaluation launch, and the new C entry point lbbnn_fold_rows."""
import ctypes
import os

import pytest
import torch

NAMES = ("weight_mu", "weight_rho", "weight_a", "weight_b", "lambdal", "pa", "pb", "bias_mu", "bias_rho", "bias_a", "bias_b")


@pytest.fixture(scope="module")
def base():
    from bnn_amd import base
    return base


def _dims(n):
    return tuple(5 + (3 * i) % 7 for i in range(n))


# ---------------------------------------------------------------------------------------------------------- construction
@pytest.mark.parametrize("length", [2, 3, 5, 10, 17])
def test_layers_are_built_in_order(base, length):
    dims = _dims(length)
    net = base.BayesianNetwork(dims)
    n = length - 1
    layers = net._layers()
    assert len(layers) == n and net.dims == dims
    assert [name for name, _ in net.named_children()] == ["l%d" % (i + 1) for i in range(n)]
    for i, l in enumerate(layers):
        assert l is getattr(net, "l%d" % (i + 1))
        assert isinstance(l, base.BayesianLinear) and l.layer == 1
        assert (l.in_features, l.out_features) == (dims[i], dims[i + 1])
        assert tuple(l.weight_mu.shape) == (dims[i + 1], dims[i])
        assert l._layer_id == 32 + i
    assert list(net.state_dict()) == ["l%d.%s" % (i + 1, p) for i in range(n) for p in NAMES]


@pytest.mark.parametrize("length", [1, 18])
def test_other_lengths_are_refused(base, length):
    with pytest.raises(ValueError, match="1 to 16 layers"):
        base.BayesianNetwork(_dims(length))


def test_default_network_is_the_reference(base):
    net = base.BayesianNetwork()
    assert net.dims == (784, 400, 600, 10) and len(net._layers()) == 3
    assert list(net.state_dict()) == ["l%d.%s" % (i, p) for i in (1, 2, 3) for p in NAMES]


@pytest.mark.parametrize("dims", [(9, 7, 6, 4), (9, 7, 6, 8, 5, 4)], ids=["three", "five"])
def test_seeded_values_are_those_of_standalone_layers(base, dims):
    torch.manual_seed(1234)
    net = base.BayesianNetwork(dims)
    torch.manual_seed(1234)
    alone = [base.BayesianLinear(dims[i], dims[i + 1], 1) for i in range(len(dims) - 1)]
    for l, a in zip([getattr(net, "l%d" % (i + 1)) for i in range(len(alone))], alone):
        for p in NAMES:
            assert torch.equal(getattr(l, p), getattr(a, p)), p
        assert torch.equal(l.gammas, a.gammas) and torch.equal(l.alpha, a.alpha)


# ---------------------------------------------------------------------------------------------------------- forward
def _stubbed(base, dims):
    net = base.BayesianNetwork(dims)
    seen = []
    for k, l in enumerate(net._layers()):
        def fwd(x, *a, _k=k, _l=l, **kw):
            seen.append((_k, tuple(x.shape), a, kw))
            return torch.zeros(x.shape[0], _l.out_features)
        l.forward = fwd
    return net, seen


def test_forward_takes_gates_by_position_by_name_and_mixed(base):
    dims = (6, 5, 4, 3, 2, 2)
    net, seen = _stubbed(base, dims)
    n = 5
    g = [torch.full((1,), float(i)) for i in range(n)]
    x = torch.rand(3, 6)
    names = ["g%d" % (i + 1) for i in range(n)]
    calls = [lambda: net(x, *g), lambda: net(x, **dict(zip(names, g))), lambda: net(x, g[0], g[1], g3=g[2], g5=g[4], g4=g[3]),
             lambda: net.forward(x, g[0], g2=g[1], g3=g[2], g4=g[3], g5=g[4])]
    for call in calls:
        del seen[:]
        out = call()
        assert tuple(out.shape) == (3, 2)
        assert [s[0] for s in seen] == list(range(n))
        for k, shape, a, kw in seen:
            assert shape == (3, dims[k]) and not kw
            assert a[0] is g[k] and tuple(a[1:]) == (False, False)
    # None is a gate like any other (the posterior-mean forward)
    del seen[:]
    net(x, *[None] * n, sample=False)
    assert [s[2] for s in seen] == [(None, False, False)] * n


def test_forward_hands_sample_and_medimean_on(base):
    net, seen = _stubbed(base, (6, 5, 4, 3))
    g = [torch.zeros(1) for _ in range(3)]
    x = torch.rand(2, 6)
    for call, want in ((lambda: net(x, *g, True), (True, False)), (lambda: net(x, *g, True, True), (True, True)),
                       (lambda: net(x, *g, False, True), (False, True)), (lambda: net(x, *g, sample=True), (True, False)),
                       (lambda: net(x, g1=g[0], g2=g[1], g3=g[2], sample=True, medimean=False), (True, False)),
                       (lambda: net(x, *g, medimean=True), (False, True))):
        del seen[:]
        call()
        assert [tuple(s[2][1:]) for s in seen] == [want] * 3


def test_forward_refuses_a_wrong_number_of_gates(base):
    net, seen = _stubbed(base, (6, 5, 4, 3, 2))
    g = [torch.zeros(1) for _ in range(4)]
    x = torch.rand(2, 6)
    with pytest.raises(TypeError, match="missing g4"):
        net(x, g[0], g[1], g[2])                               # too few
    with pytest.raises(TypeError, match="missing g2"):
        net(x, g1=g[0], g3=g[2], g4=g[3])
    with pytest.raises(TypeError):
        net(x, *g, True, False, g[0])                          # too many
    with pytest.raises(TypeError, match="g5"):
        net(x, *g, g5=g[0])
    with pytest.raises(TypeError, match="twice"):
        net(x, g[0], g[1], g[2], g[3], g2=g[1])                # a duplicate
    with pytest.raises(TypeError, match="twice"):
        net(x, g[0], g1=g[0], g2=g[1], g3=g[2], g4=g[3])
    with pytest.raises(TypeError, match="multiple values for argument 'sample'"):
        net(x, *g, True, sample=False)                         # as a plain signature would refuse it
    with pytest.raises(TypeError, match="multiple values for argument 'medimean'"):
        net(x, *g, True, False, medimean=False)
    assert not seen                                            # nothing ran


# ---------------------------------------------------------------------------------------------------------- grouping
class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: lets the host side of a launch sequence run with the library replaced."""
    is_cuda = property(lambda self: True)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.mark.parametrize("n,groups", [(3, (3,)), (4, (4,)), (5, (4, 1)), (9, (4, 4, 1))])
def test_predict_members_groups_the_gate_launch(base, monkeypatch, n, groups):
    from bnn_amd import _lib, distributions, ops
    dims = tuple(8 + 4 * (i % 3) for i in range(n)) + (3,)
    net = base.BayesianNetwork(dims)
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_ptr", lambda t, name="tensor": None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    x = torch.rand(6, dims[0]).as_subclass(_OnDevice)
    rng = torch.tensor([7, 11], dtype=torch.int64)
    S = 3
    res, rows, kept = net._predict_members(x, rng, S, rows=True, keep_gates=True)
    assert tuple(res.shape) == (S, 6, 3) and len(rows) == n and len(kept) == n
    gm = [a for name, a in rec.calls if name == "lbbnn_gate_members"]
    mm = [a for name, a in rec.calls if name == "lbbnn_gemm_members_mean"]
    assert len(rec.calls) == len(gm) + len(mm)
    assert tuple(a[1] for a in gm) == groups
    first = 0
    for a in gm:
        descs, cnt = a[0], a[1]
        assert len(descs) == cnt <= _lib.MAX_LAYERS
        assert [descs[j].layer_id for j in range(cnt)] == [32 + first + j for j in range(cnt)]
        assert [(descs[j].O, descs[j].I) for j in range(cnt)] == [(dims[first + j + 1], dims[first + j]) for j in range(cnt)]
        # the same members, gate mode, temperature, Philox state and advance in every group
        assert a[2:] == (S, ops.GATES_SAMPLE, float(distributions.TEMPER_PRIOR), rng.data_ptr(), 1, 0)
        first += cnt
    assert first == n
    if n <= _lib.MAX_LAYERS:
        assert len(gm[0][0]) == n                              # one call over the network's whole descriptor array, as before
    # one GEMM per layer, in layer order, ReLU in every epilogue but the head's log_softmax
    assert len(mm) == n
    for k, a in enumerate(mm):
        B, I, O, flags, members = a[11:16]
        assert (B, I, O, members) == (6, dims[k], dims[k + 1], S)
        assert flags == (ops.F_RELU if k < n - 1 else ops.F_LOG_SOFTMAX)
    # the chain: every layer reads what the previous one wrote
    for k in range(1, n):
        assert mm[k][0] == mm[k - 1][8]


def test_operand_formats_in_the_second_group_under_a_split_precision(base, monkeypatch):
    """The per-layer operand-format rule at depth: under bf16x3 a layer takes the bf16 hi | lo operands exactly where the split
    kernels accept its shape (O > 16, I % 8 == 0, 8 spare columns) -- here layers 5 and 6, both in the SECOND group; the flag is
    on that group's descriptors and on those layers' GEMM calls, and nowhere else.  The first layer also needs aligned x rows."""
    import bnn_amd
    from bnn_amd import _lib, ops
    dims = (8, 8, 8, 8, 8, 24, 18, 3)                          # layers 5 (8 -> 24) and 6 (24 -> 18) are split-eligible
    want = [ops.split_eligible(dims[i], dims[i + 1]) for i in range(7)]
    assert want == [False, False, False, False, True, True, False]
    net = base.BayesianNetwork(dims)
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_ptr", lambda t, name="tensor": None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    x = torch.rand(6, dims[0]).as_subclass(_OnDevice)
    rng = torch.tensor([7, 11], dtype=torch.int64)
    for precision in ("bf16x3", "fp32"):
        bnn_amd.set_precision(precision)
        try:
            del rec.calls[:]
            net._predict_members(x, rng, 2)
        finally:
            bnn_amd.set_precision("fp32")
        split = [w and precision == "bf16x3" for w in want]
        gm = [a for name, a in rec.calls if name == "lbbnn_gate_members"]
        mm = [a for name, a in rec.calls if name == "lbbnn_gemm_members_mean"]
        assert [a[1] for a in gm] == [4, 3]
        flags = [gm[0][0][j].flags for j in range(4)] + [gm[1][0][j].flags for j in range(3)]
        assert flags == [ops.F_SPLIT16 if s else 0 for s in split], (precision, flags)
        for k, a in enumerate(mm):
            act = ops.F_RELU if k < 6 else ops.F_LOG_SOFTMAX
            assert a[14] == act | (ops.F_SPLIT16 if split[k] else 0), (precision, k)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("per_member", [False, True])
@pytest.mark.parametrize("form", ["dual", "mean"])
@pytest.mark.parametrize("C,head,head_flag", [(3, "log_softmax", 0x8), (18, "log_softmax", 0), (1, "sigmoid", 0),
                                              (3, "sigmoid", 0)])
def test_member_gemm_chain_wires_one_call_per_layer(monkeypatch, C, head, head_flag, form, per_member, wide):
    """ops.member_gemm_chain, the one place that wires a chain of member GEMMs: per layer ONE call of the form's entry point
    with the positional arguments the ensemble sites pass; member stride pad4(B * O) (B * O = 60, 100 and 15 / 90 / 5: the
    padding matters), or the row stride of a caller's wider last buffer; ReLU on every layer but the last, log_softmax in the
    last epilogue exactly for the log_softmax head with C <= 16; layer 0 reads x for every member (member stride 0); layer
    k + 1 reads what layer k wrote; the buffers in between come from the given allocator."""
    from bnn_amd import _lib, ops
    B, S, I0 = 5, 3, 8
    widths = (12, 20, C)
    dims = (I0,) + widths
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: 77)
    x = torch.rand(B, 12)[:, :I0]                               # rows wider than I0: ldx is the row stride
    lds = [ops.operand_ld(i) for i in dims[:3]]
    ws = [torch.zeros(((S,) if per_member else ()) + (dims[k + 1], lds[k])) for k in range(3)]
    mean_per_member = per_member and form == "mean"             # (the dual-moment form has one bias for all members)
    bs = [torch.zeros(((S,) if mean_per_member else ()) + (dims[k + 1],)) for k in range(3)]
    splits = [False, True, False]
    pad = [ops.pad4(B * o) for o in widths]
    assert pad[:2] == [60, 100] and pad[2] == {3: 16, 18: 92, 1: 8}[C] and pad[2] != B * C
    out = torch.zeros(S, pad[2] + (8 if wide else 0))
    handed = []

    def alloc(*size, **kw):
        handed.append(torch.empty(*size, **kw))
        return handed[-1]

    if form == "dual":
        vs, bvs = [torch.zeros(dims[k + 1], lds[k]) for k in range(3)], [torch.zeros(dims[k + 1]) for k in range(3)]
        rng = torch.tensor([7, 11], dtype=torch.int64)
        layers = [(ws[k], bs[k], splits[k], vs[k], bvs[k], 64 + k, 1000 * k) for k in range(3)]
        got = ops.member_gemm_chain(x, S, layers, head=head, out=out, empty=alloc, rng=rng, stream=5)
    else:
        layers = [(ws[k], bs[k], splits[k]) for k in range(3)]
        got = ops.member_gemm_chain(x, S, layers, head=head, out=out, empty=alloc)               # (the current stream)
    assert got is out
    name = "lbbnn_lrt_gemm_members" if form == "dual" else "lbbnn_gemm_members_mean"
    assert [c[0] for c in rec.calls] == [name] * 3
    assert [tuple(t.shape) for t in handed] == [(S, pad[0]), (S, pad[1])] and all(t.dtype == torch.float32 for t in handed)
    outs = [handed[0], handed[1], out]
    o_ms = [pad[0], pad[1], out.stride(0)]
    for k, (_, a) in enumerate(rec.calls):
        I, O = dims[k], dims[k + 1]
        src = (x.data_ptr(), 12, 0) if k == 0 else (outs[k - 1].data_ptr(), I, o_ms[k - 1])
        flags = (0x4 if splits[k] else 0) | (0x1 if k < 2 else head_flag)
        w_ms = O * lds[k] if per_member else 0
        if form == "dual":
            assert a == src + (ws[k].data_ptr(), w_ms, vs[k].data_ptr(), lds[k], bs[k].data_ptr(), bvs[k].data_ptr(),
                               rng.data_ptr(), 64 + k, 1000 * k, 1, outs[k].data_ptr(), O, o_ms[k], B, I, O, flags, S, 5)
        else:
            assert a == src + (ws[k].data_ptr(), w_ms, lds[k], bs[k].data_ptr(), O if per_member else 0,
                               outs[k].data_ptr(), O, o_ms[k], B, I, O, flags, S, 77)


def test_gate_members_refuses_more_than_one_group(base):
    """The entry point takes at most LBBNN_MAX_LAYERS descriptors: the grouping above is what keeps a deep network inside it."""
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    d = (_lib.GateMemberDesc * 5)()
    assert _lib.lib().lbbnn_gate_members(d, 5, 3, 0, 0.5, ctypes.c_void_p(4096), 1, None) == -2


# ---------------------------------------------------------------------------------------------------------- the new symbol
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_fold_rows_is_exported_bound_and_declared(lib):
    from bnn_amd import _lib
    assert hasattr(lib, "lbbnn_fold_rows")
    assert "lbbnn_fold_rows" in _lib.SIGNATURES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int lbbnn_fold_rows(" in open(os.path.join(root, "include", "lbbnn.h")).read()


def test_fold_rows_argument_checks(lib):
    """Every bad argument returns its code before anything is launched (the pointers are never dereferenced)."""
    fake = ctypes.c_void_p(4096)
    assert lib.lbbnn_fold_rows(None, 2, 5, 5, fake, None) == -1
    assert lib.lbbnn_fold_rows(fake, 2, 5, 5, None, None) == -1
    assert lib.lbbnn_fold_rows(fake, 0, 5, 5, fake, None) == -2
    assert lib.lbbnn_fold_rows(fake, 65, 5, 5, fake, None) == -2
    assert lib.lbbnn_fold_rows(fake, 2, 0, 5, fake, None) == -2
    assert lib.lbbnn_fold_rows(fake, 2, 65, 65, fake, None) == -2
    assert lib.lbbnn_fold_rows(fake, 2, 5, 4, fake, None) == -2                # ld < n
    assert lib.lbbnn_fold_rows(ctypes.c_void_p(4098), 2, 5, 5, fake, None) == -3
    assert lib.lbbnn_fold_rows(fake, 2, 5, 5, ctypes.c_void_p(4097), None) == -3


def test_ops_fold_rows_has_no_cpu_path():
    from bnn_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fold_rows(torch.zeros(2, 5), 2, 5)
