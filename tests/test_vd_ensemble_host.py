"""CPU tier of variational dropout's batched ensemble evaluation (include/lbbnn.h lbbnn_vd_gemm_members,
evaluate.vd_ensemble): the new entry point is exported and bound, its argument checks return the documented codes without
launching, vd.BNN builds at any depth from 1 to 16 layers (the default dims exactly as before), and the Python interface
rejects what it cannot run."""
import ctypes
import os

import pytest
import torch

NEW = ("lbbnn_vd_gemm_members",)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_new_symbol_exported_and_bound(lib):
    from bnn_amd import _lib, ops
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert len(_lib.SIGNATURES[n][1]) == 21
    assert callable(ops.vd_gemm_members)


def test_vd_gemm_members_argument_checks(lib):
    """Every bad argument returns its code before anything is launched (the pointers are never dereferenced)."""
    fake = ctypes.c_void_p(4096)
    B, I, O, ld = 8, 32, 24, 32
    ok = dict(x=fake, x_ms=0, rng=fake, o_ms=B * O, flags=0x1, members=3, fanout=1, B=B, ldx=I)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.lbbnn_vd_gemm_members(a["x"], a["ldx"], a["x_ms"], fake, fake, ld, fake, a["rng"], 48, 0, 4, fake, O,
                                         a["o_ms"], a["B"], I, O, a["flags"], a["members"], a["fanout"], None)
    # members outside 1..65535, fanout not 0 / 1
    assert call(members=0) == -2 and call(members=65536) == -2 and call(members=-1) == -2
    assert call(fanout=2) == -2 and call(fanout=-1) == -2
    # fan-out reads one input for every member
    assert call(x_ms=B * I) == -2 and call(x_ms=4) == -2
    # negative strides, member stride shorter than a member's output
    assert call(fanout=0, x_ms=-4) == -2 and call(o_ms=-4) == -2 and call(o_ms=B * O - 4) == -2
    # member strides must keep every member 16-B aligned
    assert call(fanout=0, x_ms=B * I + 2) == -3 and call(o_ms=B * O + 2) == -3
    # flags: RELU | SPLIT16 | SINGLE16 | HALF16 only (no mean-only form, no fused log_softmax, no fp16-scaled operands)
    for f in (0x2, 0x8, 0x40, 0x80, 0x100, 0x200, 0x1 | 0x100):
        assert call(flags=f) == -4, hex(f)
    assert call(flags=0x10) == -4                                   # SINGLE16 without SPLIT16
    assert call(flags=0x4 | 0x20) == -4                             # HALF16 without SINGLE16
    # in-kernel noise only: the Philox state is required
    assert call(rng=None) == -5
    # the split kernels address x through 32-bit buffer offsets
    big = 0x20000000
    assert call(flags=0x4, B=2, ldx=big, o_ms=2 * O) == -2
    assert call(flags=0x4, fanout=0, B=2, ldx=big, o_ms=2 * O) == -2
    # the shared checks of the GEMM (NULL pointers)
    assert call(x=None) == -1


def test_existing_members_entry_points_still_reject_unknown_flags(lib):
    fake = ctypes.c_void_p(4096)
    B, I, O, ld = 8, 32, 24, 32
    assert lib.lbbnn_lrt_gemm_members(fake, I, 0, fake, O * ld, fake, ld, fake, fake, fake, 0, 0, 1, fake, O, B * O,
                                      B, I, O, 0x100, 3, None) == -4
    assert lib.lbbnn_gemm_members_mean(fake, I, 0, fake, O * ld, ld, fake, O, fake, O, B * O, B, I, O, 0x100, 3, None) == -4


@pytest.mark.parametrize("dims", [(20, 7), (20, 16, 3), (50, 37, 29, 3), (64, 48, 40, 33, 24, 10)])
def test_bnn_any_depth_builds_with_the_right_shapes(dims):
    from bnn_amd import vd
    net = vd.BNN(dims)
    L = len(dims) - 1
    layers = net._layers()
    assert len(layers) == L
    assert sorted(k for k, _ in net.named_children()) == sorted("l%d" % (i + 1) for i in range(L))
    for i, l in enumerate(layers):
        assert l is getattr(net, "l%d" % (i + 1))
        assert (l.n, l.m) == (dims[i], dims[i + 1])
        assert tuple(l.theta.shape) == (dims[i], dims[i + 1])
        assert l._layer_id == 48 + i
    assert list(net.state_dict()) == ["l%d.theta" % (i + 1) for i in range(L)]


def test_bnn_depth_limits():
    from bnn_amd import vd
    assert len(vd.BNN((8,) * 17)._layers()) == 16
    assert vd.BNN((8,) * 17).l16._layer_id == 63
    for dims in ((784,), (), (8,) * 18):
        with pytest.raises(ValueError):
            vd.BNN(dims)


def test_bnn_default_dims_unchanged():
    """The default network: the same modules, state_dict keys, seeded initial values and stream ids as the four loose
    layers it was assembled from before."""
    from bnn_amd import vd
    dims = (784, 1200, 1200, 1200, 10)
    torch.manual_seed(11)
    ref = [vd.BayesianLayer(dims[i], dims[i + 1]) for i in range(4)]
    torch.manual_seed(11)
    net = vd.BNN()
    assert net.dims == dims
    assert list(net.state_dict()) == ["l1.theta", "l2.theta", "l3.theta", "l4.theta"]
    for i, (l, r) in enumerate(zip((net.l1, net.l2, net.l3, net.l4), ref)):
        assert torch.equal(l.theta, r.theta)
        assert torch.equal(l.alpha, r.alpha)
        assert l._layer_id == 48 + i
    assert [k for k, _ in net.named_children()] == ["l1", "l2", "l3", "l4"]


def test_python_interface_rejects_what_it_cannot_run():
    from bnn_amd import evaluate, vd
    torch.manual_seed(0)
    net = vd.BNN((20, 16, 12, 3))
    x = torch.rand(4, 20)
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.vd_ensemble(net, x, 3)                           # no quiet CPU fallback
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.ensemble_forward(net, x, 3, batched=True)
    with pytest.raises(RuntimeError):
        evaluate.ensemble_forward(net, x, 3)                      # the loop's forwards have no CPU path either
    with pytest.raises(ValueError):
        evaluate.ensemble_forward(net, x, 3, gates="mpm")         # the median probability model is the baseline's
    for bad in (0, -1):
        with pytest.raises(ValueError):
            evaluate.vd_ensemble(net, x, bad)
        with pytest.raises(ValueError):
            evaluate.ensemble_forward(net, x, bad)
        with pytest.raises(ValueError):
            evaluate.vd_ensemble(net, x, 3, max_members=bad)
        with pytest.raises(ValueError):
            evaluate.ensemble_forward(net, x, 3, max_members=bad)
    net.l2.noise = {"zeta": torch.zeros(4, 12)}
    with pytest.raises(ValueError):
        evaluate.ensemble_forward(net, x, 3, batched=True)        # injected noise: the loop only
    with pytest.raises(ValueError):
        evaluate.vd_ensemble(net, x, 3)
    with pytest.raises(ValueError):
        evaluate.vd_ensemble(torch.nn.Linear(20, 3), x, 3)
