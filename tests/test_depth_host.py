"""CPU tier of LRT / MNF networks of any depth: the classes build l1 .. lN for 1 to 16 layers and refuse anything else, a
three-layer network is still constructed as before (seeded values, parameter names), the groups in which a deep network
issues its batched C calls, and the argument checks of lbbnn_kl_total (include/lbbnn.h)."""
import ctypes
import os

import pytest
import torch

E_NULL, E_SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def _make(family, dims):
    import bnn_amd
    if family == "lrt":
        return bnn_amd.lrt.BayesianNetwork(dims)
    return bnn_amd.mnf.BayesianNetwork(dims, 2, z_flow_type=family, r_flow_type=family)


def _dims(n):
    return (40,) + tuple((32, 24, 48, 40)[i % 4] for i in range(n - 1)) + (10,)


@pytest.mark.parametrize("n", [1, 2, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("family", ["lrt", "Planar", "RNVP"])
def test_layer_count_names_and_state_dict_keys(family, n):
    from bnn_amd import layers
    dims = _dims(n)
    net = _make(family, dims)
    assert net.dims == dims and layers.MAX_DEPTH == 16
    ls = net._layers()
    assert len(ls) == n and [name for name, _ in net.named_children()] == ["l%d" % (i + 1) for i in range(n)]
    assert not hasattr(net, "l%d" % (n + 1))
    for i, l in enumerate(ls):
        assert l is getattr(net, "l%d" % (i + 1))
        assert (l.in_features, l.out_features, l._layer_id) == (dims[i], dims[i + 1], i)
    keys = list(net.state_dict())
    assert {k.split(".")[0] for k in keys} == {"l%d" % (i + 1) for i in range(n)}
    for i in range(n):
        for name in ("weight_mu", "weight_rho", "lambdal", "bias_mu", "bias_rho"):
            assert "l%d.%s" % (i + 1, name) in keys
    assert keys == ["l%d.%s" % (i + 1, k) for i, l in enumerate(ls) for k in l.state_dict()]      # layer by layer, in order
    # the depth-generic helpers reach every layer
    net.set_precision("bf16x3")
    assert all(l.precision == "bf16x3" for l in ls)
    net.set_precision(None)
    net.set_row_offset(7)
    assert all(l.row_offset == 7 for l in ls)
    assert net.kl() == 0                                     # no forward yet: the sum of the layers' initial 0


@pytest.mark.parametrize("family", ["lrt", "Planar"])
@pytest.mark.parametrize("bad", [1, 18])
def test_other_lengths_raise_a_value_error_that_names_the_limits(family, bad):
    with pytest.raises(ValueError, match=r"1 to 16 layers \(len\(dims\) 2 to 17\)"):
        _make(family, tuple(range(8, 8 + bad)))


@pytest.mark.parametrize("family", ["lrt", "Planar", "RNVP"])
def test_three_layer_construction_order_is_three_stand_alone_layers(family):
    """The seeded initial values of a three-layer network are those of three stand-alone layers constructed in order after the
    same seed, key for key and bit for bit; the default dims are the reference's."""
    import bnn_amd
    dims = (20, 16, 12, 3)
    torch.manual_seed(0)
    net = _make(family, dims)
    torch.manual_seed(0)
    if family == "lrt":
        alone = [bnn_amd.lrt.BayesianLinear(i, o) for i, o in zip(dims[:-1], dims[1:])]
    else:
        alone = [bnn_amd.mnf.BayesianLinear(i, o, 2, z_flow_type=family, r_flow_type=family) for i, o in zip(dims[:-1], dims[1:])]
    want = {"l%d.%s" % (i + 1, k): v for i, l in enumerate(alone) for k, v in l.state_dict().items()}
    got = net.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert bnn_amd.lrt.BayesianNetwork().dims == (784, 400, 600, 10)
    assert [l._layer_id for l in net._layers()] == [0, 1, 2]


def test_layer_groups_and_group_slices():
    from bnn_amd import _lib
    assert _lib.MAX_LAYERS == 4 and _lib.MAX_DEPTH == 16
    assert _lib.layer_groups(1) == [(0, 1)] and _lib.layer_groups(3) == [(0, 3)] and _lib.layer_groups(4) == [(0, 4)]
    assert _lib.layer_groups(5) == [(0, 4), (4, 1)] and _lib.layer_groups(9) == [(0, 4), (4, 4), (8, 1)]
    assert _lib.layer_groups(16) == [(0, 4), (4, 4), (8, 4), (12, 4)]
    arr = (_lib.LayerDesc * 9)()
    for i in range(9):
        arr[i].O = 100 + i
    assert _lib.group_slice(arr, 0, 9) is arr                # one group: the very array, as before
    g = _lib.group_slice(arr, 4, 4)
    assert len(g) == 4 and [d.O for d in g] == [104, 105, 106, 107]
    assert ctypes.addressof(g) == ctypes.addressof(arr) + 4 * ctypes.sizeof(_lib.LayerDesc)     # a view, not a copy
    g[0].I = 55
    assert arr[4].I == 55


def test_kl_total_exported_bound_and_argument_checks(lib):
    from bnn_amd import _lib
    assert hasattr(lib, "lbbnn_kl_total") and "lbbnn_kl_total" in _lib.SIGNATURES
    assert lib.lbbnn_abi_version() == 1
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call fails before launching
    fn = lib.lbbnn_kl_total
    assert fn(None, 1, fake, None) == E_NULL
    assert fn(fake, 1, None, None) == E_NULL
    assert fn(None, 1, None, None) == E_NULL
    assert fn(fake, 0, fake, None) == E_SHAPE
    assert fn(fake, -1, fake, None) == E_SHAPE
    assert fn(fake, _lib.MAX_DEPTH + 1, fake, None) == E_SHAPE


def test_freeze_refuses_more_than_max_depth_layers():
    from bnn_amd import evaluate, _lib
    class L:                                                 # what _check_freezable_layers reads of a layer
        noise, as_written, _mnf = None, False, False
    evaluate._check_freezable_layers([L()] * _lib.MAX_DEPTH)
    with pytest.raises(ValueError, match="at most 16 layers"):
        evaluate._check_freezable_layers([L()] * (_lib.MAX_DEPTH + 1))
