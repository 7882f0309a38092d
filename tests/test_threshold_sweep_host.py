"""CPU tier of the threshold sweep (evaluate.threshold_sweep / ThresholdSweep / sweep_batches; include/lbbnn.h
lbbnn_sparse_count_levels / lbbnn_sparse_pack_levels / lbbnn_sparse_layer_levels): the reference inputs' own assertions on every
case and threshold set, every argument check of the new entry points (nothing is launched), the descriptor's layout, and every
refusal that needs no device."""
import ctypes
import os
import subprocess

import pytest
import torch

import threshold_sweep_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_F = ctypes.c_void_p(4096)            # never dereferenced
_ODD = ctypes.c_void_p(4098)          # off 4 bytes
_RELU, _MEAN, _LSM = 0x1, 0x2, 0x8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


# --------------------------------------------------------------------------- the reference inputs
@pytest.mark.parametrize("name", sorted(tr.SETS))
@pytest.mark.parametrize("case", tr.CASES, ids=tr.IDS)
def test_reference_lambdals_hold_their_rules(case, name):
    _, dims, _, _ = case
    thresholds, span, empty_last = tr.SETS[name]
    lams, masks = tr.lambdals(dims, thresholds, span=span, empty_last=empty_last)     # (asserts the module docstring's rules)
    assert len(masks) == len(thresholds) and all(len(m) == len(dims) - 1 for m in masks)
    totals = [sum(int(k.sum()) for k in m) for m in masks]
    assert all(a >= b for a, b in zip(totals, totals[1:])) and totals[0] > 0          # nested levels
    assert (totals[-1] == 0) == empty_last
    if name == "sixteen":
        assert len(thresholds) == 16 and abs(thresholds[0] - 0.05) < 1e-12 and abs(thresholds[-1] - 0.95) < 1e-12
        assert len(set(totals)) == 16                                                 # sixteen different models


def test_reference_lambdals_row_three_counts():
    """The row that is one past a wave, one past a chunk and exactly a chunk, spelled out for the first layer of (100, 20, 1)."""
    lams, masks = tr.lambdals((100, 20, 1), (0.3, 0.5, 0.9, 0.99), span=3.0, empty_last=True)
    assert [int(masks[j][0][3].sum()) for j in range(4)] == [65, 9, 8, 0]
    assert [int(masks[j][0][2].sum()) for j in range(4)] == [1, 0, 0, 0]
    assert [int(masks[j][0][1].sum()) for j in range(4)] == [100, 100, 100, 0]
    assert int(masks[0][1].sum()) > 0 and int(masks[3][1].sum()) == 0        # the one-row layer keeps its random row


# --------------------------------------------------------------------------- argument checks: nothing is launched
def _desc(**kw):
    from bnn_amd import _lib
    d = (_lib.SparseLevelsDesc * 5)()
    base = dict(weight_mu=4096, weight_rho=4096, lambdal=4096, bias_rho=4096, row_ptr=4096, col=4096, mean=4096, var=4096,
                bias_var=4096, kept_rows=4096, O=4, I=8, nnz=5, levels=3, cut=(-1.0, 0.0, 2.0))
    for k, v in dict(base, **kw).items():
        if k == "cut":
            for j, c in enumerate(v):
                d[0].cut[j] = c
        else:
            setattr(d[0], k, v)
    return d


def test_count_and_pack_levels_argument_checks(lib):
    for fn in (lib.lbbnn_sparse_count_levels, lib.lbbnn_sparse_pack_levels):
        assert fn(None, 1, None) == -1
        assert fn(_desc(), 0, None) == -2
        assert fn(_desc(), 5, None) == -2                     # more than LBBNN_MAX_LAYERS
        assert fn(_desc(lambdal=None, O=0), 1, None) == -1    # NULL before shape
        assert fn(_desc(O=0, lambdal=4098), 1, None) == -2    # shape before alignment
        assert fn(_desc(I=0), 1, None) == -2
        assert fn(_desc(levels=0), 1, None) == -2
        assert fn(_desc(levels=17), 1, None) == -2            # more than LBBNN_MAX_LEVELS
        assert fn(_desc(levels=-1, lambdal=4098), 1, None) == -2
        assert fn(_desc(cut=(0.0, 0.0, 2.0)), 1, None) == -2  # not strictly ascending
        assert fn(_desc(cut=(0.0, -1.0, 2.0)), 1, None) == -2
        assert fn(_desc(cut=(0.0, 1.0, float("inf"))), 1, None) == -2
        assert fn(_desc(cut=(float("nan"), 1.0, 2.0)), 1, None) == -2
        assert fn(_desc(cut=(0.0, float("nan"), 2.0), lambdal=4098), 1, None) == -2
        assert fn(_desc(levels=1, cut=(float("-inf"),)), 1, None) == -2
        assert fn(_desc(lambdal=4098), 1, None) == -3
    assert lib.lbbnn_sparse_count_levels(_desc(kept_rows=None), 1, None) == -1
    assert lib.lbbnn_sparse_count_levels(_desc(kept_rows=4098), 1, None) == -3
    for name in ("weight_mu", "weight_rho", "bias_rho", "row_ptr", "bias_var", "col", "mean", "var"):
        assert lib.lbbnn_sparse_pack_levels(_desc(**{name: None}), 1, None) == -1, name
        assert lib.lbbnn_sparse_pack_levels(_desc(**{name: 4098}), 1, None) == -3, name
    assert lib.lbbnn_sparse_pack_levels(_desc(nnz=-1), 1, None) == -2


def test_levels_desc_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    D = _lib.SparseLevelsDesc
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%zu %%zu %%zu %%d\\n", '
                   'sizeof(lbbnn_sparse_levels_desc_t), offsetof(lbbnn_sparse_levels_desc_t, kept_rows), '
                   'offsetof(lbbnn_sparse_levels_desc_t, nnz), offsetof(lbbnn_sparse_levels_desc_t, levels), '
                   'offsetof(lbbnn_sparse_levels_desc_t, cut), LBBNN_MAX_LEVELS); return 0; }\n'
                   % os.path.join(ROOT, "include", "lbbnn.h"))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, kept, nnz, levels, cut, max_levels = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                                        text=True).stdout.split())
    assert max_levels == _lib.MAX_LEVELS == 16
    assert ctypes.sizeof(D) == size
    assert (D.kept_rows.offset, D.nnz.offset, D.levels.offset, D.cut.offset) == (kept, nnz, levels, cut)
    assert D.cut.size == 4 * max_levels


_LAYER = dict(row_ptr=_F, col=_F, mean=_F, var=_F, nnz=5, bias_mu=_F, bias_var=_F, a=_F, lda=64, a_mstride=0, z=None,
              z_mstride=0, rng=_F, rng_stream=0, row_offset=0, member_advance=1, out=_F, ldo=64, o_mstride=4 * 64, out_rows=0,
              B=3, I=8, O=4, flags=0, levels=3, members_per_level=2)
# in the order of the checks; every row but the first of a code is also invalid at a LATER check
_LAYER_ROWS = [
    (dict(B=0, row_ptr=None, levels=0), 0),                            # an empty batch: nothing to do
    (dict(row_ptr=None, levels=0), -1), (dict(bias_mu=None), -1), (dict(bias_var=None), -1), (dict(a=None), -1), (dict(out=None), -1),
    (dict(col=None, I=0), -1), (dict(mean=None), -1), (dict(var=None), -1),
    (dict(levels=0, flags=0x100), -2), (dict(levels=17), -2), (dict(levels=-1), -2),
    (dict(members_per_level=0), -2), (dict(members_per_level=-3), -2),
    (dict(levels=16, members_per_level=4096), -2),                     # 65536 members
    (dict(levels=1, members_per_level=65536), -2),
    (dict(levels=3, members_per_level=21846), -2),                     # 65538 members
    (dict(B=-1, flags=0x100), -2), (dict(B=65535 * 64 + 1, lda=1 << 23, ldo=1 << 23), -2), (dict(I=0), -2), (dict(O=0), -2),
    (dict(nnz=-1, col=None), -2),
    (dict(lda=2), -2), (dict(ldo=2), -2), (dict(out_rows=1, ldo=3, flags=_LSM), -2),
    (dict(a_mstride=-1), -2), (dict(z_mstride=-1), -2), (dict(o_mstride=-1), -2),
    (dict(o_mstride=3 * 64 + 2), -2), (dict(out_rows=1, ldo=4, o_mstride=11), -2),
    (dict(members_per_level=1, o_mstride=3 * 64 + 2), -2),             # the levels of ONE draw still write apart
    (dict(a_mstride=7 * 64 + 2), -2), (dict(z=_F, z_mstride=7), -2),
    (dict(flags=0x100, rng=None), -4), (dict(flags=0x4), -4),
    (dict(flags=_LSM, rng=None), -4),                                  # log_softmax into a transposed output
    (dict(flags=_LSM | _RELU, out_rows=1, ldo=4, o_mstride=12), -4),
    (dict(flags=_LSM, out_rows=1, O=17, ldo=17, o_mstride=64), -4),
    (dict(rng=None, a=_ODD), -5),
    (dict(row_ptr=_ODD), -3), (dict(col=_ODD), -3), (dict(mean=_ODD), -3), (dict(var=_ODD), -3), (dict(bias_mu=_ODD), -3),
    (dict(bias_var=_ODD), -3), (dict(a=_ODD), -3), (dict(z=_ODD, z_mstride=8), -3), (dict(out=_ODD), -3),
    (dict(rng=ctypes.c_void_p(4100)), -3),
    (dict(members_per_level=1, z=_F, z_mstride=0, out=_ODD), -3),      # one draw: its z needs no member stride
    (dict(levels=16, members_per_level=4095, out=_ODD), -3),           # 65520 members are taken
]


@pytest.mark.parametrize("change,code", _LAYER_ROWS, ids=[str(i) for i in range(len(_LAYER_ROWS))])
def test_sparse_layer_levels_argument_checks(lib, change, code):
    assert not set(change) - set(_LAYER), change
    assert lib.lbbnn_sparse_layer_levels(*dict(_LAYER, **change).values(), None) == code, change


def test_the_plain_layer_entry_point_keeps_its_checks(lib):
    """lbbnn_sparse_layer_members shares the argument checks: members is its own count, whatever a sweep's limits are."""
    plain = dict((k, v) for k, v in _LAYER.items() if k not in ("levels", "members_per_level"))
    f = lib.lbbnn_sparse_layer_members
    assert f(*dict(plain, out=_ODD).values(), 65535, None) == -3        # 65535 members pass the shape checks
    assert f(*plain.values(), 65536, None) == -2 and f(*plain.values(), 0, None) == -2
    assert f(*dict(plain, z=_F, z_mstride=7).values(), 2, None) == -2
    assert f(*dict(plain, z=_F, z_mstride=7, out=_ODD).values(), 1, None) == -3


# --------------------------------------------------------------------------- refusals that need no device
def test_threshold_arguments(bnn):
    ev = bnn.evaluate
    net = bnn.lrt.BayesianNetwork((20, 16, 12, 3))
    with pytest.raises(ValueError, match="1 to 16 thresholds, got 0"):
        ev.threshold_sweep(net, ())
    with pytest.raises(ValueError, match="1 to 16 thresholds, got 17"):
        ev.threshold_sweep(net, tuple(0.05 * k for k in range(1, 18)))
    for bad in ((0.0, 0.5), (0.5, 1.0), (-0.1,), (1.5,)):
        with pytest.raises(ValueError, match="threshold must lie strictly between 0 and 1"):
            ev.threshold_sweep(net, bad)
    for bad in ((0.5, 0.5), (0.9, 0.5), (0.3, 0.9, 0.5)):
        with pytest.raises(ValueError, match="ascend strictly"):
            ev.threshold_sweep(net, bad)
    # ascending doubles whose logits round to one fp32 number: they would be the same level twice
    a, b = 0.9, 0.9 + 1e-10
    assert a < b and ev._cut(a) == ev._cut(b)
    with pytest.raises(ValueError, match="same fp32 cut"):
        ev.threshold_sweep(net, (0.5, a, b))


def test_threshold_sweep_refusals(bnn):
    ev = bnn.evaluate
    for net in (bnn.lrt.BayesianNetwork((20, 16, 12, 3)),
                bnn.mnf.BayesianNetwork((20, 16, 12, 3), 2, z_flow_type="Planar", r_flow_type="Planar")):
        with pytest.raises(RuntimeError, match="threshold_sweep needs the network on a HIP device"):   # said before any launch
            ev.threshold_sweep(net)
        net._layers()[1].as_written = True
        with pytest.raises(ValueError, match="layer 2 has as_written set"):
            ev.threshold_sweep(net, (0.5, 0.9))
        net._layers()[1].as_written = False
        net._layers()[0].noise = {"eps_out": torch.zeros(1, 16)}
        with pytest.raises(ValueError, match="layer 1 has injected noise"):
            ev.threshold_sweep(net, (0.5, 0.9))
    dense = bnn.mnf.BayesianNetwork((20, 16, 12, 3), 2)              # the reference's default: dense coupling z flows
    if dense.l1._check_flows() == "dense":
        with pytest.raises(ValueError, match=r"not built for dense coupling z flows.*freeze\(net, \"mpm\", threshold=t, dense=True\)"):
            ev.threshold_sweep(dense)
    with pytest.raises(TypeError, match=r"baseline.*freeze_base\(net, \"mpm\", threshold=t, sparse=True\)"):
        ev.threshold_sweep(bnn.base.BayesianNetwork((20, 16, 3)))
    with pytest.raises(TypeError, match=r"variational-dropout.*vd_ensemble"):
        ev.threshold_sweep(bnn.vd.BNN((20, 16, 3)))
    with pytest.raises(TypeError, match="lrt.BayesianNetwork or mnf.BayesianNetwork, got Linear"):
        ev.threshold_sweep(torch.nn.Linear(3, 3))


def test_sweep_class_and_sweep_batches_arguments(bnn):
    ev = bnn.evaluate
    sw = ev.ThresholdSweep((20, 16, 3), (0.5, 0.9), "lrt")
    assert isinstance(sw, torch.nn.Module) and not ev._is_frozen(sw) and list(sw.parameters()) == []
    assert sw.thresholds == (0.5, 0.9) and sw.cuts == (ev._cut(0.5), ev._cut(0.9)) and sw.cuts[0] == 0.0
    assert sw.kept.shape == (2, 2) and sw.kept.dtype == torch.int64 and sw.density.dtype == torch.float64
    assert bnn.ThresholdSweep is ev.ThresholdSweep and bnn.threshold_sweep is ev.threshold_sweep
    assert bnn.sweep_batches is ev.sweep_batches
    with pytest.raises(RuntimeError, match="not bound to a network"):
        sw.model(0)
    with pytest.raises(IndexError, match="no level 2"):
        sw.model(2)
    with pytest.raises(ValueError, match="at most 16 output units"):
        ev.ThresholdSweep((20, 17), (0.5,), "lrt", head="sigmoid")
    with pytest.raises(TypeError, match="sweep_batches takes a ThresholdSweep"):
        ev.sweep_batches(ev.SparseFrozenNetwork((20, 16, 3), "lrt", 0.9), [])
    with pytest.raises(ValueError, match=r"one accumulator per threshold \(2\), got 1"):
        ev.sweep_batches(sw, [], accs=[object()])
    with pytest.raises(ValueError, match="got no batches and no accumulators"):
        ev.sweep_batches(sw, [])
    with pytest.raises(ValueError, match=r"head='log_softmax' sweep takes EvalAccumulators, got \['object'\]"):
        ev.sweep_batches(sw, [], accs=[object(), object()])
    reg = ev.ThresholdSweep((8, 32, 2), (0.5, 0.9), "mnf", head="identity")
    with pytest.raises(ValueError, match=r"head=\"identity\" \(regression\): accs must be 2 evaluate.RegressionAccumulator, got None"):
        ev.sweep_batches(reg, [])
    with pytest.raises(ValueError, match=r"accs must be 2 evaluate.RegressionAccumulator, got \['object'\]"):
        ev.sweep_batches(reg, [], accs=[object(), object()])
    multi = ev.ThresholdSweep((20, 16, 3), (0.5,), "lrt", head="sigmoid")
    with pytest.raises(ValueError, match="sigmoid head with ONE output unit"):
        ev.sweep_batches(multi, [])
