"""CPU tier of the sparse median-probability model (evaluate.freeze(net, "mpm", sparse=True); include/lbbnn.h
lbbnn_sparse_count / lbbnn_sparse_pack / lbbnn_frozen_members_z / lbbnn_sparse_layer_members): the reference CSR builder
against brute force on the case networks, the exclusive scan, the fp64 CSR forward against the oracle's dense forward, every
argument check of the new entry points (nothing is launched), the descriptor's layout, and every refusal of freeze that
needs no device."""
import ctypes
import os
import subprocess

import pytest
import torch

import frozen_sparse_ref as sr
from oracle import lbbnn_oracle as orc

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


# --------------------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("case", sr.CASES, ids=sr.IDS)
def test_reference_csr_against_brute_force(case, threshold):
    _, dims, _, _ = case
    lams, masks = sr.lambdals(dims, threshold)               # (asserts the structural facts and the densities)
    cut = sr.cut_of(threshold)
    for lam, keep in zip(lams, masks):
        if lam.numel() > 50000:
            lam = lam[:40, :]                                # the big layers: their first rows carry every special row
        row_ptr, col, k = sr.csr_of(lam, cut)
        rp2, col2 = sr.csr_brute(lam, cut)
        assert row_ptr.dtype == col.dtype == torch.int32
        assert torch.equal(row_ptr, rp2) and torch.equal(col, col2)
        assert torch.equal(row_ptr, sr.exclusive_scan(k.sum(1)))
        for o in range(lam.shape[0]):
            c = col[row_ptr[o]:row_ptr[o + 1]]
            assert bool((c[1:] > c[:-1]).all())              # ascending within a row
        assert torch.equal(sr.decode(row_ptr, col, torch.ones(col.numel()), *lam.shape).bool(), k)


def test_reference_csr_never_keeps_nan():
    lam = torch.tensor([[float("nan"), 1.0, -1.0], [0.0, float("nan"), 2.0]])
    row_ptr, col, _ = sr.csr_of(lam, 0.0)
    assert row_ptr.tolist() == [0, 1, 2] and col.tolist() == [1, 2]


def test_exclusive_scan(bnn):
    for kept in ([0, 3, 0, 65, 1], [0], [7], [0, 0, 0]):
        k = torch.tensor(kept, dtype=torch.int32)
        rp = bnn.ops.sparse_row_ptr(k)
        assert rp.dtype == torch.int32 and rp.shape == (len(kept) + 1,)
        assert torch.equal(rp, sr.exclusive_scan(k))
        assert int(rp[0]) == 0 and int(rp[-1]) == sum(kept)
    assert [bnn.ops.sparse_row_pad(b) for b in (1, 64, 65, 257, 4096)] == [64, 64, 128, 320, 4096]


@pytest.mark.parametrize("stochastic", [True, False])
def test_reference_csr_forward_equals_the_oracles_dense_forward(stochastic):
    """member_from_csr against oracle.lrt_forward with lambdal = +-1000 (fp64 alpha exactly 1 / 0), in float64."""
    dims = (50, 37, 29, 3)
    lams, masks = sr.lambdals(dims, 0.5)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(9, dims[0], generator=g, dtype=torch.float64)
    h, layers = x, []
    for i, (lam, keep) in enumerate(zip(lams, masks)):
        O, I = lam.shape
        p = {"weight_mu": torch.randn(O, I, generator=g, dtype=torch.float64), "weight_rho": torch.randn(O, I, generator=g, dtype=torch.float64) - 3,
             "bias_mu": torch.randn(O, generator=g, dtype=torch.float64), "bias_rho": torch.randn(O, generator=g, dtype=torch.float64) - 3,
             "lambdal": torch.where(keep, 1000.0, -1000.0).double()}
        eps = torch.randn(9, O, generator=g, dtype=torch.float64)
        h, _, _ = orc.lrt_forward(h, p, eps if stochastic else None, stochastic=stochastic, compute_kl=False)
        if i < 2:
            h = torch.relu(h)
        row_ptr, col, _ = sr.csr_of(lam, 0.0)
        layers.append({"row_ptr": row_ptr, "col": col, "mean": p["weight_mu"][keep], "var": orc.sigma_of(p["weight_rho"])[keep] ** 2,
                       "bias_mu": p["bias_mu"], "bias_var": orc.sigma_of(p["bias_rho"]) ** 2, "z": None, "eps": eps})
    ref = torch.log_softmax(h, dim=1)
    out = sr.member_from_csr(x, layers, stochastic=stochastic)
    assert float((out - ref).abs().max()) < 1e-12


# --------------------------------------------------------------------------- argument checks: nothing is launched
def _desc(**kw):
    from bnn_amd import _lib
    d = (_lib.SparseDesc * 5)()
    base = dict(weight_mu=4096, weight_rho=4096, lambdal=4096, bias_rho=4096, row_ptr=4096, col=4096, mean=4096, var=4096,
                bias_var=4096, kept_rows=4096, O=4, I=8, nnz=5, cut=0.0)
    for k, v in dict(base, **kw).items():
        setattr(d[0], k, v)
    return d


def test_sparse_count_and_pack_argument_checks(lib):
    for fn in (lib.lbbnn_sparse_count, lib.lbbnn_sparse_pack):
        assert fn(None, 1, None) == -1
        assert fn(_desc(), 0, None) == -2
        assert fn(_desc(), 5, None) == -2                     # more than LBBNN_MAX_LAYERS
        assert fn(_desc(lambdal=None, O=0), 1, None) == -1    # NULL before shape
        assert fn(_desc(O=0, lambdal=4098), 1, None) == -2    # shape before alignment
        assert fn(_desc(I=0), 1, None) == -2
        assert fn(_desc(lambdal=4098), 1, None) == -3
    assert lib.lbbnn_sparse_count(_desc(kept_rows=None), 1, None) == -1
    assert lib.lbbnn_sparse_count(_desc(kept_rows=4098), 1, None) == -3
    for name in ("weight_mu", "weight_rho", "bias_rho", "row_ptr", "bias_var", "col", "mean", "var"):
        assert lib.lbbnn_sparse_pack(_desc(**{name: None}), 1, None) == -1, name
        assert lib.lbbnn_sparse_pack(_desc(**{name: 4098}), 1, None) == -3, name
    assert lib.lbbnn_sparse_pack(_desc(nnz=-1), 1, None) == -2


def test_sparse_desc_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%zu\\n", '
                   'sizeof(lbbnn_sparse_desc_t), offsetof(lbbnn_sparse_desc_t, kept_rows), offsetof(lbbnn_sparse_desc_t, cut)); '
                   'return 0; }\n' % os.path.join(ROOT, "include", "lbbnn.h"))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, kept, cut = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(_lib.SparseDesc) == size
    assert _lib.SparseDesc.kept_rows.offset == kept and _lib.SparseDesc.cut.offset == cut


def test_frozen_members_z_argument_checks(lib):
    from bnn_amd import _lib
    z = lib.lbbnn_frozen_members_z

    def desc(**kw):
        d = (_lib.FrozenDesc * 5)()
        base = dict(q0_mean=4096, q0_log_var=4096, z_fwd=4096, z_mstride=32, O=4, I=8)
        for k, v in dict(base, **kw).items():
            setattr(d[0], k, v)
        return d
    assert z(None, 1, 2, _F, 1, None) == -1
    assert z(desc(), 0, 2, _F, 1, None) == -2
    assert z(desc(), 5, 2, _F, 1, None) == -2
    assert z(desc(), 1, 0, _F, 1, None) == -2
    assert z(desc(), 1, 65536, _F, 1, None) == -2
    assert z(desc(q0_mean=None), 1, 2, None, 1, None) == 0            # no MNF layer: a successful no-op, rng not needed
    assert z(desc(q0_log_var=None), 1, 2, _F, 1, None) == -1
    assert z(desc(z_fwd=None), 1, 2, _F, 1, None) == -1
    d = desc()
    d[0].z_flow.T = 1                                                 # a transform without its vectors
    assert z(d, 1, 2, _F, 1, None) == -1
    assert z(desc(), 1, 2, None, 1, None) == -5
    assert z(desc(O=0), 1, 2, _F, 1, None) == -2
    assert z(desc(I=0), 1, 2, _F, 1, None) == -2
    assert z(desc(I=20000), 1, 2, _F, 1, None) == -2                  # LBBNN_MAX_FLOW_DIM
    assert z(desc(z_mstride=4), 1, 2, _F, 1, None) == -2
    d = desc()
    d[0].z_flow.T = 17
    assert z(d, 1, 2, _F, 1, None) == -2
    assert z(desc(I=6), 1, 2, _F, 1, None) == -3
    assert z(desc(z_mstride=30), 1, 2, _F, 1, None) == -3
    assert z(desc(z_fwd=4100), 1, 2, _F, 1, None) == -3
    # what the scale launch of lbbnn_frozen_members needs is not asked for: no e0, no e_w_members, no ld, any flags
    assert lib.lbbnn_frozen_members(desc(), 1, 2, _F, 1, None) == -1
    assert z(desc(flags=0x100, ld=7, I=20000), 1, 2, _F, 1, None) == -2


_LAYER = dict(row_ptr=_F, col=_F, mean=_F, var=_F, nnz=5, bias_mu=_F, bias_var=_F, a=_F, lda=64, a_mstride=0, z=None,
              z_mstride=0, rng=_F, rng_stream=0, row_offset=0, member_advance=1, out=_F, ldo=64, o_mstride=4 * 64, out_rows=0,
              B=3, I=8, O=4, flags=0, members=2)
# in the order of the checks; every row but the first of a code is also invalid at a LATER check
_LAYER_ROWS = [
    (dict(B=0, row_ptr=None), 0),                                      # an empty batch: nothing to do
    (dict(row_ptr=None, B=-1), -1), (dict(bias_mu=None), -1), (dict(bias_var=None), -1), (dict(a=None), -1), (dict(out=None), -1),
    (dict(col=None, I=0), -1), (dict(mean=None), -1), (dict(var=None), -1),
    (dict(B=-1, flags=0x100), -2), (dict(B=65535 * 64 + 1, lda=1 << 23, ldo=1 << 23), -2), (dict(I=0), -2), (dict(O=0), -2),
    (dict(nnz=-1, col=None), -2), (dict(members=0), -2), (dict(members=65536), -2),
    (dict(lda=2), -2), (dict(ldo=2), -2), (dict(out_rows=1, ldo=3, flags=_LSM), -2),
    (dict(a_mstride=-1), -2), (dict(z_mstride=-1), -2), (dict(o_mstride=-1), -2),
    (dict(o_mstride=3 * 64 + 2), -2), (dict(out_rows=1, ldo=4, o_mstride=11), -2),
    (dict(a_mstride=7 * 64 + 2), -2), (dict(z=_F, z_mstride=7), -2),
    (dict(flags=0x100, rng=None), -4), (dict(flags=0x4), -4),
    (dict(flags=_LSM, rng=None), -4),                                  # log_softmax into a transposed output
    (dict(flags=_LSM | _RELU, out_rows=1, ldo=4, o_mstride=12), -4),
    (dict(flags=_LSM, out_rows=1, O=17, ldo=17, o_mstride=64), -4),
    (dict(rng=None, a=_ODD), -5),
    (dict(row_ptr=_ODD), -3), (dict(col=_ODD), -3), (dict(mean=_ODD), -3), (dict(var=_ODD), -3), (dict(bias_mu=_ODD), -3),
    (dict(bias_var=_ODD), -3), (dict(a=_ODD), -3), (dict(z=_ODD, z_mstride=8), -3), (dict(out=_ODD), -3),
    (dict(rng=ctypes.c_void_p(4100)), -3),
]


@pytest.mark.parametrize("change,code", _LAYER_ROWS, ids=[str(i) for i in range(len(_LAYER_ROWS))])
def test_sparse_layer_members_argument_checks(lib, change, code):
    assert not set(change) - set(_LAYER), change
    assert lib.lbbnn_sparse_layer_members(*dict(_LAYER, **change).values(), None) == code, change


def test_sparse_layer_members_takes_an_empty_csr_without_its_arrays(lib):
    """nnz == 0 (every row empty) needs no col / mean / var; the remaining checks still hold (here: no rng)."""
    args = dict(_LAYER, nnz=0, col=None, mean=None, var=None, rng=None)
    assert lib.lbbnn_sparse_layer_members(*args.values(), None) == -5


# --------------------------------------------------------------------------- refusals that need no device
def _nets(bnn):
    return (bnn.lrt.BayesianNetwork((20, 16, 12, 3)),
            bnn.mnf.BayesianNetwork((20, 16, 12, 3), 2, z_flow_type="Planar", r_flow_type="Planar"))


def test_freeze_sparse_refusals(bnn):
    ev = bnn.evaluate
    for net in _nets(bnn):
        with pytest.raises(ValueError, match=r'sparse=True needs gates="mpm".*freeze\(net, "mpm", sparse=True\)'):
            ev.freeze(net, "alpha", sparse=True)
        with pytest.raises(ValueError, match=r'sparse=True needs gates="mpm"'):
            ev.freeze(net, sparse=True)
        with pytest.raises(ValueError, match=r"sparse=True does not take compact=True.*freeze\(net, \"mpm\", sparse=True\)"):
            ev.freeze(net, "mpm", sparse=True, compact=True)
        with pytest.raises(ValueError, match=r"sparse=True does not take dense=True.*freeze\(net, \"mpm\", dense=True\)"):
            ev.freeze(net, "mpm", sparse=True, dense=True)
        with pytest.raises(ValueError, match="threshold"):
            ev.freeze(net, "mpm", sparse=True, threshold=1.0)
        with pytest.raises(RuntimeError, match="HIP device"):        # a CPU network: no CPU path, said before any launch
            ev.freeze(net, "mpm", sparse=True)
    dense = bnn.mnf.BayesianNetwork((20, 16, 12, 3), 2)              # the reference's default: dense coupling z flows
    if dense.l1._check_flows() == "dense":
        with pytest.raises(ValueError, match=r"sparse=True is not built for dense coupling z flows.*dense=True"):
            ev.freeze(dense, "mpm", sparse=True)


def test_freeze_sparse_refuses_other_families(bnn):
    ev = bnn.evaluate
    with pytest.raises(TypeError, match="baseline"):
        ev.freeze(bnn.base.BayesianNetwork((20, 16, 3)), "mpm", sparse=True)
    with pytest.raises(TypeError, match="variational-dropout"):
        ev.freeze(bnn.vd.BNN((20, 16, 3)), "mpm", sparse=True)
    with pytest.raises(TypeError):
        ev.freeze(torch.nn.Linear(3, 3), "mpm", sparse=True)


def test_sparse_model_class(bnn):
    ev = bnn.evaluate
    assert issubclass(ev.SparseFrozenNetwork, ev.FrozenNetwork)
    fz = ev.SparseFrozenNetwork((20, 16, 3), "lrt", 0.9)
    assert ev._is_frozen(fz) and fz.gates == "mpm" and fz.threshold == 0.9 and fz.nnz == 0 and list(fz.parameters()) == []
    with pytest.raises(NotImplementedError, match=r"freeze again \(evaluate.freeze\(net, \"mpm\", sparse=True\)\)"):
        fz.refresh()
    with pytest.raises(ValueError, match=r"explain is not built for sparse=True models.*freeze\(net, \"mpm\"\)"):
        ev.explain(fz, torch.zeros(2, 20))
