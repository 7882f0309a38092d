"""CPU tier of the baseline family's sparse median-probability model (include/lbbnn.h: lbbnn_base_sparse_count / _pack /
lbbnn_base_sparse_draw_members; evaluate.freeze_base(net, "mpm", sparse=True)): the argument checks of the new entry points on
fake pointers (nothing is launched), the ctypes mirrors against the header compiled by gcc, the refusals that need no device,
and the inputs of the GPU tier (tests/base_sparse_ref.py) checked from torch alone."""
import ctypes
import os
import subprocess

import pytest
import torch

import base_sparse_ref as br
import frozen_sparse_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN, E_FLAGS, E_NOISE = -1, -2, -3, -4, -5
F = 4096                                   # a fake pointer: never dereferenced
ODD = 4098


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


def test_ctypes_structs_match_the_header(tmp_path):
    from bnn_amd import _lib
    pairs = [("lbbnn_base_sparse_desc_t", _lib.BaseSparseDesc, "nnz"),
             ("lbbnn_base_sparse_draw_desc_t", _lib.BaseSparseDrawDesc, "layer_id")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"), "int main(void) {"]
    for cname, _, last in pairs:
        lines.append('printf("%s %%zu %%zu\\n", sizeof(%s), offsetof(%s, %s));' % (cname, cname, cname, last))
    lines += ["return 0; }"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict((l.split()[0], (int(l.split()[1]), int(l.split()[2])))
               for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls, last in pairs:
        assert ctypes.sizeof(cls) == out[cname][0], (cname, ctypes.sizeof(cls), out[cname][0])
        assert getattr(cls, last).offset == out[cname][1], (cname, last)
    # every field of the mirrors, by name and in order, is a member of the header's struct
    hdr = open(os.path.join(ROOT, "include", "lbbnn.h")).read()
    for cname, cls, _ in pairs:
        body = hdr[hdr.index("typedef struct " + cname[:-2]):hdr.index("} " + cname)]
        at = 0
        for name, _t in cls._fields_:
            at = body.index(name, at)


def _pack_desc(_lib, **kw):
    d = (_lib.BaseSparseDesc * 5)()
    base = dict(mu=F, rho=F, lambdal=F, bias_mu=F, bias_rho=F, row_ptr=F, col=F, mean=F, sigma=F, b_mu=F, b_sigma=F,
                kept_rows=F, O=4, I=8, nnz=6)
    for k, v in dict(base, **kw).items():
        setattr(d[0], k, v)
    return d


def test_count_and_pack_argument_checks(lib):
    from bnn_amd import _lib
    thr = ctypes.c_float(0.5)
    for fn in (lib.lbbnn_base_sparse_count, lib.lbbnn_base_sparse_pack):
        assert fn(None, 1, thr, None) == E_NULL
        assert fn(_pack_desc(_lib), 0, thr, None) == E_SHAPE
        assert fn(_pack_desc(_lib), 5, thr, None) == E_SHAPE                 # more than LBBNN_MAX_LAYERS
        for bad in (0.0, 1.0, -0.5, float("nan")):
            assert fn(_pack_desc(_lib), 1, ctypes.c_float(bad), None) == E_FLAGS
        assert fn(_pack_desc(_lib, lambdal=None), 1, thr, None) == E_NULL
        assert fn(_pack_desc(_lib, O=0), 1, thr, None) == E_SHAPE
        assert fn(_pack_desc(_lib, I=0), 1, thr, None) == E_SHAPE
        assert fn(_pack_desc(_lib, lambdal=ODD), 1, thr, None) == E_ALIGN
    assert lib.lbbnn_base_sparse_count(_pack_desc(_lib, kept_rows=None), 1, thr, None) == E_NULL
    assert lib.lbbnn_base_sparse_count(_pack_desc(_lib, kept_rows=ODD), 1, thr, None) == E_ALIGN
    for k in ("mu", "rho", "bias_mu", "bias_rho", "row_ptr", "b_mu", "b_sigma", "col", "mean", "sigma"):
        assert lib.lbbnn_base_sparse_pack(_pack_desc(_lib, **{k: None}), 1, thr, None) == E_NULL, k
        assert lib.lbbnn_base_sparse_pack(_pack_desc(_lib, **{k: ODD}), 1, thr, None) == E_ALIGN, k
    assert lib.lbbnn_base_sparse_pack(_pack_desc(_lib, nnz=-1), 1, thr, None) == E_SHAPE
    # (a layer that keeps nothing has no col / mean / sigma: legal, and it would launch -- so it is not called here)
    # an invalid second layer is found too
    d = _pack_desc(_lib)
    for k, _t in _lib.BaseSparseDesc._fields_:
        setattr(d[1], k, getattr(d[0], k))
    d[1].O = -3
    assert lib.lbbnn_base_sparse_pack(d, 2, thr, None) == E_SHAPE


def _draw_desc(_lib, **kw):
    d = (_lib.BaseSparseDrawDesc * 5)()
    base = dict(row_ptr=F, col=F, mean=F, sigma=F, b_mu=F, b_sigma=F, tpos=None, wt=None, w=F, w_mstride=8, b=F, b_mstride=4,
                O=4, I=8, nnz=6, layer_id=1)
    for k, v in dict(base, **kw).items():
        setattr(d[0], k, v)
    return d


def test_draw_argument_checks(lib):
    from bnn_amd import _lib
    fn = lib.lbbnn_base_sparse_draw_members
    assert fn(None, 1, 2, F, 1, 0, None) == E_NULL
    assert fn(_draw_desc(_lib), 0, 2, F, 1, 0, None) == E_SHAPE
    assert fn(_draw_desc(_lib), 5, 2, F, 1, 0, None) == E_SHAPE
    assert fn(_draw_desc(_lib), 1, 0, F, 1, 0, None) == E_SHAPE
    assert fn(_draw_desc(_lib), 1, 65536, F, 1, 0, None) == E_SHAPE
    assert fn(_draw_desc(_lib), 1, 2, F, 1, 0x1, None) == E_FLAGS             # only LBBNN_F_MEAN_ONLY is a flag here
    assert fn(_draw_desc(_lib), 1, 2, None, 1, 0, None) == E_NOISE
    assert fn(_draw_desc(_lib), 1, 2, 4100, 1, 0, None) == E_ALIGN            # rng off 8 B
    for k in ("row_ptr", "b_mu", "b_sigma", "b", "col", "mean", "sigma", "w"):
        assert fn(_draw_desc(_lib, **{k: None}), 1, 2, F, 1, 0, None) == E_NULL, k
    assert fn(_draw_desc(_lib, tpos=F), 1, 2, F, 1, 0, None) == E_NULL        # tpos and wt come together
    assert fn(_draw_desc(_lib, wt=F), 1, 2, F, 1, 0, None) == E_NULL
    for kw in (dict(O=0), dict(I=0), dict(nnz=-1), dict(w_mstride=4), dict(b_mstride=0), dict(nnz=9)):
        assert fn(_draw_desc(_lib, **kw), 1, 2, F, 1, 0, None) == E_SHAPE, kw
    for kw in (dict(row_ptr=ODD), dict(col=ODD), dict(mean=ODD), dict(sigma=ODD), dict(b_mu=ODD), dict(b_sigma=ODD),
               dict(w=4100), dict(b=4100), dict(tpos=ODD, wt=F), dict(tpos=F, wt=4100), dict(w_mstride=10), dict(b_mstride=6)):
        assert fn(_draw_desc(_lib, **kw), 1, 2, F, 1, 0, None) == E_ALIGN, kw
    # the gather keeps its three modes
    g = _lib.SparseGatherArgs()
    g.B, g.mode = 4, 3
    assert lib.lbbnn_sparse_gather_members(ctypes.byref(g), None) == E_FLAGS


def test_refusals_without_a_device(bnn):
    ev = bnn.evaluate
    net = bnn.base.BayesianNetwork((20, 16, 1), head="sigmoid")
    with pytest.raises(ValueError, match=r"sparse=True needs gates=\"mpm\".*freeze_base\(net, \"mpm\", sparse=True\)"):
        ev.freeze_base(net, "sample", sparse=True)
    with pytest.raises(ValueError, match=r"sparse=True needs gates=\"mpm\""):
        ev.freeze_base(net, sparse=True)
    with pytest.raises(ValueError, match=r"sparse=True with compact=True.*already touches no pruned weight"):
        ev.freeze_base(net, "mpm", sparse=True, compact=True)
    with pytest.raises(ValueError, match="no CPU path"):
        ev.freeze_base(net, "mpm", sparse=True)
    with pytest.raises(ValueError, match="between 0 and 1"):
        ev.freeze_base(net, "mpm", threshold=1.0, sparse=True)
    net.l1.noise = {"eps_w": torch.zeros(16, 20)}
    with pytest.raises(ValueError, match="injected noise"):
        ev.freeze_base(net, "mpm", sparse=True)
    net.l1.noise = None
    x = torch.zeros(2, 20)
    for what in (net, ev.FrozenBaseNetwork((20, 16, 1), "mpm", head="sigmoid")):
        with pytest.raises(TypeError, match=r"evaluate\.freeze_base\(net, \"mpm\", sparse=True\)"):
            ev.explain_ensemble(what, x)
    # the model class: the median probability model only, a _FrozenModel of family "base", no refresh
    fz = ev.SparseFrozenBaseNetwork((20, 16, 1), 0.9, head="sigmoid")
    assert isinstance(fz, ev._FrozenModel) and not isinstance(fz, ev.FrozenBaseNetwork)
    assert (fz.family, fz.gates, fz.threshold, fz.head) == ("base", "mpm", 0.9, "sigmoid")
    assert not [k for k, _ in fz.named_buffers() if not k.startswith("kept_rows_")]      # no dense plane it never fills
    with pytest.raises(NotImplementedError, match=r"freeze again.*sparse=True"):
        fz.refresh()
    with pytest.raises(ValueError, match="explain_ensemble\\(fz, data, samples=1, weight_noise=False\\)"):
        ev.explain(fz, x)
    assert bnn.SparseFrozenBaseNetwork is ev.SparseFrozenBaseNetwork


@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
def test_the_inputs_are_unambiguous(threshold):
    """tests/frozen_sparse_ref.py's builder holds its assertions at the GPU tier's shapes, and there the keep rule of the dense
    baseline model (sigmoid(lambdal) > threshold) and of the LRT pack (lambdal > logit(threshold)) give one pattern, with a
    margin of at least 1e-4 in alpha: a thousand times what an fp32 sigmoid can be off by."""
    worst = 1.0
    for dims, _ in br.CASES + [(br.BIG, "log_softmax")]:
        lams, masks = sr.lambdals(dims, threshold)
        for lam, keep in zip(lams, masks):
            alpha32 = torch.sigmoid(lam)
            assert torch.equal(alpha32 > torch.tensor(threshold, dtype=torch.float32), keep)
            assert torch.equal(torch.sigmoid(lam.double()) > threshold, keep)
            worst = min(worst, float((torch.sigmoid(lam.double()) - threshold).abs().min()))
    print("smallest |sigmoid(lambdal) - threshold| at %g: %.3g" % (threshold, worst))
    assert worst >= 1e-4
