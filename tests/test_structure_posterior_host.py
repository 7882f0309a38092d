"""CPU tier of the posterior over network structures (include/lbbnn.h lbbnn_gate_structure / lbbnn_gate_structure_width,
evaluate.structure_posterior): the entry point's early return codes (nothing is launched), the size helper, the ctypes
struct, the Python refusals, and the numpy reference of the GPU tier against evaluate.live_structure."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import philox_ref as pr
import structure_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_F = ctypes.c_void_p(4096)             # never dereferenced
_ODD = ctypes.c_void_p(4098)           # off 4 bytes


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def _descs(shapes, ld=None, lambdal=4096):
    from bnn_amd import _lib
    d = (_lib.StructureDesc * max(len(shapes), 1))()
    for k, (O, I) in enumerate(shapes):
        d[k].lambdal, d[k].O, d[k].I, d[k].ld, d[k].layer_id = lambdal, O, I, (I if ld is None else ld), k
    return d


def _call(lib, d, n, samples=3, rng=_F, kept=_F, needed=_F, active=_F, feature_count=_F, unit_count=None, need_out=None):
    return lib.lbbnn_gate_structure(d, n, samples, rng, kept, needed, active, feature_count, unit_count, need_out, None)


def test_the_symbols_are_declared_and_bound(lib):
    from bnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "lbbnn.h")).read()
    for name in ("lbbnn_gate_structure", "lbbnn_gate_structure_width"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "gate_structure.hip" in open(os.path.join(ROOT, "bayesian-neural-nets_amd", "csrc", "Makefile")).read()


def test_early_return_codes_nothing_launched(lib):
    one = _descs([(3, 5)])
    # NULL pointers
    assert _call(lib, None, 1) == -1
    for name in ("kept", "needed", "active", "feature_count"):
        assert _call(lib, one, 1, **{name: None}) == -1, name
    assert _call(lib, _descs([(3, 5)], lambdal=None), 1) == -1
    assert _call(lib, one, 1, rng=None) == -5                           # the draws need the Philox state
    # n of 0 and 17, samples of 0 and 65536
    sixteen = _descs([(4, 4)] * 17)
    assert _call(lib, sixteen, 0) == -2 and _call(lib, sixteen, 17) == -2 and _call(lib, sixteen, -1) == -2
    assert _call(lib, one, 1, samples=0) == -2 and _call(lib, one, 1, samples=65536) == -2
    # a width of 0 and of 4097, either side
    for shape in ((0, 5), (3, 0), (4097, 5), (3, 4097)):
        assert _call(lib, _descs([shape]), 1) == -2, shape
    # row stride below I
    assert _call(lib, _descs([(3, 5)], ld=4), 1) == -2
    # the layers chain: I of a layer is the O of the one below
    assert _call(lib, _descs([(3, 5), (2, 4)]), 2) == -2
    # alignment: lambdal and the int32 outputs on 4 bytes
    assert _call(lib, _descs([(3, 5)], lambdal=4098), 1) == -3
    for name in ("kept", "needed", "active", "feature_count", "unit_count"):
        assert _call(lib, one, 1, **{name: _ODD}) == -3, name
    # precedence: the earlier check's code wins
    assert _call(lib, None, 0) == -1 and _call(lib, one, 0, rng=None) == -2
    assert _call(lib, _descs([(3, 5)], ld=4, lambdal=4098), 1) == -2 and _call(lib, _descs([(3, 5)], lambdal=4098), 1, rng=None) == -3


def test_width_helper(lib):
    w = lib.lbbnn_gate_structure_width
    assert w(_descs([(3, 5)]), 1) == 8
    assert w(_descs([(1200, 784), (1200, 1200), (10, 1200)]), 3) == 784 + 1200 + 1200 + 10
    assert w(_descs([(4096, 4096)]), 1) == 8192
    assert w(_descs([(4, 4)] * 16), 16) == 17 * 4
    # layers the call would refuse: 0
    assert w(None, 1) == 0 and w(_descs([(3, 5)]), 0) == 0 and w(_descs([(4, 4)] * 17), 17) == 0
    assert w(_descs([(3, 5), (2, 4)]), 2) == 0 and w(_descs([(4097, 5)]), 1) == 0 and w(_descs([(3, 5)], ld=4), 1) == 0
    assert w(_descs([(3, 5)], lambdal=None), 1) == 0


def test_ctypes_struct_matches_the_header(tmp_path):
    from bnn_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                   'printf("%%zu %%zu %%zu %%d %%d\\n", sizeof(lbbnn_structure_desc_t), offsetof(lbbnn_structure_desc_t, O), '
                   'offsetof(lbbnn_structure_desc_t, layer_id), LBBNN_STRUCTURE_MAX_LAYERS, LBBNN_STRUCTURE_MAX_WIDTH);\n'
                   'return 0; }\n' % os.path.join(ROOT, "include", "lbbnn.h"))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, off_o, off_id, max_layers, max_width = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(_lib.StructureDesc) == size
    assert _lib.StructureDesc.O.offset == off_o and _lib.StructureDesc.layer_id.offset == off_id
    assert (_lib.STRUCTURE_MAX_LAYERS, _lib.STRUCTURE_MAX_WIDTH) == (max_layers, max_width) == (_lib.MAX_DEPTH, 4096)


def test_python_refusals():
    import bnn_amd
    ev = bnn_amd.evaluate
    with pytest.raises(ValueError, match="variational-dropout"):
        ev.structure_posterior(bnn_amd.vd.BNN((8, 4, 2)), 4)
    with pytest.raises(ValueError, match="frozen"):
        ev.structure_posterior(ev.FrozenNetwork((20, 3), "lrt"), 4)
    with pytest.raises(ValueError, match="LRT, MNF or baseline"):
        ev.structure_posterior(torch.nn.Linear(4, 2), 4)
    for net in (bnn_amd.lrt.BayesianNetwork((8, 4, 2)), bnn_amd.base.BayesianNetwork((8, 4, 2)),
                bnn_amd.mnf.BayesianNetwork((8, 4, 2), 2, z_flow_type="Planar", r_flow_type="Planar")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ev.structure_posterior(net, 4)                               # a CPU network
        with pytest.raises(ValueError, match="samples"):
            ev.structure_posterior(net, 0)
        with pytest.raises(ValueError, match="max_members"):
            ev.structure_posterior(net, 4, max_members=0)
    # a width above 4096 names the layer (reached before the device check)
    with pytest.raises(ValueError, match="layer 1 is 3 x 4097"):
        ev.structure_posterior(bnn_amd.lrt.BayesianNetwork((4097, 3)), 4)
    with pytest.raises(ValueError, match="layer 2 is 4097 x 3"):
        ev.structure_posterior(bnn_amd.base.BayesianNetwork((4, 3, 4097)), 4)


@pytest.mark.parametrize("dims", [(5, 3, 2), (7, 1), (9, 6, 6, 4, 3), (65, 17, 4, 3)])
def test_structure_ref_agrees_with_live_structure(dims):
    from bnn_amd import evaluate
    rs = np.random.RandomState(len(dims))
    S, n = 5, len(dims) - 1
    gates = [rs.rand(S, dims[l + 1], dims[l]) < (0.15 if dims[l] > 8 else 0.45) for l in range(n)]
    ref = sr.structure_ref(gates)
    assert ref["kept"].shape == (S, n) and ref["needed"].shape == (S, n + 1) and len(ref["unit_count"]) == n - 1
    fc = np.zeros(dims[0], np.int64)
    for s in range(S):
        masks = [torch.from_numpy(g[s]) for g in gates]
        need, _ = evaluate.live_structure(masks)
        for b in range(n + 1):
            assert np.array_equal(ref["need"][b][s], need[b].numpy()), (s, b)
            assert ref["needed"][s, b] == int(need[b].sum())
        for l in range(n):
            assert ref["kept"][s, l] == int(masks[l].sum())
            assert ref["active_kept"][s, l] == int((masks[l] & need[l + 1][:, None]).sum())
            # a kept weight of a needed row has a needed column, so this is also the sum over needed rows AND columns
            assert ref["active_kept"][s, l] == int((masks[l] & need[l + 1][:, None] & need[l][None, :]).sum())
        fc += need[0].numpy()
    assert np.array_equal(ref["feature_count"], fc)
    assert (ref["needed"][:, n] == dims[-1]).all() and (ref["active_kept"] <= ref["kept"]).all()
    one = sr.structure_ref([g[0] for g in gates])                        # (O, I) arrays: one sample
    assert np.array_equal(one["kept"], ref["kept"][:1]) and np.array_equal(one["need"][0], ref["need"][0][:1])


def test_gate_uniforms_are_the_documented_words():
    """Element (o, i) is word i % 4 of counter (o, i // 4) of the gate stream, mapped into (0, 1); the state enters by the key."""
    u = sr.gate_uniforms(7, 100, 33, 3, 6)
    assert u.dtype == np.float32 and u.shape == (3, 6) and (u > 0).all() and (u < 1).all()
    k0, k1 = pr.key_of(7, 100)
    w = pr.philox4x32_10(np.uint64(2), np.uint64(0), np.uint64(1), np.uint64(8 * 64 + 33), k0, k1)
    assert u[2, 5] == np.float32(((int(w[1]) >> 8) + 0.5) * 2.0 ** -24)
    assert not np.array_equal(u, sr.gate_uniforms(7, 101, 33, 3, 6))
    gates, dist = sr.gates_ref([np.full((3, 6), 0.5, np.float32)], [33], 7, 100, 2)
    assert gates[0].shape == (2, 3, 6) and np.array_equal(gates[0][0], u < 0.5)
    assert np.array_equal(gates[0][1], sr.gate_uniforms(7, 101, 33, 3, 6) < 0.5) and dist[0].min() > 0
