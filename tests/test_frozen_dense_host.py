"""CPU tier of the frozen evaluation model for RNVP / MNF-type z flows (include/lbbnn.h lbbnn_flow_dense_members /
lbbnn_frozen_members_dense, evaluate.freeze(dense=True)): the entry points are exported and bound, lbbnn_dense_members_t
matches the header, the argument checks return the documented codes without launching, the Python interface keeps its
planar refusal without ``dense=True`` and names the layer and the loop form in every new refusal, and the mask helper of
the GPU tier (philox_bits_ref.mask_bits) is deterministic, distinct per member offset and unbiased."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lbbnn_flow_dense_members", "lbbnn_flow_dense_members_max_dim", "lbbnn_frozen_members_dense")
E_NULL, E_SHAPE, E_ALIGN, E_FLAGS, E_NOISE = -1, -2, -3, -4, -5
FAKE = 4096                      # never dereferenced: every call below must fail before launching


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_new_symbols_exported_and_bound(lib):
    from bnn_amd import _lib
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.lbbnn_abi_version() == 1
    # LDS: 1280 B per 16 elements of z (image + mask bytes) + 49 KiB within 160 KiB; every width the reference uses fits
    lim = lib.lbbnn_flow_dense_members_max_dim()
    assert lim == 16 * ((160 * 1024 - 4 * (2 * 16 * 136 + 4 * 8 * 256)) // 1280) == 1408
    assert lim >= 1200 and lim % 16 == 0


def test_dense_members_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    cname, cls = "lbbnn_dense_members_t", _lib.DenseMembers
    fields = ("q0_mean", "q0_log_var", "zt", "T", "I", "layer_id", "z_fwd", "z_mstride", "mask_out")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"),
             "int main(void) {", 'printf("size %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f in fields]
    lines += ['printf("maxt %d\\n", LBBNN_MAX_DENSE_T);', 'printf("maxh %d\\n", LBBNN_MAX_HIDDEN);', "return 0; }"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict((l.split()[0], int(l.split()[1]))
               for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == got["size"]
    for f in fields:
        assert getattr(cls, f).offset == got[f], f
    assert (got["maxt"], got["maxh"]) == (_lib.MAX_DENSE_T, _lib.MAX_HIDDEN)


def _transforms(_lib, T=2, kind=0, hidden=75):
    arr = (_lib.DenseTransform * max(T, 1))()
    for t in range(T):
        d = arr[t]
        d.kind, d.hidden = kind, hidden
        for name in ("w_in", "b_in", "w_a", "b_a", "w_b", "b_b"):
            setattr(d, name, FAKE)
        if kind == 0:
            for l in range(3):
                d.w_mid[l], d.b_mid[l] = FAKE, FAKE
    return arr


def _flows(_lib, I=8, T=2, kind=0, hidden=75, n=1, stride=None):
    keep = []
    f = (_lib.DenseMembers * n)()
    for k in range(n):
        zt = _transforms(_lib, T, kind, hidden)
        keep.append(zt)
        f[k].q0_mean, f[k].q0_log_var, f[k].z_fwd = FAKE, FAKE, FAKE
        f[k].zt = ctypes.cast(zt, ctypes.POINTER(_lib.DenseTransform))
        f[k].T, f[k].I, f[k].layer_id = T, I, k
        f[k].z_mstride = I if stride is None else stride
    return f, keep


def test_flow_dense_members_argument_checks(lib):
    from bnn_amd import _lib
    fn = lib.lbbnn_flow_dense_members
    lim = lib.lbbnn_flow_dense_members_max_dim()
    rng = FAKE
    assert fn(None, 1, 1, rng, 1, None) == E_NULL
    f, k = _flows(_lib)
    assert fn(f, 0, 1, rng, 1, None) == E_SHAPE
    assert fn(f, _lib.MAX_LAYERS + 1, 1, rng, 1, None) == E_SHAPE
    assert fn(f, 1, 0, rng, 1, None) == E_SHAPE
    assert fn(f, 1, 65536, rng, 1, None) == E_SHAPE
    assert fn(f, 1, 10, None, 1, None) == E_NOISE
    for name in ("q0_mean", "q0_log_var", "z_fwd", "zt"):
        f, k = _flows(_lib)
        setattr(f[0], name, None)
        assert fn(f, 1, 10, rng, 1, None) == E_NULL, name
    for name in ("w_in", "b_in", "w_a", "b_a", "w_b", "b_b"):
        f, k = _flows(_lib)
        setattr(k[0][1], name, None)
        assert fn(f, 1, 10, rng, 1, None) == E_NULL, name
    f, k = _flows(_lib)
    k[0][0].w_mid[2] = None                                    # RNVP needs its middle layers ...
    assert fn(f, 1, 10, rng, 1, None) == E_NULL
    f, k = _flows(_lib, kind=1)                                # ... the MNF type has none
    assert fn(f, 1, 10, None, 1, None) == E_NOISE
    for kw in (dict(T=-1), dict(T=_lib.MAX_DENSE_T + 1), dict(I=0), dict(I=lim + 4), dict(hidden=0),
               dict(hidden=_lib.MAX_HIDDEN + 1), dict(I=8, stride=4), dict(kind=2)):
        f, k = _flows(_lib, **kw)
        assert fn(f, 1, 10, rng, 1, None) == E_SHAPE, kw
    f, k = _flows(_lib)
    k[0][1].kind = 1                                           # kinds mixed within a layer
    k[0][1].hidden = 100
    assert fn(f, 1, 10, rng, 1, None) == E_SHAPE
    f, k = _flows(_lib, I=10, stride=12)
    assert fn(f, 1, 10, rng, 1, None) == E_ALIGN
    f, k = _flows(_lib, I=8, stride=10)
    assert fn(f, 1, 10, rng, 1, None) == E_ALIGN
    f, k = _flows(_lib)
    f[0].z_fwd = FAKE + 4
    assert fn(f, 1, 10, rng, 1, None) == E_ALIGN
    f, k = _flows(_lib, n=2)                                   # the second layer is checked too
    f[1].I = lim + 16
    f[1].z_mstride = lim + 16
    assert fn(f, 2, 10, rng, 1, None) == E_SHAPE


def _desc(_lib, O=4, I=8, ld=32, n=1):
    d = (_lib.FrozenDesc * n)()
    for k in range(n):
        for j, name in enumerate(("weight_mu", "weight_rho", "lambdal", "bias_rho", "e0", "e_w", "var_w", "bias_var",
                                  "kept_rows")):
            setattr(d[k], name, 4096 * (j + 1))
        d[k].O, d[k].I, d[k].ld, d[k].flags, d[k].mode, d[k].cut, d[k].layer_id = O, I, ld, 0, 0, 0.0, k
        d[k].q0_mean, d[k].q0_log_var, d[k].z_fwd, d[k].e_w_members = 4096 * 20, 4096 * 21, 4096 * 22, 4096 * 23
        d[k].z_mstride = ld
        d[k].z_flow.T = 99                                     # ignored by the dense form
    return d


def test_frozen_members_dense_argument_checks(lib):
    from bnn_amd import _lib
    fn = lib.lbbnn_frozen_members_dense
    rng = FAKE
    f, k = _flows(_lib)
    assert fn(None, f, 1, 1, rng, 1, None) == E_NULL
    assert fn(_desc(_lib), None, 1, 1, rng, 1, None) == E_NULL
    assert fn(_desc(_lib), f, 0, 1, rng, 1, None) == E_SHAPE
    assert fn(_desc(_lib), f, _lib.MAX_LAYERS + 1, 1, rng, 1, None) == E_SHAPE
    assert fn(_desc(_lib), f, 1, 0, rng, 1, None) == E_SHAPE
    assert fn(_desc(_lib), f, 1, 65536, rng, 1, None) == E_SHAPE
    assert fn(_desc(_lib), f, 1, 10, None, 1, None) == E_NOISE
    for name in ("q0_log_var", "z_fwd", "e0", "e_w_members"):
        d = _desc(_lib)
        setattr(d[0], name, None)
        assert fn(d, f, 1, 10, rng, 1, None) == E_NULL, name
    for kw in (dict(O=0), dict(I=0), dict(I=40, ld=32)):
        assert fn(_desc(_lib, **kw), f, 1, 10, rng, 1, None) == E_SHAPE, kw
    d = _desc(_lib)
    d[0].z_mstride = 4
    assert fn(d, f, 1, 10, rng, 1, None) == E_SHAPE
    assert fn(_desc(_lib, ld=48), f, 1, 10, rng, 1, None) == E_ALIGN
    assert fn(_desc(_lib, I=6), f, 1, 10, rng, 1, None) == E_ALIGN
    d = _desc(_lib)
    d[0].z_fwd = 4096 * 22 + 8
    assert fn(d, f, 1, 10, rng, 1, None) == E_ALIGN
    d = _desc(_lib)
    d[0].flags = 0x100
    assert fn(d, f, 1, 10, rng, 1, None) == E_FLAGS
    # the flow's own checks come through: too many transforms, a transform without its matrices
    f2, k2 = _flows(_lib, T=_lib.MAX_DENSE_T + 1)
    assert fn(_desc(_lib), f2, 1, 10, rng, 1, None) == E_SHAPE
    f2, k2 = _flows(_lib)
    k2[0][0].w_b = None
    assert fn(_desc(_lib), f2, 1, 10, rng, 1, None) == E_NULL
    # an LRT layer (q0_mean NULL) is skipped and its flow entry not read: nothing to do is a successful no-op
    d = _desc(_lib)
    d[0].q0_mean = None
    assert fn(d, (_lib.DenseMembers * 1)(), 1, 10, None, 1, None) == 0


# ------------------------------------------------------------------------------------------------- Python interface
def _net(kind="RNVP", dims=(20, 16, 12, 3), T=1):
    import bnn_amd
    torch.manual_seed(0)
    return bnn_amd.mnf.BayesianNetwork(dims, T, z_flow_type=kind, r_flow_type=kind)


def test_freeze_without_dense_keeps_the_planar_refusal(lib):
    from bnn_amd import evaluate as ev
    with pytest.raises(ValueError, match="planar flows"):
        ev.freeze(_net("RNVP"))
    with pytest.raises(ValueError, match="planar flows"):
        ev.freeze(_net("MNF"), "mpm", dense=False)


@pytest.mark.parametrize("kind", ["RNVP", "MNF"])
def test_freeze_dense_accepts_and_reaches_the_device_check(lib, kind):
    from bnn_amd import evaluate as ev
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.freeze(_net(kind), dense=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.freeze(_net(kind, (784, 1200, 1200, 10), 2), "mpm", dense=True)


def test_freeze_dense_refusals_name_the_layer_and_the_loop(lib):
    from bnn_amd import evaluate as ev, _lib
    lim = lib.lbbnn_flow_dense_members_max_dim()
    loop = r"ensemble_forward\(net, data, samples\)"
    with pytest.raises(ValueError, match=r"layer 2.*in_features % 4.*" + loop):
        ev.freeze(_net("RNVP", (20, 18, 12, 3)), dense=True)
    with pytest.raises(ValueError, match=r"layer 2.*in_features = %d.*\(%d\).*" % (lim + 4, lim) + loop):
        ev.freeze(_net("MNF", (16, lim + 4, 8, 3)), dense=True)
    with pytest.raises(ValueError, match=r"layer 1.*%d transforms.*at most %d.*" % (_lib.MAX_DENSE_T + 1, _lib.MAX_DENSE_T)
                       + loop):
        ev.freeze(_net("MNF", (8, 8, 4, 2), _lib.MAX_DENSE_T + 1), dense=True)
    net = _net("RNVP")
    net.l2.noise = {"eps_z": torch.zeros(1, 16)}
    with pytest.raises(ValueError, match=r"layer 2 has injected noise.*batched=False"):
        ev.freeze(net, dense=True)
    net = _net("RNVP")
    net.l3.as_written = True
    with pytest.raises(ValueError, match=r"layer 3 has as_written.*batched=False"):
        ev.freeze(net, dense=True)
    with pytest.raises(ValueError):                              # 1-D chain flows stay outside either form
        ev.freeze(_net("Radial"), dense=True)
    with pytest.raises(ValueError, match="flows must be"):
        ev.FrozenNetwork((4, 4, 4, 2), "lrt", flows="dense")
    assert ev.FrozenNetwork((4, 4, 4, 2), "mnf").flows == "planar" and ev.FrozenNetwork((4, 4, 4, 2), "lrt").flows is None
    assert ev.FrozenNetwork((4, 4, 4, 2), "mnf", flows="dense").flows == "dense"


# ------------------------------------------------------------------------------------------------- the mask helper
def test_mask_bits_deterministic_distinct_and_unbiased():
    from philox_bits_ref import mask_bits
    I, T = 1200, 8
    rows = [mask_bits(3, o, 1, I, T) for o in range(5, 16)]
    for o, r in zip(range(5, 16), rows):
        assert r.shape == (T, I) and r.dtype == np.float32 and bool(((r == 0) | (r == 1)).all())
        assert np.array_equal(r, mask_bits(3, o, 1, I, T))
        assert np.array_equal(r[:3], mask_bits(3, o, 1, I, 3))                # bit t does not depend on T
        assert np.array_equal(r[:, :100], mask_bits(3, o, 1, 100, T))         # ... nor element i on I
    bits = np.stack(rows)
    n = bits.size
    assert n == 105600
    dev = abs(float(bits.mean()) - 0.5) * np.sqrt(n)
    print("mask_bits: n = %d mean %.5f |mean - 0.5| sqrt(n) = %.2f" % (n, bits.mean(), dev))
    assert dev < 4.0                                                          # 8 standard deviations
    for a, b in zip(rows[:-1], rows[1:]):                                     # member offsets give distinct masks
        assert 0.45 < float((a != b).mean()) < 0.55
    assert 0.45 < float((mask_bits(3, 5, 1, I, T) != mask_bits(3, 5, 2, I, T)).mean()) < 0.55   # and so do layers
    assert 0.45 < float((mask_bits(3, 5, 1, I, T) != mask_bits(4, 5, 1, I, T)).mean()) < 0.55   # and seeds
    for t in range(T - 1):                                                    # and transforms
        assert 0.4 < float((rows[0][t] != rows[0][t + 1]).mean()) < 0.6
