"""CPU tier of the compact median-probability model (evaluate.live_structure / freeze(..., compact=True) /
CompactFrozenNetwork; include/lbbnn.h lbbnn_frozen_operands_compact, lbbnn_frozen_members_compact, lbbnn_gather_columns):
the structure rule against brute-force path reachability, the top-up rule, exactness of dropping the unneeded units in
float64, the C ABI (symbols, struct layout, every argument check without a launch) and the refusals of freeze."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import frozen_compact_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lbbnn_frozen_operands_compact", "lbbnn_frozen_members_compact", "lbbnn_gather_columns")
E_NULL, E_SHAPE, E_ALIGN, E_FLAGS, E_NOISE = -1, -2, -3, -4, -5
DIMS = sorted({d for _, d, _, _ in cc.CASES})


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


# --------------------------------------------------------------------------- the structure rule
@pytest.mark.parametrize("dims", DIMS, ids=["-".join(map(str, d)) for d in DIMS])
def test_live_structure_equals_path_reachability(dims):
    from bnn_amd import evaluate
    _, masks = cc.lambdals(dims)
    n = len(dims) - 1
    need, live = evaluate.live_structure(masks)
    ref = cc.brute_need(masks)
    assert len(need) == len(live) == n + 1
    for b in range(n + 1):
        assert need[b].dtype == torch.bool and torch.equal(need[b], ref[b]), b
    sizes = cc.expected_live_sizes(ref)
    for b, t in enumerate(live):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.numel() == sizes[b], (b, t.numel(), sizes[b])
        tl = t.long()
        assert bool((tl[1:] > tl[:-1]).all())                              # sorted and unique
        assert int(tl[0]) >= 0 and int(tl[-1]) < dims[b]
        inlive = torch.zeros(dims[b], dtype=torch.bool)
        inlive[tl] = True
        assert bool(inlive[ref[b]].all())                                  # every needed unit is live
        extra = int(inlive.sum()) - int(ref[b].sum())
        dead = torch.nonzero(~ref[b]).reshape(-1)
        assert torch.equal(torch.nonzero(inlive & ~ref[b]).reshape(-1), dead[:extra])   # topped up from the lowest index
    assert torch.equal(live[n].long(), torch.arange(dims[-1]))
    assert all(s % 8 == 0 or s == dims[b] for b, s in enumerate(sizes[:n]))
    if dims in cc.TABLE:
        assert tuple(int(nd.sum()) for nd in need) == cc.TABLE[dims][0]
        assert tuple(t.numel() for t in live) == cc.TABLE[dims][1]


def test_live_structure_edges():
    from bnn_amd import evaluate
    # a boundary nobody needs gives `align` units (the lowest indices), never an empty layer
    k0 = torch.ones(12, 20, dtype=torch.bool)
    k1 = torch.zeros(3, 12, dtype=torch.bool)
    need, live = evaluate.live_structure([k0, k1])
    assert not need[1].any() and not need[0].any() and need[2].all()
    assert live[1].tolist() == list(range(8)) and live[0].tolist() == list(range(8)) and live[2].tolist() == [0, 1, 2]
    need, live = evaluate.live_structure([k0, k1], align=4)
    assert live[1].tolist() == [0, 1, 2, 3]
    # narrower than align: the whole boundary
    need, live = evaluate.live_structure([torch.ones(3, 5, dtype=torch.bool)])
    assert live[0].tolist() == [0, 1, 2, 3, 4]
    # nothing unneeded: the identity at every boundary
    need, live = evaluate.live_structure([torch.ones(16, 24, dtype=torch.bool), torch.ones(4, 16, dtype=torch.bool)])
    assert [t.tolist() for t in live] == [list(range(24)), list(range(16)), list(range(4))]
    # a needed unit with no kept input stays
    k0 = torch.ones(16, 24, dtype=torch.bool)
    k0[5] = False
    need, live = evaluate.live_structure([k0, torch.ones(4, 16, dtype=torch.bool)])
    assert bool(need[1][5]) and 5 in live[1].tolist()
    with pytest.raises(ValueError, match="columns"):
        evaluate.live_structure([torch.ones(16, 24, dtype=torch.bool), torch.ones(4, 15, dtype=torch.bool)])
    with pytest.raises(ValueError, match="bool"):
        evaluate.live_structure([torch.ones(16, 24)])


def _forward64(x, P, masks, eps):
    h = x
    n = len(P)
    for i, (p, keep) in enumerate(zip(P, masks)):
        k = keep.double()
        mean = h @ (p["mu"] * k).t() + p["bias_mu"]
        var = (h * h) @ (p["s2"] * k).t() + p["bias_var"]
        h = mean + var.sqrt() * eps[i]
        if i < n - 1:
            h = torch.relu(h)
    return h


@pytest.mark.parametrize("dims", DIMS, ids=["-".join(map(str, d)) for d in DIMS])
def test_compact_forward_equals_full_forward_in_float64(dims):
    """Dropping the unneeded units (and keeping the topped-up dead ones) changes nothing: the float64 compact forward
    equals the float64 full forward whose noise is the compact noise scattered to the live columns (zeros elsewhere)."""
    from bnn_amd import evaluate
    _, masks = cc.lambdals(dims)
    n, B = len(dims) - 1, 5
    _, live = evaluate.live_structure(masks)
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    P = [dict(mu=rnd(dims[i + 1], dims[i]), s2=rnd(dims[i + 1], dims[i]) ** 2 * 0.1, bias_mu=rnd(dims[i + 1]),
              bias_var=rnd(dims[i + 1]) ** 2 * 0.1) for i in range(n)]
    x = torch.rand(B, dims[0], generator=g, dtype=torch.float64)
    L = [t.long() for t in live]
    eps_c = [rnd(B, L[i + 1].numel()) for i in range(n)]
    eps_f = []
    for i in range(n):
        e = torch.zeros(B, dims[i + 1], dtype=torch.float64)
        e[:, L[i + 1]] = eps_c[i]
        eps_f.append(e)
    full = _forward64(x, P, masks, eps_f)
    Pc = [dict(mu=p["mu"][L[i + 1]][:, L[i]], s2=p["s2"][L[i + 1]][:, L[i]], bias_mu=p["bias_mu"][L[i + 1]],
               bias_var=p["bias_var"][L[i + 1]]) for i, p in enumerate(P)]
    mc = [m[L[i + 1]][:, L[i]] for i, m in enumerate(masks)]
    comp = _forward64(x[:, L[0]], Pc, mc, eps_c)
    assert comp.shape == full.shape == (B, dims[-1])
    err = float((comp - full).abs().max() / full.abs().max())
    print("compact vs full float64 %s: %.3g" % (dims, err))
    assert err < 1e-12, err


# --------------------------------------------------------------------------- the C ABI
def test_new_symbols_declared_exported_and_bound(lib):
    from bnn_amd import _lib
    src = open(os.path.join(ROOT, "include", "lbbnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lbbnn_[a-z0-9_]+)\s*\(", src))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.lbbnn_abi_version() == 1


def test_compact_map_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    cname, cls = "lbbnn_compact_map_t", _lib.CompactMap
    fields = ("rows", "cols", "O_full", "I_full")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"),
             "int main(void) {", 'printf("size %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f in fields]
    lines += ["return 0; }"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict((l.split()[0], int(l.split()[1]))
               for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == got["size"]
    for f in fields:
        assert getattr(cls, f).offset == got[f], f


def _desc(_lib, O=4, I=8, ld=32, mnf=False, n=1, O_full=8, I_full=16):
    """Descriptors and maps whose pointers are never dereferenced: every call below must fail before launching."""
    d = (_lib.FrozenDesc * n)()
    m = (_lib.CompactMap * n)()
    for k in range(n):
        for j, name in enumerate(("weight_mu", "weight_rho", "lambdal", "bias_rho", "e0", "e_w", "var_w", "bias_var",
                                  "kept_rows")):
            setattr(d[k], name, 4096 * (j + 1))
        d[k].O, d[k].I, d[k].ld, d[k].flags, d[k].mode, d[k].cut, d[k].layer_id = O, I, ld, 0, 1, 0.0, k
        m[k].rows, m[k].cols, m[k].O_full, m[k].I_full = 4096 * 40, 4096 * 41, O_full, I_full
        if mnf:
            d[k].q0_mean, d[k].q0_log_var, d[k].z_fwd, d[k].e_w_members = 4096 * 20, 4096 * 21, 4096 * 22, 4096 * 23
            d[k].z_mstride = 32
            d[k].z_flow.T = 0
    return d, m


def test_frozen_operands_compact_argument_checks(lib):
    from bnn_amd import _lib
    f = lib.lbbnn_frozen_operands_compact
    d, m = _desc(_lib)
    assert f(None, m, 1, None) == E_NULL
    assert f(d, None, 1, None) == E_NULL
    assert f(d, m, 0, None) == E_SHAPE
    assert f(d, m, _lib.MAX_LAYERS + 1, None) == E_SHAPE
    for name in ("weight_mu", "weight_rho", "lambdal", "bias_rho", "e0", "e_w", "var_w", "bias_var", "kept_rows"):
        d, m = _desc(_lib)
        setattr(d[0], name, None)
        assert f(d, m, 1, None) == E_NULL, name
    for name in ("rows", "cols"):
        d, m = _desc(_lib)
        setattr(m[0], name, None)
        assert f(d, m, 1, None) == E_NULL, name
    assert f(*_desc(_lib, O=0), 1, None) == E_SHAPE
    assert f(*_desc(_lib, I=0), 1, None) == E_SHAPE
    assert f(*_desc(_lib, I=33, ld=32, I_full=64), 1, None) == E_SHAPE        # I' > ld'
    assert f(*_desc(_lib, O=9, O_full=8), 1, None) == E_SHAPE                 # O' > O_full
    assert f(*_desc(_lib, I=24, I_full=16), 1, None) == E_SHAPE               # I' > I_full
    assert f(*_desc(_lib, ld=48), 1, None) == E_ALIGN                         # ld % 32 != 0
    for name in ("e0", "e_w", "var_w"):                                       # 16-B vector stores
        d, m = _desc(_lib)
        setattr(d[0], name, 4096 + 4)
        assert f(d, m, 1, None) == E_ALIGN, name
    d, m = _desc(_lib)
    d[0].lambdal = 4096 + 2
    assert f(d, m, 1, None) == E_ALIGN
    d, m = _desc(_lib, I=12)
    d[0].flags = 0x4                                                          # bf16 hi | lo operands need I' % 8 == 0
    assert f(d, m, 1, None) == E_ALIGN
    for mode in (0, 2, -1):                                                   # only the median probability model
        d, m = _desc(_lib)
        d[0].mode = mode
        assert f(d, m, 1, None) == E_FLAGS, mode
    d, m = _desc(_lib)
    d[0].flags = 0x1
    assert f(d, m, 1, None) == E_FLAGS
    d, m = _desc(_lib, n=2)                                                   # the second layer is checked too
    m[1].cols = None
    assert f(d, m, 2, None) == E_NULL


def test_frozen_members_compact_argument_checks(lib):
    from bnn_amd import _lib
    f = lib.lbbnn_frozen_members_compact
    rng = ctypes.c_void_p(4096 * 30)
    d, m = _desc(_lib, mnf=True)
    assert f(None, m, 1, 1, rng, 1, None) == E_NULL
    assert f(d, None, 1, 1, rng, 1, None) == E_NULL
    assert f(d, m, 0, 1, rng, 1, None) == E_SHAPE
    assert f(d, m, _lib.MAX_LAYERS + 1, 1, rng, 1, None) == E_SHAPE
    assert f(d, m, 1, 0, rng, 1, None) == E_SHAPE
    assert f(d, m, 1, 65536, rng, 1, None) == E_SHAPE
    assert f(d, m, 1, 2, None, 1, None) == E_NOISE
    assert f(*_desc(_lib, mnf=False), 1, 2, None, 1, None) == 0               # LRT layers only: nothing launched
    for name in ("q0_log_var", "z_fwd", "e0", "e_w_members"):
        d, m = _desc(_lib, mnf=True)
        setattr(d[0], name, None)
        assert f(d, m, 1, 2, rng, 1, None) == E_NULL, name
    for name in ("rows", "cols"):
        d, m = _desc(_lib, mnf=True)
        setattr(m[0], name, None)
        assert f(d, m, 1, 2, rng, 1, None) == E_NULL, name
    assert f(*_desc(_lib, mnf=True, I=36, ld=32, I_full=64), 1, 2, rng, 1, None) == E_SHAPE
    assert f(*_desc(_lib, mnf=True, O=9, O_full=8), 1, 2, rng, 1, None) == E_SHAPE
    assert f(*_desc(_lib, mnf=True, I=24, I_full=16), 1, 2, rng, 1, None) == E_SHAPE
    d, m = _desc(_lib, mnf=True)
    d[0].z_flow.T = 17
    assert f(d, m, 1, 2, rng, 1, None) == E_SHAPE
    d[0].z_flow.T = 2                                                         # transforms without parameters
    assert f(d, m, 1, 2, rng, 1, None) == E_NULL
    d, m = _desc(_lib, mnf=True)
    d[0].z_mstride = 8                                                        # shorter than a FULL-width z vector (16)
    assert f(d, m, 1, 2, rng, 1, None) == E_SHAPE
    assert f(*_desc(_lib, mnf=True, I=6), 1, 2, rng, 1, None) == E_ALIGN
    assert f(*_desc(_lib, mnf=True, I_full=18), 1, 2, rng, 1, None) == E_ALIGN
    assert f(*_desc(_lib, mnf=True, ld=48), 1, 2, rng, 1, None) == E_ALIGN
    d, m = _desc(_lib, mnf=True)
    d[0].z_fwd = 4096 * 22 + 4
    assert f(d, m, 1, 2, rng, 1, None) == E_ALIGN
    d, m = _desc(_lib, mnf=True)
    d[0].flags = 0x2
    assert f(d, m, 1, 2, rng, 1, None) == E_FLAGS
    d, m = _desc(_lib, mnf=True, I=12)
    d[0].flags = 0x4
    assert f(d, m, 1, 2, rng, 1, None) == E_ALIGN


def test_gather_columns_argument_checks(lib):
    f = lib.lbbnn_gather_columns
    x, idx, out = 4096, 4096 * 2, 4096 * 3
    assert f(None, 16, None, 8, None, 8, 0, None) == 0                        # an empty batch: a successful no-op
    assert f(x, 16, idx, 8, out, 8, -1, None) == E_SHAPE
    assert f(None, 16, idx, 8, out, 8, 2, None) == E_NULL
    assert f(x, 16, None, 8, out, 8, 2, None) == E_NULL
    assert f(x, 16, idx, 8, None, 8, 2, None) == E_NULL
    assert f(x, 16, idx, 0, out, 8, 2, None) == E_SHAPE
    assert f(x, 16, idx, 12, out, 8, 2, None) == E_SHAPE                      # ldo < n_idx
    assert f(x, 16, idx, 8, out + 4, 8, 2, None) == E_ALIGN
    assert f(x, 16, idx, 5, out, 6, 2, None) == E_ALIGN                       # ldo % 4


# --------------------------------------------------------------------------- the Python interface
def test_freeze_compact_refusals_say_what_to_use():
    import bnn_amd
    from bnn_amd import evaluate
    torch.manual_seed(0)
    lrt = bnn_amd.lrt.BayesianNetwork((20, 16, 12, 3))
    with pytest.raises(ValueError, match="never exactly zero.*freeze\\(net, \"mpm\", compact=True\\)"):
        evaluate.freeze(lrt, compact=True)
    with pytest.raises(ValueError, match="never exactly zero"):
        evaluate.freeze(lrt, "alpha", compact=True)
    with pytest.raises(ValueError, match="dense=True.*freeze\\(net, \"mpm\", dense=True\\)"):
        evaluate.freeze(lrt, "mpm", dense=True, compact=True)
    rnvp = bnn_amd.mnf.BayesianNetwork((20, 16, 12, 3), 2, z_flow_type="RNVP", r_flow_type="RNVP")
    with pytest.raises(ValueError, match="dense coupling z flows.*freeze\\(net, \"mpm\", dense=True\\)"):
        evaluate.freeze(rnvp, "mpm", compact=True)
    with pytest.raises(RuntimeError, match="no CPU path"):                    # what passes gets as far as the device check
        evaluate.freeze(lrt, "mpm", compact=True)
    with pytest.raises(RuntimeError, match="no CPU path"):                    # ... and compact=False is today's call
        evaluate.freeze(lrt, "mpm", compact=False)


def test_compact_network_without_a_device():
    """The object itself is host logic: widths, counts and the refusal to refresh need no GPU."""
    from bnn_amd import evaluate
    dims = (64, 48, 40, 20)
    _, masks = cc.lambdals(dims)
    need, live = evaluate.live_structure(masks)
    needed = [int(n.sum()) for n in need]
    fz = evaluate.CompactFrozenNetwork(dims, live, needed, "lrt", 0.5)
    assert isinstance(fz, evaluate.FrozenNetwork) and list(fz.parameters()) == []
    assert fz.dims == cc.TABLE[dims][1] and fz.full_dims == dims and tuple(fz.needed) == cc.TABLE[dims][0]
    assert fz.gates == "mpm" and fz.cut == 0.0
    assert [t.tolist() for t in fz.live] == [t.tolist() for t in live]
    assert all(t.dtype == torch.int32 for t in fz.live)
    assert [tuple(k.shape) for k in fz.kept_rows] == [(d,) for d in fz.dims[1:]]
    assert "live_0" in dict(fz.named_buffers()) and "live_3" in dict(fz.named_buffers())
    with pytest.raises(NotImplementedError, match="freeze again"):
        fz.refresh()
    with pytest.raises(ValueError, match="boundaries"):
        evaluate.CompactFrozenNetwork(dims, live[:-1], needed, "lrt", 0.5)
