"""CPU tier of the frozen evaluation model (include/lbbnn.h lbbnn_frozen_operands / lbbnn_frozen_members,
evaluate.freeze / FrozenNetwork): the entry points are exported and bound, the descriptor matches the header, the argument
checks return the documented codes without launching, the Python interface refuses what it cannot run and says what to use
instead, and kept / density follow from kept_rows."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lbbnn_frozen_operands", "lbbnn_frozen_members")
E_NULL, E_SHAPE, E_ALIGN, E_FLAGS, E_NOISE = -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_new_symbols_exported_and_bound_abi_unchanged(lib):
    from bnn_amd import _lib
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert lib.lbbnn_abi_version() == 1


def test_frozen_desc_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    cname, cls = "lbbnn_frozen_desc_t", _lib.FrozenDesc
    fields = ("weight_mu", "bias_rho", "q0_log_var", "z_flow", "e0", "var_w", "kept_rows", "z_fwd", "e_w_members",
              "z_mstride", "O", "ld", "flags", "mode", "cut", "layer_id")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"),
             "int main(void) {", 'printf("size %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f in fields]
    lines += ['printf("alpha %d\\n", LBBNN_FROZEN_ALPHA);', 'printf("mpm %d\\n", LBBNN_FROZEN_MPM);', "return 0; }"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict((l.split()[0], int(l.split()[1]))
               for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == got["size"]
    for f in fields:
        assert getattr(cls, f).offset == got[f], f
    assert (got["alpha"], got["mpm"]) == (0, 1)               # the modes FrozenNetwork._descs writes


def _desc(_lib, O=4, I=4, ld=32, mnf=False, n=1):
    """Descriptors whose pointers are never dereferenced: every call below must fail before launching."""
    d = (_lib.FrozenDesc * n)()
    for k in range(n):
        for j, name in enumerate(("weight_mu", "weight_rho", "lambdal", "bias_rho", "e0", "e_w", "var_w", "bias_var",
                                  "kept_rows")):
            setattr(d[k], name, 4096 * (j + 1))
        d[k].O, d[k].I, d[k].ld, d[k].flags, d[k].mode, d[k].cut, d[k].layer_id = O, I, ld, 0, 0, 0.0, k
        if mnf:
            d[k].q0_mean, d[k].q0_log_var, d[k].z_fwd, d[k].e_w_members = 4096 * 20, 4096 * 21, 4096 * 22, 4096 * 23
            d[k].z_mstride = ld
            d[k].z_flow.T = 0
    return d


def test_frozen_operands_argument_checks(lib):
    from bnn_amd import _lib
    ops_ = lib.lbbnn_frozen_operands
    assert ops_(None, 1, None) == E_NULL
    assert ops_(_desc(_lib), 0, None) == E_SHAPE
    assert ops_(_desc(_lib, n=1), _lib.MAX_LAYERS + 1, None) == E_SHAPE
    for name in ("weight_mu", "weight_rho", "lambdal", "bias_rho", "e0", "e_w", "var_w", "bias_var", "kept_rows"):
        d = _desc(_lib)
        setattr(d[0], name, None)
        assert ops_(d, 1, None) == E_NULL, name
    assert ops_(_desc(_lib, O=0), 1, None) == E_SHAPE
    assert ops_(_desc(_lib, I=0), 1, None) == E_SHAPE
    assert ops_(_desc(_lib, I=33, ld=32), 1, None) == E_SHAPE            # I > ld
    assert ops_(_desc(_lib, I=4, ld=48), 1, None) == E_ALIGN             # ld % 32 != 0
    for name in ("e0", "e_w", "var_w"):                                   # 16-B vector stores
        d = _desc(_lib)
        setattr(d[0], name, 4096 + 4)
        assert ops_(d, 1, None) == E_ALIGN, name
    d = _desc(_lib)
    d[0].lambdal = 4096 + 2                                               # not even a float boundary
    assert ops_(d, 1, None) == E_ALIGN
    d = _desc(_lib)
    d[0].flags, d[0].weight_mu = 0x4, 4096 + 4                            # bf16 hi | lo operands need aligned float4 rows
    assert ops_(d, 1, None) == E_ALIGN
    d = _desc(_lib, I=6)
    d[0].flags = 0x4                                                      # ... and I % 4 == 0
    assert ops_(d, 1, None) == E_ALIGN
    for mode in (2, -1):
        d = _desc(_lib)
        d[0].mode = mode
        assert ops_(d, 1, None) == E_FLAGS, mode
    d = _desc(_lib)
    d[0].flags = 0x1
    assert ops_(d, 1, None) == E_FLAGS
    d = _desc(_lib, n=2)                                                  # the second descriptor is checked too
    d[1].mode = 7
    assert ops_(d, 2, None) == E_FLAGS


def test_frozen_members_argument_checks(lib):
    from bnn_amd import _lib
    mem = lib.lbbnn_frozen_members
    rng = ctypes.c_void_p(4096 * 30)
    assert mem(None, 1, 1, rng, 1, None) == E_NULL
    assert mem(_desc(_lib, mnf=True), 0, 1, rng, 1, None) == E_SHAPE
    assert mem(_desc(_lib, mnf=True), _lib.MAX_LAYERS + 1, 1, rng, 1, None) == E_SHAPE
    assert mem(_desc(_lib, mnf=True), 1, 0, rng, 1, None) == E_SHAPE
    assert mem(_desc(_lib, mnf=True), 1, 65536, rng, 1, None) == E_SHAPE
    assert mem(_desc(_lib, mnf=True), 1, 2, None, 1, None) == E_NOISE     # an MNF layer draws z: rng required
    assert mem(_desc(_lib, mnf=False), 1, 2, None, 1, None) == 0          # LRT layers only: nothing to do, nothing launched
    for name in ("q0_log_var", "z_fwd", "e0", "e_w_members"):
        d = _desc(_lib, mnf=True)
        setattr(d[0], name, None)
        assert mem(d, 1, 2, rng, 1, None) == E_NULL, name
    assert mem(_desc(_lib, mnf=True, I=33, ld=32), 1, 2, rng, 1, None) == E_SHAPE
    d = _desc(_lib, mnf=True)
    d[0].z_flow.T = 17
    assert mem(d, 1, 2, rng, 1, None) == E_SHAPE
    d[0].z_flow.T = 2                                                     # transforms without parameters
    assert mem(d, 1, 2, rng, 1, None) == E_NULL
    d = _desc(_lib, mnf=True, I=8)
    d[0].z_mstride = 4                                                    # shorter than a z vector
    assert mem(d, 1, 2, rng, 1, None) == E_SHAPE
    assert mem(_desc(_lib, mnf=True, I=6), 1, 2, rng, 1, None) == E_ALIGN
    assert mem(_desc(_lib, mnf=True, ld=48), 1, 2, rng, 1, None) == E_ALIGN
    d = _desc(_lib, mnf=True)
    d[0].z_fwd = 4096 * 22 + 4
    assert mem(d, 1, 2, rng, 1, None) == E_ALIGN
    d = _desc(_lib, mnf=True)
    d[0].flags = 0x2
    assert mem(d, 1, 2, rng, 1, None) == E_FLAGS


def _early_return_rows(_lib):
    """(entry point, label, arguments, code): one row per early return of the five frozen entry points, in the order the
    code takes them.  Most rows are invalid a second time at a later check with another code, so a reordered check changes
    what comes back.  No row reaches a launch: the pointers are never dereferenced."""
    import test_frozen_compact_host as tc
    import test_frozen_dense_host as td
    BIG = 16384 + 4                                                       # > LBBNN_MAX_FLOW_DIM, % 4 == 0
    BIG_LD = 16416                                                        # >= BIG, % 32 == 0
    rng = ctypes.c_void_p(4096 * 30)
    rows = []

    def full(**kw):
        split, z_ms = kw.pop("split", False), kw.pop("z_mstride", None)
        d = _desc(_lib, **kw)
        for k in range(len(d)):
            d[k].flags = 0x4 if split else 0
            if z_ms is not None:
                d[k].z_mstride = z_ms
        return d

    def compact(**kw):
        split, z_ms = kw.pop("split", False), kw.pop("z_mstride", None)
        d, m = tc._desc(_lib, **kw)
        for k in range(len(d)):
            d[k].flags = 0x4 if split else 0
            if z_ms is not None:
                d[k].z_mstride = z_ms
        return d, m

    def dense(**kw):
        z_ms = kw.pop("z_mstride", None)
        d = td._desc(_lib, **kw)
        if z_ms is not None:
            for k in range(len(d)):
                d[k].z_mstride = z_ms
        return d

    def edit(d, k=0, **fields):
        for name, v in fields.items():
            if name == "T":
                d[k].z_flow.T = v
            else:
                setattr(d[k], name, v)
        return d

    # ---------------------------------------------------------------- lbbnn_frozen_operands(L, n, stream)
    e = "lbbnn_frozen_operands"
    rows += [
        (e, "L null, n = 0", (None, 0, None), E_NULL),
        (e, "n = 0, weight_mu null", (edit(full(), weight_mu=None), 0, None), E_SHAPE),
        (e, "n too large, e0 null", (edit(full(), e0=None), _lib.MAX_LAYERS + 1, None), E_SHAPE),
        (e, "kept_rows null, ld = 48", (edit(full(ld=48), kept_rows=None), 1, None), E_NULL),
        (e, "bias_rho null, O = 0", (edit(full(O=0), bias_rho=None), 1, None), E_NULL),
        (e, "O = 0, ld = 48", (full(O=0, ld=48), 1, None), E_SHAPE),
        (e, "I > ld, e0 misaligned", (edit(full(I=33, ld=32), e0=4096 + 4), 1, None), E_SHAPE),
        (e, "ld = 48, unknown flag", (edit(full(ld=48), flags=0x1), 1, None), E_ALIGN),
        (e, "e_w misaligned, mode 7", (edit(full(), e_w=4096 + 4, mode=7), 1, None), E_ALIGN),
        (e, "lambdal off a float, unknown flag", (edit(full(), lambdal=4096 + 2, flags=0x1), 1, None), E_ALIGN),
        (e, "unknown flag beside split, I = 6", (edit(full(I=6), flags=0x5), 1, None), E_FLAGS),
        (e, "mode 2, split with I = 6", (edit(full(I=6, split=True), mode=2), 1, None), E_FLAGS),
        (e, "split with I = 6", (full(I=6, split=True), 1, None), E_ALIGN),
        (e, "split with weight_mu off 16 B", (edit(full(split=True), weight_mu=4096 + 4), 1, None), E_ALIGN),
        # no I % 8 rule for split operands here (the compact call has it): layer 0 passes, layer 1 is what fails
        (e, "split with I = 12 passes; second layer: mode 7", (edit(full(I=12, split=True, n=2), 1, mode=7), 2, None), E_FLAGS),
        (e, "second layer: kept_rows null, ld = 48", (edit(full(n=2), 1, kept_rows=None, ld=48), 2, None), E_NULL),
    ]
    # ---------------------------------------------------------------- lbbnn_frozen_operands_compact(L, M, n, stream)
    e = "lbbnn_frozen_operands_compact"

    def cm(dm, k=0, **fields):                                            # edit the map
        for name, v in fields.items():
            setattr(dm[1][k], name, v)
        return dm

    def cd(dm, k=0, **fields):                                            # edit the descriptor
        edit(dm[0], k, **fields)
        return dm
    rows += [
        (e, "L null, n = 0", (None, compact()[1], 0, None), E_NULL),
        (e, "M null, n = 0", (compact()[0], None, 0, None), E_NULL),
        (e, "n = 0, rows null", (*cm(compact(), rows=None), 0, None), E_SHAPE),
        (e, "kept_rows null, ld = 48", (*cd(compact(ld=48), kept_rows=None), 1, None), E_NULL),
        (e, "O = 0, cols null", (*cm(compact(O=0), cols=None), 1, None), E_SHAPE),
        (e, "ld = 48, mode 0", (*cd(compact(ld=48), mode=0), 1, None), E_ALIGN),
        (e, "var_w misaligned, mode 0", (*cd(compact(), var_w=4096 + 4, mode=0), 1, None), E_ALIGN),
        (e, "lambdal off a float, mode 0", (*cd(compact(), lambdal=4096 + 2, mode=0), 1, None), E_ALIGN),
        (e, "unknown flag, cols null", (*cm(cd(compact(), flags=0x1), cols=None), 1, None), E_FLAGS),
        (e, "mode 0, cols null", (*cm(cd(compact(), mode=0), cols=None), 1, None), E_FLAGS),
        (e, "cols null, split with I = 12", (*cm(compact(I=12, split=True), cols=None), 1, None), E_NULL),
        (e, "O' > O_full, rows misaligned", (*cm(compact(O=9, O_full=8), rows=4096 * 40 + 2), 1, None), E_SHAPE),
        (e, "I' > I_full, split with I' = 20", (*compact(I=20, I_full=16, split=True), 1, None), E_SHAPE),
        (e, "cols off an int, split with I' = 12", (*cm(compact(I=12, split=True), cols=4096 * 41 + 2), 1, None), E_ALIGN),
        (e, "split with I' = 12", (*compact(I=12, split=True), 1, None), E_ALIGN),
        (e, "second layer: mode 0, cols null", (*cm(cd(compact(n=2), 1, mode=0), 1, cols=None), 2, None), E_FLAGS),
    ]
    # ---------------------------------------------------------------- lbbnn_frozen_members(L, n, members, rng, adv, stream)
    e = "lbbnn_frozen_members"
    mf = lambda **kw: full(mnf=True, **kw)
    rows += [
        (e, "L null, n = 0", (None, 0, 1, rng, 1, None), E_NULL),
        (e, "n = 0, e0 null", (edit(mf(), e0=None), 0, 1, rng, 1, None), E_SHAPE),
        (e, "members = 0, q0_log_var null", (edit(mf(), q0_log_var=None), 1, 0, rng, 1, None), E_SHAPE),
        (e, "q0_log_var null, T = 17", (edit(mf(), q0_log_var=None, T=17), 1, 2, rng, 1, None), E_NULL),
        (e, "T = 17, no rng", (edit(mf(), T=17), 1, 2, None, 1, None), E_SHAPE),
        (e, "transforms without parameters, no rng", (edit(mf(), T=2), 1, 2, None, 1, None), E_NULL),
        (e, "no rng, O = 0", (mf(O=0), 1, 2, None, 1, None), E_NOISE),
        (e, "O = 0, ld = 48", (mf(O=0, ld=48), 1, 2, rng, 1, None), E_SHAPE),
        # the flow runs at I: refused beyond LBBNN_MAX_FLOW_DIM (the compact call has no such test of I')
        (e, "I > LBBNN_MAX_FLOW_DIM, z_fwd misaligned", (edit(mf(I=BIG, ld=BIG_LD), z_fwd=4096 * 22 + 4), 1, 2, rng, 1, None), E_SHAPE),
        (e, "z_mstride < I, ld = 48", (mf(I=8, ld=48, z_mstride=4), 1, 2, rng, 1, None), E_SHAPE),
        (e, "ld = 48, unknown flag", (edit(mf(ld=48), flags=0x2), 1, 2, rng, 1, None), E_ALIGN),
        (e, "I = 6, unknown flag", (edit(mf(I=6), flags=0x2), 1, 2, rng, 1, None), E_ALIGN),
        (e, "z_fwd misaligned, unknown flag", (edit(mf(), z_fwd=4096 * 22 + 4, flags=0x2), 1, 2, rng, 1, None), E_ALIGN),
        (e, "unknown flag", (edit(mf(), flags=0x2), 1, 2, rng, 1, None), E_FLAGS),
        (e, "split with I = 12 passes; second layer: unknown flag", (edit(mf(I=12, split=True, n=2), 1, flags=0x2), 2, 2, rng, 1, None),
         E_FLAGS),
        (e, "first layer LRT; second layer: no rng, O = 0", (edit(edit(mf(n=2), 0, q0_mean=None), 1, O=0), 2, 2, None, 1, None), E_NOISE),
    ]
    # ---------------------------------------------------------------- lbbnn_frozen_members_dense(L, F, n, members, rng, adv, stream)
    e = "lbbnn_frozen_members_dense"
    flows, keep = td._flows(_lib, n=2)
    rows += [
        (e, "L null, n = 0", (None, flows, 0, 1, rng, 1, None), E_NULL),
        (e, "F null, n = 0", (dense(), None, 0, 1, rng, 1, None), E_NULL),
        (e, "members = 65536, z_fwd null", (edit(dense(), z_fwd=None), flows, 1, 65536, rng, 1, None), E_SHAPE),
        (e, "e_w_members null, no rng", (edit(dense(), e_w_members=None), flows, 1, 2, None, 1, None), E_NULL),
        (e, "z_flow.T is not read: no rng, O = 0", (edit(dense(O=0), T=99), flows, 1, 2, None, 1, None), E_NOISE),
        (e, "I > LBBNN_MAX_FLOW_DIM, z_fwd misaligned", (edit(dense(I=BIG, ld=BIG_LD), z_fwd=4096 * 22 + 8), flows, 1, 2, rng, 1, None),
         E_SHAPE),
        (e, "z_mstride < I, ld = 48", (dense(I=8, ld=48, z_mstride=4), flows, 1, 2, rng, 1, None), E_SHAPE),
        (e, "z_mstride % 4, unknown flag", (edit(dense(z_mstride=34), flags=0x2), flows, 1, 2, rng, 1, None), E_ALIGN),
        (e, "e0 misaligned, unknown flag", (edit(dense(), e0=4096 * 5 + 4, flags=0x2), flows, 1, 2, rng, 1, None), E_ALIGN),
        (e, "unknown flag", (edit(dense(), flags=0x2), flows, 1, 2, rng, 1, None), E_FLAGS),
        (e, "second layer: z_mstride < I, ld = 48", (edit(dense(n=2), 1, ld=48, z_mstride=4), flows, 2, 2, rng, 1, None), E_SHAPE),
    ]
    # ---------------------------------------------------------------- lbbnn_frozen_members_compact(L, M, n, members, rng, adv, stream)
    e = "lbbnn_frozen_members_compact"
    mc = lambda **kw: compact(mnf=True, **kw)
    rows += [
        (e, "L null, members = 0", (None, mc()[1], 1, 0, rng, 1, None), E_NULL),
        (e, "M null, members = 0", (mc()[0], None, 1, 0, rng, 1, None), E_NULL),
        (e, "members = 65536, rows null", (*cm(mc(), rows=None), 1, 65536, rng, 1, None), E_SHAPE),
        (e, "e0 null, T = 17", (*cd(mc(), e0=None, T=17), 1, 2, rng, 1, None), E_NULL),
        (e, "T = 17, no rng", (*cd(mc(), T=17), 1, 2, None, 1, None), E_SHAPE),
        (e, "transforms without parameters, no rng", (*cd(mc(), T=2), 1, 2, None, 1, None), E_NULL),
        (e, "no rng, O = 0", (*mc(O=0), 1, 2, None, 1, None), E_NOISE),
        (e, "O = 0, rows null", (*cm(mc(O=0), rows=None), 1, 2, rng, 1, None), E_SHAPE),
        # no test of I' against LBBNN_MAX_FLOW_DIM (the flow runs at I_full): the map's null pointer is what is found
        (e, "I' > LBBNN_MAX_FLOW_DIM is not refused as such: rows null",
         (*cm(mc(I=BIG, ld=BIG_LD, I_full=BIG + 4, z_mstride=BIG_LD), rows=None), 1, 2, rng, 1, None), E_NULL),
        (e, "rows null, z_mstride < I_full", (*cm(mc(z_mstride=8), rows=None), 1, 2, rng, 1, None), E_NULL),
        (e, "O' > O_full, z_fwd misaligned", (*cd(mc(O=9, O_full=8), z_fwd=4096 * 22 + 4), 1, 2, rng, 1, None), E_SHAPE),
        (e, "cols off an int, z_mstride < I_full", (*cm(mc(z_mstride=8), cols=4096 * 41 + 2), 1, 2, rng, 1, None), E_ALIGN),
        (e, "I_full > LBBNN_MAX_FLOW_DIM, ld = 48", (*mc(ld=48, I_full=BIG, z_mstride=BIG_LD), 1, 2, rng, 1, None), E_SHAPE),
        (e, "z_mstride < I_full, ld = 48", (*mc(ld=48, z_mstride=8), 1, 2, rng, 1, None), E_SHAPE),
        (e, "I_full % 4, unknown flag", (*cd(mc(I_full=18), flags=0x2), 1, 2, rng, 1, None), E_ALIGN),
        (e, "z_fwd misaligned, unknown flag", (*cd(mc(), z_fwd=4096 * 22 + 4, flags=0x2), 1, 2, rng, 1, None), E_ALIGN),
        (e, "unknown flag beside split, I' = 12", (*cd(mc(I=12), flags=0x6), 1, 2, rng, 1, None), E_FLAGS),
        (e, "split with I' = 12", (*mc(I=12, split=True), 1, 2, rng, 1, None), E_ALIGN),
        (e, "second layer: I_full % 4, unknown flag", (*cd(cm(mc(n=2), 1, I_full=18), 1, flags=0x2), 2, 2, rng, 1, None), E_ALIGN),
    ]
    return rows, keep


def test_frozen_entry_points_early_return_order(lib):
    """Every early return of lbbnn_frozen_operands, lbbnn_frozen_operands_compact, lbbnn_frozen_members,
    lbbnn_frozen_members_dense and lbbnn_frozen_members_compact, in the order each entry point takes them, with the two
    places where the full and the compact calls differ on purpose: I against LBBNN_MAX_FLOW_DIM (members) and I % 8 with
    the split flag (operands, members)."""
    from bnn_amd import _lib
    rows, keep = _early_return_rows(_lib)
    assert {r[0] for r in rows} == {"lbbnn_frozen_operands", "lbbnn_frozen_operands_compact", "lbbnn_frozen_members",
                                    "lbbnn_frozen_members_dense", "lbbnn_frozen_members_compact"}
    got = [(entry, label, getattr(lib, entry)(*args)) for entry, label, args, _ in rows]
    assert got == [(entry, label, code) for entry, label, _, code in rows]


def test_freeze_refusals_say_what_to_use():
    import bnn_amd
    from bnn_amd import evaluate
    torch.manual_seed(0)
    lrt = bnn_amd.lrt.BayesianNetwork((20, 16, 12, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.freeze(lrt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.freeze(bnn_amd.mnf.BayesianNetwork((20, 16, 12, 3), 2, z_flow_type="Planar", r_flow_type="Planar"), "mpm")
    with pytest.raises(ValueError, match="'alpha'.*'mpm'"):
        evaluate.freeze(lrt, gates="sample")
    for t in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="threshold"):
            evaluate.freeze(lrt, "mpm", threshold=t)
    with pytest.raises(TypeError, match='gates="mpm"'):
        evaluate.freeze(bnn_amd.base.BayesianNetwork((20, 16, 12, 3)))
    with pytest.raises(TypeError, match="vd_ensemble"):
        evaluate.freeze(bnn_amd.vd.BNN((20, 16, 12, 3)))
    with pytest.raises(TypeError, match="lrt.BayesianNetwork"):
        evaluate.freeze(torch.nn.Linear(4, 4))


def test_layer_refusals_of_freeze():
    """What a frozen model cannot represent is refused before anything else (so also without a device); a network that
    passes these checks gets as far as the device check."""
    import bnn_amd
    from bnn_amd import evaluate
    torch.manual_seed(0)
    planar = dict(z_flow_type="Planar", r_flow_type="Planar")
    lrt = bnn_amd.lrt.BayesianNetwork((20, 16, 12, 3))
    lrt.l2.noise = {"eps_out": torch.zeros(5, 12)}
    with pytest.raises(ValueError, match="injected noise.*batched=False"):
        evaluate.freeze(lrt)
    lrt.l2.noise = None
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.freeze(lrt)
    with pytest.raises(RuntimeError, match="no CPU path"):                # outside the member rule: an LRT network still freezes
        evaluate.freeze(bnn_amd.lrt.BayesianNetwork((21, 16, 12, 3)))
    with pytest.raises(ValueError, match="planar flows.*ensemble_forward"):
        evaluate.freeze(bnn_amd.mnf.BayesianNetwork((20, 16, 12, 3), 2, z_flow_type="RNVP", r_flow_type="RNVP"))
    with pytest.raises(ValueError, match="at most 4 transforms.*ensemble_forward"):
        evaluate.freeze(bnn_amd.mnf.BayesianNetwork((20, 16, 12, 3), 5, **planar), "mpm")
    with pytest.raises(ValueError, match="in_features % 4 == 0.*ensemble_forward"):
        evaluate.freeze(bnn_amd.mnf.BayesianNetwork((22, 16, 12, 3), 2, **planar))
    mnf = bnn_amd.mnf.BayesianNetwork((20, 16, 12, 3), 2, **planar)
    mnf.l1.as_written = True
    with pytest.raises(ValueError, match="as_written"):
        evaluate.freeze(mnf)
    mnf.l1.as_written = False
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.freeze(mnf)


def test_frozen_network_constructor_refusals():
    from bnn_amd import evaluate
    with pytest.raises(ValueError, match="'alpha'.*'mpm'"):
        evaluate.FrozenNetwork((20, 16, 12, 3), "lrt", "sample")
    with pytest.raises(ValueError, match="threshold"):
        evaluate.FrozenNetwork((20, 16, 12, 3), "lrt", "mpm", 1.0)
    with pytest.raises(ValueError, match="family"):
        evaluate.FrozenNetwork((20, 16, 12, 3), "base")
    fz = evaluate.FrozenNetwork((20, 16, 12, 3), "lrt", "mpm")
    assert list(fz.parameters()) == []                                    # buffers only
    assert fz.cut == 0.0 and fz.gates == "mpm" and fz.threshold == 0.5 and fz.dims == (20, 16, 12, 3)
    with pytest.raises(RuntimeError, match="evaluate.freeze"):
        fz.refresh()                                                      # not bound to a network


def test_ensemble_forward_refusals():
    import bnn_amd
    from bnn_amd import evaluate
    torch.manual_seed(0)
    x = torch.rand(5, 20)
    lrt = bnn_amd.lrt.BayesianNetwork((20, 16, 12, 3))
    with pytest.raises(ValueError, match="evaluate.freeze"):              # still a ValueError; now it says where to go
        evaluate.ensemble_forward(lrt, x, 3, gates="mpm")
    mnf = bnn_amd.mnf.BayesianNetwork((20, 16, 12, 3), 2, z_flow_type="Planar", r_flow_type="Planar")
    with pytest.raises(ValueError, match="evaluate.freeze"):
        evaluate.ensemble_forward(mnf, x, 3, gates="mpm")
    fz = evaluate.FrozenNetwork((20, 16, 12, 3), "lrt", "alpha")
    for g in ("mpm", "alpha"):
        with pytest.raises(ValueError, match="fixed by evaluate.freeze"):
            evaluate.ensemble_forward(fz, x, 3, gates=g)
    with pytest.raises(ValueError, match="batched"):
        evaluate.ensemble_forward(fz, x, 3, batched=False)


@pytest.mark.parametrize("threshold", [0.5, 0.1, 0.9])
def test_kept_and_density_follow_kept_rows(threshold):
    from bnn_amd import evaluate
    dims = (20, 16, 12, 3)
    fz = evaluate.FrozenNetwork(dims, "mnf", "mpm", threshold)
    cut = torch.logit(torch.tensor(threshold, dtype=torch.float64)).float()
    assert fz.cut == float(cut)
    g = torch.Generator().manual_seed(3)
    kept, total = [], 0
    for i in range(3):
        lam = torch.empty(dims[i + 1], dims[i]).uniform_(-3, 3, generator=g)
        rows = (lam > cut).sum(1)
        fz.kept_rows[i].copy_(rows)
        assert fz.kept_rows[i].dtype == torch.int32 and fz.kept_rows[i].shape == (dims[i + 1],)
        kept.append(int(rows.sum()))
        total += lam.numel()
    assert fz.kept == kept
    assert isinstance(fz.density, float) and fz.density == sum(kept) / total
    assert 0.0 < fz.density < 1.0


def test_unbound_models_deep_copy_and_a_full_model_has_the_compact_surface():
    import copy
    from bnn_amd import evaluate
    dims = (20, 16, 12, 3)
    fz = evaluate.FrozenNetwork(dims, "mnf", "mpm", 0.3)
    live = [torch.arange(8, dtype=torch.int32), torch.arange(8, dtype=torch.int32), torch.arange(8, dtype=torch.int32),
            torch.arange(3, dtype=torch.int32)]
    cp = evaluate.CompactFrozenNetwork(dims, live, [5, 6, 7, 3], "lrt", 0.3)
    for m in (fz, cp):
        twin = copy.deepcopy(m)
        assert type(twin) is type(m) and twin is not m
        assert (twin.dims, twin.full_dims, twin.gates, twin.cut) == (m.dims, m.full_dims, m.gates, m.cut)
        assert sorted(dict(twin.named_buffers())) == sorted(dict(m.named_buffers()))
        assert twin.kept_rows[0].data_ptr() != m.kept_rows[0].data_ptr()
    assert cp.compact and cp.dims == (8, 8, 8, 3) and cp.full_dims == dims
    # a full model: the surface of a full FrozenBaseNetwork
    base = evaluate.FrozenBaseNetwork(dims, "mpm", 0.3)
    assert fz.full_dims == fz.dims == dims and not fz.compact and not base.compact
    for what in ("live", "active_kept", "active_density"):
        for m in (fz, base):
            with pytest.raises(RuntimeError, match="belongs to a compact model"):
                getattr(m, what)
