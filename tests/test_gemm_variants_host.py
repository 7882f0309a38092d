"""CPU tier of the dual-moment GEMM's variant matrix (tests/gemm_variant_cases.py): through ``ops.lrt_gemm_plan`` -- the
selection function the dispatcher itself launches from, asked on the host -- every case reaches the instantiation it claims,
and the cases together with the fan-out rows cover EVERY instantiation a sweep of the plan over the dispatcher's input space
can reach.  A shape that stops reaching its variant, or a variant the dispatcher gains without a case, fails here, without a
GPU."""
import itertools
import os

import pytest

import gemm_variant_cases as gv


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    from bnn_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    _lib.lib()
    return ops


def test_plan_symbol_bound_and_struct_matches_header(ops, tmp_path):
    import ctypes
    import subprocess
    from bnn_amd import _lib
    assert "lbbnn_lrt_gemm_plan" in _lib.SIGNATURES and len(_lib.SIGNATURES["lbbnn_lrt_gemm_plan"][1]) == 10
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "plan_size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%d %%d\\n", '
                   'sizeof(lbbnn_gemm_plan_t), offsetof(lbbnn_gemm_plan_t, kernel_id), LBBNN_GEMM_SKINNY, LBBNN_GEMM_SPLIT); '
                   'return 0; }\n' % os.path.join(root, "include", "lbbnn.h"))
    exe = tmp_path / "plan_size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, off, skinny, split = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(_lib.GemmPlan) == size and _lib.GemmPlan.kernel_id.offset == off
    assert _lib.GEMM_FAMILIES[skinny] == "skinny" and _lib.GEMM_FAMILIES[split] == "split"
    assert [ops.F_RELU, ops.F_MEAN_ONLY, ops.F_SPLIT16, ops.F_LOG_SOFTMAX, ops.F_SINGLE16, ops.F_HALF16] == \
        [gv.F_RELU, gv.F_MEAN_ONLY, gv.F_SPLIT16, gv.F_LOG_SOFTMAX, gv.F_SINGLE16, gv.F_HALF16]


def _case_plan(ops, c):
    return ops.lrt_gemm_plan(c.B, c.I, c.O, ldx=c.ldx, x_aligned=c.x_aligned, flags=c.flags)


def _family_plan(ops, row, **kw):
    name, B, I, O, mode, relu = row
    return ops.lrt_gemm_plan(B, I, O, flags=gv.mode_flags(mode, False) | (gv.F_RELU if relu else 0), **kw)


@pytest.mark.parametrize("c", gv.CASES, ids=[c.id for c in gv.CASES])
def test_case_reaches_its_variant(ops, c):
    assert gv.variant_of(_case_plan(ops, c)) == c.variant
    # ReLU, and members of a member launch, never change the kernel
    assert ops.lrt_gemm_plan(c.B, c.I, c.O, ldx=c.ldx, x_aligned=c.x_aligned, flags=c.flags ^ gv.F_RELU,
                             members=3).kernel_id == _case_plan(ops, c).kernel_id


def test_case_ids_are_unique_and_name_the_variant():
    ids = [c.id for c in gv.CASES]
    assert len(set(ids)) == len(ids)
    assert all(c.id.startswith(c.variant.name + "-B") for c in gv.CASES)


@pytest.mark.parametrize("row", gv.FAMILIES, ids=[f[0] for f in gv.FAMILIES])
def test_family_row_reaches_its_fanout_variant(ops, row):
    want = gv.FAMILY_VARIANTS[row[0]]
    fan = _family_plan(ops, row, fan=gv.FAN_MEMBERS)
    assert gv.variant_of(fan) == want
    # the members form and the single launch the test compares with take the same kernel: the non-fan twin
    one, mem = _family_plan(ops, row), _family_plan(ops, row, members=gv.FAN_MEMBERS)
    assert one.kernel_id == mem.kernel_id != fan.kernel_id
    assert gv.variant_of(one) == want._replace(fan=False)


def test_ineligible_x_layouts(ops):
    """I = 32 with the base 4 bytes off, or with ldx = 33: fp32 plans the staged kernel with scalar loads, the split kernels
    refuse (LBBNN_E_ALIGN), as the launch does."""
    for kw in gv.SPLIT_REJECTED:
        p = ops.lrt_gemm_plan(kw["B"], kw["I"], kw["O"], ldx=kw["ldx"], x_aligned=kw["x_aligned"])
        assert (p.family, p.xvec) == ("staged", False)
        for mode in ("bf16x3", "bf16", "fp16"):
            rc, plan = ops.lrt_gemm_plan_code(kw["B"], kw["I"], kw["O"], ldx=kw["ldx"], x_aligned=kw["x_aligned"],
                                              flags=gv.mode_flags(mode, False))
            assert rc == -3 and plan is None
        with pytest.raises(RuntimeError, match="lbbnn_lrt_gemm_plan"):
            ops.lrt_gemm_plan(kw["B"], kw["I"], kw["O"], ldx=kw["ldx"], x_aligned=kw["x_aligned"], flags=gv.F_SPLIT16)
    # the same width in the eligible layout is the split kernel's
    assert ops.lrt_gemm_plan(96, 32, 84, ldx=36, flags=gv.F_SPLIT16).family == "split"


def test_splitk_plan(ops):
    k = gv.SPLITK
    p = ops.lrt_gemm_plan(k["B"], k["I"], k["O"], flags=gv.F_MEAN_ONLY | gv.F_SPLIT16, kchunk=k["kchunk"])
    assert gv.variant_of(p) == k["variant"]
    # the k slabs count as workgroups: 4 slabs x 16 column tiles x 4 row tiles reach the large tile that one slab does not
    assert ops.lrt_gemm_plan(512, 200, 1204, flags=gv.F_MEAN_ONLY | gv.F_SPLIT16, kchunk=64).large_tile
    assert not ops.lrt_gemm_plan(512, 200, 1204, flags=gv.F_MEAN_ONLY | gv.F_SPLIT16).large_tile


def test_rejected_inputs_return_the_dispatchers_codes(ops):
    code = lambda *a, **kw: ops.lrt_gemm_plan_code(*a, **kw)[0]
    assert code(-1, 8, 8) == -2 and code(8, 0, 8) == -2 and code(8, 8, 0) == -2 and code(8, 8, 8, ldx=7) == -2
    assert code(8, 8, 8, members=0) == -2 and code(8, 8, 8, fan=-1) == -2
    assert code(8, 8, 8, flags=0x40) == -4
    assert code(8, 8, 8, flags=gv.F_SINGLE16) == -4                                   # single without split
    assert code(8, 8, 40, flags=gv.F_SPLIT16 | gv.F_HALF16) == -4                     # half without single
    assert code(8, 8, 40, flags=gv.F_SPLIT16 | gv.F_SINGLE16 | gv.F_HALF16 | gv.F_MEAN_ONLY) == -4
    assert code(8, 8, 17, flags=gv.F_LOG_SOFTMAX) == -4 and code(8, 8, 16, flags=gv.F_LOG_SOFTMAX | gv.F_RELU) == -4
    assert code(8, 8, 40, flags=gv.F_MEAN_ONLY, fan=3) == -4 and code(8, 8, 40, members=2, fan=3) == -4
    assert code(8, 8, 16, flags=gv.F_LOG_SOFTMAX, fan=3) == -4
    assert code(8, 64, 40, flags=gv.F_MEAN_ONLY | gv.F_SPLIT16, kchunk=64, members=2) == -4
    assert code(8, 64, 40, kchunk=64) == -4 and code(8, 64, 40, flags=gv.F_MEAN_ONLY | gv.F_SPLIT16, kchunk=48) == -3
    assert code(8, 12, 40, flags=gv.F_SPLIT16) == -3 and code(8, 8, 16, flags=gv.F_SPLIT16) == -3
    assert code(1 << 20, 512, 40, flags=gv.F_SPLIT16) == -2                           # 32-bit buffer offsets of x
    rc, p = ops.lrt_gemm_plan_code(0, 8, 8)
    assert rc == 0 and p.family == "none" and p.kernel_id == -1                       # empty batch: nothing is launched


def _accepted_flags(ops):
    """Every flag combination the dispatcher accepts for some shape (O = 16 admits LOG_SOFTMAX, I = 64 the split kernels)."""
    bits = (gv.F_RELU, gv.F_MEAN_ONLY, gv.F_SPLIT16, gv.F_LOG_SOFTMAX, gv.F_SINGLE16, gv.F_HALF16)
    out = []
    for pick in itertools.product((0, 1), repeat=len(bits)):
        f = sum(b for b, on in zip(bits, pick) if on)
        if any(ops.lrt_gemm_plan_code(37, 64, O, flags=f)[0] == 0 for O in (16, 84)):
            out.append(f)
    return out


def test_cases_cover_every_reachable_instantiation(ops):
    flags = _accepted_flags(ops)
    # fp32: 2 of mean-only x 3 of (ReLU, log-softmax); split: 5 of (mean-only, single, half) x 2 of ReLU (log-softmax needs
    # O <= 16, the split kernels O > 16)
    assert len(flags) == 16
    reachable = {}
    for B, I, O in itertools.product(gv.SWEEP_B, gv.SWEEP_I, gv.SWEEP_O):
        for ldx, aligned, f in itertools.product((I, I + 1 + (I & 1)), (True, False), flags):
            for members, fan, kchunk in ((1, 0, 0), (3, 0, 0), (1, 4, 0), (1, 0, 64), (3, 4, 0), (3, 0, 64), (1, 4, 64)):
                rc, p = ops.lrt_gemm_plan_code(B, I, O, ldx=ldx, x_aligned=aligned, flags=f, members=members, fan=fan,
                                               kchunk=kchunk)
                assert rc in (0, -2, -3, -4)
                if rc == 0:
                    v = gv.variant_of(p)
                    assert reachable.setdefault(p.kernel_id, v) == v          # one id, one instantiation
    by_variant = {v: k for k, v in reachable.items()}
    assert len(by_variant) == len(reachable)                                   # ... and one instantiation, one id
    covered = {_case_plan(ops, c).kernel_id for c in gv.CASES}
    covered |= {_family_plan(ops, row, fan=gv.FAN_MEMBERS).kernel_id for row in gv.FAMILIES}
    missing = sorted(v.name for k, v in reachable.items() if k not in covered)
    assert not missing, missing
    assert covered <= set(reachable)
    assert len(reachable) == gv.EXPECTED_INSTANTIATIONS
    # the fan-out instantiations are exactly the FAMILIES rows', the others exactly the cases'
    assert {k for k, v in reachable.items() if v.fan} == {_family_plan(ops, r, fan=gv.FAN_MEMBERS).kernel_id for r in gv.FAMILIES}
    assert {k for k, v in reachable.items() if not v.fan} == {_case_plan(ops, c).kernel_id for c in gv.CASES}
