"""CPU tier of the planar vector-backward tests (tests/test_planar_vector_backward_gpu.py): the case table reaches what it
says it reaches, and the reference alone holds the bars the kernels are held to.

1. ``form(I, Tz, Tr)`` of every tabled case is the tabled form, every form has at least three cases, both kernels reach
   the chain forms, and (4096, ., 1, 1) sits exactly on the 144 KiB limit (4097 is the first shape beyond it).
2. E32: autograd of F in float32 against float64 over the whole table, with and without the KL branch, seeds 0-5.
   Measured on a CPU: vector leaves 1.59e-5 max-norm at most, element-wise remainder 3.6e-6 of the max at most; of 1668
   one-element leaves 3 need a bar above 5e-5 (worst E32 2.7e-5, so a bar of 1.1e-4); 10 of the 114 draws were redrawn
   by the conditioning rule of planar_vector_ref (two redraws at most).  The same for F1 (V1): vectors 1.4e-5,
   remainder 0, aux[0] 6.3e-6, no redraw.  The float32 figures depend on the CPU's vector width (another machine gave
   1.9e-5 for V1 before its draws came under the same rule), which is why the rule and not a list of seeds keeps a draw."""
import pytest
import torch

import planar_vector_ref as pv

SEEDS = range(6)


def test_every_case_takes_the_form_it_is_tabled_under():
    seen = set()
    for f, I, O, Tz, Tr, route in pv.ALL_CASES:
        assert pv.form(I, Tz, Tr) == f, (I, Tz, Tr)
        assert 0 <= Tz <= 16 and 0 <= Tr <= 16
        if route == "batch":                         # the batch kernel takes flows of at most four transforms
            assert Tz <= pv.REG_MAX_T and Tr <= pv.REG_MAX_T
        seen.add((f, route))
    for f in ("reg", "lds", "global"):
        assert len(pv.CASES[f]) >= 3, f
    assert {("lds", "single"), ("lds", "batch"), ("global", "single"), ("global", "batch")} <= seen


def test_the_lds_limit_and_the_raise_threshold_are_straddled():
    assert 4 * pv.workspace_floats(4096, 1, 1) == pv.LDS_LIMIT == 147456
    assert pv.form(4096, 1, 1) == "lds" and pv.form(4097, 1, 1) == "global"
    assert pv.workspace_floats(5, 3, 3) == 5 * (2 * 4 + 3 + 4)
    sizes = {c[:4]: 4 * pv.workspace_floats(c[0], c[2], c[3]) for c in pv.CASES["lds"]}
    assert sizes[(257, 3, 16, 16)] <= pv.LDS_RAISE < sizes[(1025, 3, 5, 1)] < sizes[(4096, 3, 1, 1)]
    assert pv.LDS_RAISE < sizes[(2049, 3, 1, 1)] < sizes[(4096, 3, 1, 1)]
    # the ownership edges of element I - 1: thread (I - 1) % 1024, first or second element of its thread
    assert {1, 1024, 1025, 2048} <= {c[0] for c in pv.CASES["reg"]}
    assert pv.form(2048, 4, 4) == "reg" and pv.form(2049, 4, 4) == "global" and pv.form(1025, 5, 1) == "lds"


def test_a_leaf_outside_the_objective_has_an_exactly_zero_reference():
    d = pv.make_inputs(5, 7, 3, 3, 0)
    r = pv.v2_reference(d, 3, 3, False)
    for k, v in r.items():
        zero = k.startswith(("r0_b", "r_flow"))
        assert (float(v.abs().max()) == 0.0) == zero, k
    r = pv.v2_reference(d, 3, 3, False, dz_fwd=False, gv_sum=False)
    assert all(float(v.abs().max()) == 0.0 for k, v in r.items() if k != "bias_mu")


@pytest.fixture(scope="module")
def e32_table():
    rows = []
    for f, I, O, Tz, Tr, _ in pv.ALL_CASES:
        for seed in SEEDS:
            d = pv.make_inputs(I, O, Tz, Tr, seed)
            for has_kl in (True, False):
                rows.append(((I, O, Tz, Tr, seed, has_kl),) + pv.e32_of(d, Tz, Tr, has_kl))
    return rows


def test_reference_in_float32_holds_the_vector_bars(e32_table):
    wv = max(r[1] for r in e32_table)
    wr = max(r[2] for r in e32_table)
    print("E32 vector max-norm %.3g, element-wise remainder %.3g" % (wv, wr))
    assert wv <= pv.E32_VEC < pv.VEC_BAR
    assert wr <= pv.E32_REM and 3 * pv.E32_REM <= 5e-5
    assert pv.A_ELEM <= 3 * pv.E32_REM              # (three times the measured remainder, which the line above bounds)


def test_reference_in_float32_holds_the_one_element_bars(e32_table):
    scal = [e for r in e32_table for e in r[3]]
    wide = [e for e in scal if max(pv.SCALAR_FLOOR, 4 * e) > pv.SCALAR_FLOOR]
    print("one-element leaves %d, bar above the floor %d, worst E32 %.3g" % (len(scal), len(wide), max(scal)))
    assert len(scal) >= 1308                        # the flow biases alone; the leaves at I = 1 and O = 1 come on top
    assert len(wide) <= pv.SCALAR_WIDE_FRAC * len(scal)
    assert 4 * max(scal) <= pv.SCALAR_CEIL


def test_the_conditioning_rule_redraws_rarely_and_from_the_reference_alone():
    n = sum(pv.redraws(I, O, Tz, Tr, s) for _, I, O, Tz, Tr, _ in pv.ALL_CASES for s in SEEDS)
    assert n <= len(pv.ALL_CASES) * len(SEEDS) // 4, n
    # first draw: the generator's seed is the case's seed
    I, O, Tz, Tr = 5, 7, 3, 3
    assert pv.redraws(I, O, Tz, Tr, 0) == 0
    assert torch.equal(pv.make_inputs(I, O, Tz, Tr, 0)["q0_mean"], pv.draw_inputs(I, O, Tz, Tr, 0)["q0_mean"])


def test_v1_reference_in_float32_holds_the_bars():
    wv = wr = ws = 0.0
    for O, I in pv.V1_CASES:
        for seed in SEEDS:
            vec, rem, scal = pv.v1_e32_of(pv.make_v1_inputs(O, I, seed))
            wv, wr, ws = max(wv, vec), max(wr, rem), max(ws, scal)
    print("V1 E32: vector %.3g, remainder %.3g, one-element %.3g" % (wv, wr, ws))
    assert wv <= pv.E32_VEC and wr <= pv.E32_REM
    assert 4 * ws <= pv.SCALAR_FLOOR                 # no one-element leaf of V1 needs a bar above the floor
