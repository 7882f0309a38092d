"""CPU tier of the planar-flow forward / KL-tail form tests (tests/planar_forward_ref.py, tests/test_planar_forward_forms_gpu.py):
the restatement of K3 and K5 against the oracle, the conditioning of every table case, the narrowness of the one-number bars
(all from the references alone), and the kernel form of every table case through lbbnn_flow_planar_form /
lbbnn_kl_finalize_form -- the functions the launchers launch from -- so that a changed budget or threshold fails here
instead of silently moving cases to another kernel.  No GPU is touched.

Figures when this was written (printed on every run): restatement against oracle.mnf_forward at most 7.4e-16 relative; the
smallest share of a KL term 0.094 over the K5 inputs; 1068 one-number bars of K3 over 178 input sets, none above the 5e-6 S
floor (worst 4 E32 / S = 1.5e-6), 43 of K5, none above the floor; 312 transforms on the abs() branch of the log-det, 4 with a
saturated tanh, 4 with an argument below 1e-3 (one of each per kernel form)."""
import ctypes
import math

import pytest
import torch

import planar_forward_ref as pf
from oracle import lbbnn_oracle as orc


def _all_k3_inputs():
    """(tag, inputs, Tz, Tr) of every K3 input set the GPU tier uses: the single-entry table and the batched groups."""
    for c in pf.K3_CASES:
        form, I, Tz, Tr, kl, off, sp = c
        yield pf.k3_id(c), pf.make_inputs(I, pf.K3_O, Tz, Tr, 0, sp), Tz, Tr
    for name, (form, layers) in pf.PREPARE_GROUPS.items():
        for k, (I, O, Tz, Tr, kl, mnf) in enumerate(layers):
            if mnf:
                yield "%s[%d]" % (name, k), pf.make_inputs(I, O, Tz, Tr, 10 + k), Tz, Tr


# --------------------------------------------------------------------------- the restatement against the oracle
@pytest.mark.parametrize("I,O,Tz,Tr", [(5, 3, 2, 2), (257, 17, 3, 2), (1025, 4, 1, 4)])
def test_restatement_reproduces_the_oracle(I, O, Tz, Tr):
    d = {k: v.double() for k, v in pf.make_inputs(I, O, Tz, Tr, 7).items()}
    p = {k: v.double() for k, v in orc.init_mnf_params(I, O, torch.Generator().manual_seed(1)).items()}
    for k in ("q0_mean", "q0_log_var", "r0_b1", "r0_b2", "bias_mu", "bias_rho"):
        p[k] = d[k]
    flows = [orc.Flow("Planar", [{"u": u, "w": w, "bias": b} for u, w, b in pf.flow_params(d, fl, T)]) for fl, T in (("z", Tz), ("r", Tr))]
    noise = {"eps_z": d["eps_fwd"][None, :], "eps_z2": d["eps_kl"][None, :], "eps_act": d["eps_act"], "eps_out": torch.zeros(1, O).double()}
    _, kl, it = orc.mnf_forward(torch.ones(1, I).double(), p, flows[0], flows[1], noise)
    k3 = pf.k3_reference(d, True)
    worst = 0.0

    def close(name, got, ref):
        nonlocal worst
        err = abs(float(got) - float(ref)) / max(abs(float(ref)), 1e-300)
        worst = max(worst, err)
        assert err <= 1e-12, (name, float(got), float(ref))

    close("log_det_q", k3["scal"][0], it["log_det_q"])
    close("log_q0", k3["scal"][1], it["log_q0"])
    close("log_det_r", k3["scal"][2], it["log_det_r"].sum())
    close("z_b[-1]", k3["scal"][3], it["z_b"][-1])
    assert pf.rel_err(k3["z_fwd"], it["z_k"]) <= 1e-12 and pf.rel_err(k3["z_kl"], it["z2"]) <= 1e-12
    # K5 on what the oracle's weight pass gives; scal stays float64 here (the kernels' float32 read is not the oracle's)
    k5_in = dict(d, kl_rows=orc.kl_weight_elem(p["weight_mu"] * it["z2"], orc.sigma_of(p["weight_rho"]), it["alpha"],
                                               orc.Priors()).sum(1), act_mu=it["act_mu"], act_var=it["act_var"])
    s = torch.tensor(k3["scal"][:4], dtype=torch.float64)
    m = pf._act_mean(k5_in, torch.float64)
    log_rb = pf._log_rb(s[3], d["r0_b1"], d["r0_b2"], m)
    close("log_rb", log_rb, it["log_rb"])
    kl_mine = (k5_in["kl_rows"].sum() + orc.kl_bias_term(d["bias_mu"], d["bias_rho"], orc.Priors())) + (-s[0] + s[1]) - (s[2] + log_rb)
    close("kl", kl_mine, kl)
    # ... and k5_reference is those lines: with scal representable in float32 it returns the same number
    s32 = s.float()
    r = pf.k5_reference(k5_in, s32)
    log_rb32 = pf._log_rb(s32[3].double(), d["r0_b1"], d["r0_b2"], m)
    kl32 = (k5_in["kl_rows"].sum() + orc.kl_bias_term(d["bias_mu"], d["bias_rho"], orc.Priors())) + (-s32[0].double() + s32[1].double()) \
        - (s32[2].double() + log_rb32)
    close("k5_reference", r["kl"], kl32)
    print("restatement (%d, %d, %d, %d): worst relative difference %.3g" % (I, O, Tz, Tr, worst))


# --------------------------------------------------------------------------- the conditioning of the inputs
def test_every_k3_input_set_is_conditioned_and_the_edges_are_present():
    seen = {"negative": 0, "saturated": 0, "tiny": 0}
    sets = 0
    for tag, d, Tz, Tr in _all_k3_inputs():
        assert pf.conditioned(d, Tz, Tr) == [], tag
        lv = d["q0_log_var"]
        assert float(lv.min()) >= -9.0 and float(lv.max()) <= 1.0, tag
        r = pf.k3_reference(d, True)
        for path in ("fwd", "kl"):
            for fl, t, inner, arg, ld in r["diag"][path]:
                assert abs(ld) >= pf.MIN_LD and abs(arg) >= pf.MIN_ARG, (tag, path, fl, t)
                seen["negative"] += arg < 0
                seen["saturated"] += abs(inner) > 6
                seen["tiny"] += abs(inner) < 1e-3
            if Tz:
                assert r["disp_" + path] >= pf.MIN_DISPLACEMENT, (tag, path)
        sets += 1
    print("input sets %d; transforms with 1 + (1 - th^2) u.w < 0: %d, |inner| > 6: %d, |inner| < 1e-3: %d" % (
        sets, seen["negative"], seen["saturated"], seen["tiny"]))
    assert all(v >= 1 for v in seen.values()), seen
    # each of the four forms meets each edge in its own single-entry table
    for form in (pf.GENERIC, pf.LDS, pf.FAST, pf.VEC):
        got = set()
        for c in pf.K3_CASES:
            if c[0] != form or not c[4]:
                continue
            r = pf.k3_reference(pf.make_inputs(c[1], pf.K3_O, c[2], c[3], 0, c[6]), True)
            for fl, t, inner, arg, ld in r["diag"]["kl"]:
                got |= {"negative"} if arg < 0 else set()
                got |= {"saturated"} if abs(inner) > 6 else set()
                got |= {"tiny"} if abs(inner) < 1e-3 else set()
        assert got == {"negative", "saturated", "tiny"}, (pf.FORM_NAME[form], got)


def _k5_sets():
    for form, O, I, mnf in pf.K5_CASES:
        yield "k5 %r" % ((O, I, mnf),), pf.make_k5_inputs(O, I, 0, mnf), mnf
    for name, (staged, layers, draws, adv) in pf.FINALIZE_GROUPS.items():
        if not draws:                                  # (with in-kernel draws eps_act is the kernel's own: measured on the GPU)
            for k, (O, I, mnf, active) in enumerate(layers):
                yield "%s[%d]" % (name, k), pf.make_k5_inputs(O, I, 20 + k, mnf), mnf


def test_every_term_of_the_k5_inputs_is_visible():
    worst = 1.0
    for tag, d, mnf in _k5_sets():
        r = pf.k5_reference(d, d["scal_k5"] if mnf else None)
        assert len([t for t in r["terms"] if t != 0.0]) == (5 if mnf else 2), tag
        share = pf.smallest_term_share(r)
        worst = min(worst, share)
        assert share >= 0.01, (tag, share, r["terms"])
    print("smallest share of a KL term: %.3g" % worst)


# --------------------------------------------------------------------------- the bars
def _narrow(bars, what):
    """bars: [(bar, S)].  At most WIDE_FRAC of them above the TIGHT S floor, none above TOL S."""
    wide = [(b, S) for b, S in bars if b > pf.TIGHT * S]
    print("%s: %d one-number bars, %d above the floor, worst bar / S = %.3g" % (what, len(bars), len(wide), max(b / S for b, S in bars)))
    assert len(wide) <= pf.WIDE_FRAC * len(bars), wide[:5]
    assert all(b <= pf.TOL * S for b, S in bars)


def test_k3_one_number_bars_stay_narrow():
    bars, worst32 = [], 0.0
    for tag, d, Tz, Tr in _all_k3_inputs():
        for kl in (True, False):
            r64, r32 = pf.k3_reference(d, kl), pf.k3_reference(d, kl, torch.float32)
            bars += list(pf.k3_bars(r64, r32).values())
            for i, nme in enumerate(pf.SCAL_NAMES):
                if not math.isnan(r64["scal"][i]):
                    worst32 = max(worst32, 4 * abs(r32["scal"][i] - r64["scal"][i]) / r64["S"][nme])
            # the float32 restatement itself holds the vector bar with room to spare: the bar measures the kernel, not the inputs
            assert pf.rel_err(r32["z_fwd"], r64["z_fwd"]) < pf.TIGHT / 2, tag
    print("worst 4 E32 / S = %.3g" % worst32)
    assert len(bars) >= 500
    _narrow(bars, "K3")


def test_k5_one_number_bars_stay_narrow():
    bars = []
    for tag, d, mnf in _k5_sets():
        s = d["scal_k5"] if mnf else None
        r64, r32 = pf.k5_reference(d, s), pf.k5_reference(d, s, torch.float32)
        bars.append((pf.k5_bar(r64, r32), r64["S"]))
    assert len(bars) >= 30
    _narrow(bars, "K5")


# --------------------------------------------------------------------------- the forms, from the library's own rule
def test_symbols_are_registered():
    from bnn_amd import _lib
    assert len(_lib.SIGNATURES["lbbnn_flow_planar_form"][1]) == 7 and len(_lib.SIGNATURES["lbbnn_kl_finalize_form"][1]) == 6
    assert _lib.lib().lbbnn_abi_version() == 1            # two new symbols, no struct changed: the same ABI


@pytest.mark.parametrize("case", pf.K3_CASES, ids=pf.k3_id)
def test_k3_case_takes_the_form_its_table_names(case):
    assert pf.k3_case_form(case) == case[0]


def test_k3_tables_cover_every_form_and_boundary():
    for form in (pf.GENERIC, pf.LDS, pf.FAST, pf.VEC):
        assert sum(1 for c in pf.K3_CASES if c[0] == form) >= 6, pf.FORM_NAME[form]
    one = lambda I, Tz, Tr, kl=1, al=1, members=1: pf.k3_form([(I, Tz, Tr, kl, al)], members)
    assert pf.need_bytes(3072, 2, 2, True) == pf.LDS_BUDGET                       # exactly the budget
    assert (one(3072, 2, 2), one(3073, 2, 2)) == (pf.FAST, pf.GENERIC)
    assert (one(2048, 2, 2), one(2052, 2, 2)) == (pf.VEC, pf.FAST)
    assert (one(1025, 8, 6), one(1025, 8, 7)) == (pf.LDS, pf.GENERIC)
    assert pf.need_bytes(1025, 8, 6, True) > pf.LDS_RAISE and pf.need_bytes(1025, 3, 2, True) < pf.LDS_RAISE
    assert (one(256, 2, 2), one(256, 2, 2, al=0), one(254, 2, 2)) == (pf.VEC, pf.FAST, pf.FAST)
    assert (one(256, 2, 2), one(256, 2, 3), one(256, 2, 3, kl=0)) == (pf.VEC, pf.LDS, pf.VEC)      # Tr counts with the KL branch only
    assert (one(3073, 2, 2), one(3073, 2, 2, kl=0)) == (pf.GENERIC, pf.FAST)
    for name, (form, layers) in pf.PREPARE_GROUPS.items():
        flows = [(I, Tz, Tr, kl, 1) for I, O, Tz, Tr, kl, mnf in layers if mnf]
        assert pf.k3_form(flows) == form, name
        # ... and the companion is what moves the (2, 2) layer of the group: alone it is the register form
        assert pf.k3_form(flows[:1]) == pf.VEC or name in ("n4-fast",), name


def test_k3_form_error_returns():
    one = lambda I, Tz, Tr, kl=1, al=1, members=1: pf.k3_form([(I, Tz, Tr, kl, al)], members)
    assert one(0, 2, 2) == -2 and one(16385, 2, 2) == -2 and one(16384, 2, 2) == pf.GENERIC
    assert one(8, 17, 0) == -2 and one(8, 0, 17) == -2 and one(8, -1, 0) == -2 and one(8, 16, 16) == pf.LDS
    assert one(8, 2, 2, members=0) == -2 and one(8, 2, 2, members=65536) == -2
    # the member dimension exists in the fast and register forms only
    assert one(256, 4, 0, kl=0, members=3) == pf.VEC and one(255, 4, 0, kl=0, members=3) == pf.FAST
    assert one(256, 5, 0, kl=0, members=2) == -2 and one(16384, 2, 0, kl=0, members=2) == -2
    assert pf.k3_form([(8, 2, 2, 1, 1)] * 5) == -2
    from bnn_amd import _lib
    L, v = _lib.lib(), (ctypes.c_int * 1)(8)
    assert L.lbbnn_flow_planar_form(0, v, v, v, v, v, 1) == -2
    assert L.lbbnn_flow_planar_form(1, None, v, v, v, v, 1) == -1 and L.lbbnn_flow_planar_form(1, v, v, v, v, None, 1) == -1


def test_k5_tables_take_the_forms_they_name():
    for form, O, I, mnf in pf.K5_CASES + pf.K5_VARIANT_CASES:
        assert pf.k5_form([(O, I, mnf, 1)]) == form, (O, I, mnf)
    assert sum(1 for c in pf.K5_CASES if c[0] == pf.K5_LDS) >= 3 and sum(1 for c in pf.K5_CASES if c[0] == pf.K5_GENERIC) >= 3
    assert 4 * (6 * 3008 + 2 * 320) > pf.LDS_RAISE                                # O = 3000: the attribute is raised
    # LRT: 6 pad64(O) + 2 * 64 floats against 36864; 6080 is the last O that fits
    assert (pf.k5_form([(6080, 0, 0, 1)]), pf.k5_form([(6081, 0, 0, 1)])) == (pf.K5_LDS, pf.K5_GENERIC)
    assert pf.k5_form([(64, 16384, 1, 1)]) == pf.K5_LDS and pf.k5_form([(700, 16384, 1, 1)]) == pf.K5_GENERIC
    # the per-layer launch goes by its LARGEST layer, the all-layers launch by the SUM over the active ones
    four = [(1600, 300, 1, 1), (1600, 0, 0, 1), (1600, 5, 1, 1), (1600, 64, 1, 1)]
    assert pf.k5_form(four) == pf.K5_LDS and pf.k5_form(four, all_layers=True) == 0
    assert pf.k5_form(four[:3], all_layers=True) == 1
    assert pf.k5_form([four[0], (1600, 0, 0, 0), four[2], four[3]], all_layers=True) == 1         # an inactive layer stages nothing
    staged = unstaged = 0
    for name, (st, layers, draws, adv) in pf.FINALIZE_GROUPS.items():
        assert pf.k5_form([(O, I, mnf, act) for O, I, mnf, act in layers], all_layers=True) == st, name
        staged, unstaged = staged + (st == 1), unstaged + (st == 0)
    assert staged >= 3 and unstaged >= 3
    assert sorted(len(g[1]) for g in pf.FINALIZE_GROUPS.values())[0] == 1 and {len(g[1]) for g in pf.FINALIZE_GROUPS.values()} == {1, 2, 3, 4}
    for name, (form, layers) in pf.PREPARE_GROUPS.items():
        assert pf.k5_form([(O, I, mnf, 1) for I, O, Tz, Tr, kl, mnf in layers if kl]) == pf.K5_LDS, name


def test_k5_form_error_returns():
    assert pf.k5_form([(0, 5, 1, 1)]) == -2 and pf.k5_form([(5, 0, 1, 1)]) == -2 and pf.k5_form([(5, 0, 0, 1)]) == pf.K5_LDS
    assert pf.k5_form([(5, 5, 1, 1)] * 5) == -2
    assert pf.k5_form([(0, 0, 1, 0), (5, 5, 1, 1)], all_layers=True) == 1         # an inactive layer is not read
    assert pf.k5_form([(0, 0, 1, 0), (5, 5, 1, 1)]) == -2                         # the per-layer launch has no inactive layers
    from bnn_amd import _lib
    L, v = _lib.lib(), (ctypes.c_int * 1)(8)
    assert L.lbbnn_kl_finalize_form(0, v, v, v, v, 0) == -2
    assert L.lbbnn_kl_finalize_form(1, None, v, v, v, 0) == -1 and L.lbbnn_kl_finalize_form(1, v, v, v, None, 0) == pf.K5_LDS
    assert L.lbbnn_kl_finalize_form(1, v, v, v, None, 1) == -1
