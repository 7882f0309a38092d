"""CPU tier of the backward-tail tests (tests/backward_tail_ref.py, tests/test_backward_tail_gpu.py): the case tables are
well-formed and reach the branches they are there for, the references agree with torch's own operators where torch has one,
and the float32 run of the K1b reference on the wide-range inputs stays a decade under the bar the kernel is held to.  No GPU
is touched.

Figures when this was written (printed on every run): float32 against float64 autograd of wpb_objective on the wide-range
inputs at most 2.7e-7 (dlambdal at (8, 260)); bar of that comparison 5e-6, bar of the kernel 2e-5."""
import math

import pytest
import torch
import torch.nn.functional as F

import backward_tail_ref as bt
from oracle import lbbnn_oracle as orc


# --------------------------------------------------------------------------- the tables
def test_wpb_tables_are_well_formed():
    ids = [c[0] for c in bt.WPB_ALL]
    assert len(set(ids)) == len(ids)
    for cid, O, I, opt in bt.WPB_ALL:
        assert O >= 1 and I >= 1
        assert not (opt["with_act"] and not opt["mnf"]), cid           # da_mu needs z_kl and r0_c (LBBNN_E_NULL otherwise)
        if opt["S"]:
            assert (O * I) % 4 == 0, cid                                # the slab stride: LBBNN_E_ALIGN otherwise
        d = bt.wpb_inputs(O, I, opt)
        assert (d["dWv"] is None) == (not opt["with_var"]) and (d["gk"] is None) == (not opt["with_kl"])
        assert (d["dam"] is None) == (not opt["with_act"]) and (d["zf"] is None) == (not opt["mnf"])
        assert d["dWm"].shape == ((opt["S"], O, I) if opt["S"] else (O, I))
    shapes = {(O, I) for _, O, I, opt in bt.WPB_CASES}
    assert any(O < 4 for O, I in shapes) and any(4 < O < 8 for O, I in shapes) and any(O > 8 for O, I in shapes)
    assert any(I % 4 == 0 and 256 < I <= 260 for O, I in shapes)        # one column group past a 256-column workgroup
    assert any(I % 4 == 0 and I < 256 for O, I in shapes) and any(I % 4 for O, I in shapes)
    # slabs: 4 per loop trip after slab 0 -- a full trip, a trip and a ragged one, and both kernels
    assert {5, 6} <= set(bt.WPB_SLABS)
    assert any(I % 4 == 0 for O, I in bt.WPB_SLAB_SHAPES) and any(I % 4 for O, I in bt.WPB_SLAB_SHAPES)
    assert all(I % 4 == 0 for _, O, I, opt in bt.WPB_UNALIGNED_CASES)   # only then is the alignment what picks the kernel
    assert any(I % 4 == 0 for _, O, I, _o in bt.WPB_WIDE_CASES) and any(I % 4 for _, O, I, _o in bt.WPB_WIDE_CASES)


def test_output_grad_tables_are_well_formed():
    tiles = [bt.og_row_tiles(B) for B, O in bt.OG_SUM_SHAPES]
    assert tiles == [17, 17, 33, 16]                                    # second trip, third trip, exactly one trip
    assert any(O > 64 for B, O in bt.OG_SUM_SHAPES) and any(O == 1 for B, O in bt.OG_SUM_SHAPES)
    assert bt.og_sum_depth(2112) == 64 + 3 + 16 and bt.og_sum_depth(1024) == 64 + 1 + 16
    # the strided views: a base that is only 4-byte aligned with O % 4 == 0, and an aligned base with ld != O
    assert (65, 64) in bt.OG_OPTION_SHAPES and bt.OG_STRIDED_OFFSETS == (1, 4) and (64 + bt.OG_PAD) % 4 == 0
    assert all(off + O <= O + bt.OG_PAD for B, O in bt.OG_OPTION_SHAPES for off in bt.OG_STRIDED_OFFSETS)
    B, O, row_offset = bt.OG_PHILOX
    assert bt.og_row_tiles(B) == 2 and O % 4 != 0 and (B, O) in bt.OG_OPTION_SHAPES


def test_head_dx_and_loss_tables_are_well_formed():
    assert len(bt.HEAD_DX_CASES) == len(set(bt.HEAD_DX_CASES)) == 4 * 2 * 5 * 2
    assert 10 in bt.HEAD_DX_CLASSES and max(bt.HEAD_DX_CLASSES) == 16 and min(bt.HEAD_DX_CLASSES) == 1
    assert bt.HEAD_DX_G_OFF + max(bt.HEAD_DX_CLASSES) <= bt.HEAD_DX_G_LD and bt.HEAD_DX_G_OFF % 4 != 0
    assert bt.HEAD_DX_X_OFF <= bt.HEAD_DX_X_PAD
    assert {B for B, I in bt.HEAD_DX_SHAPES} >= {15, 16, 17} and {I for B, I in bt.HEAD_DX_SHAPES} >= {255, 256, 257}
    assert {I for B, I in bt.DX_COMBINE_SHAPES} >= {1023, 1025}
    assert any(B * C > 512 * 256 for B, C in bt.LOSS_SHAPES) and any(1024 < B < 1100 for B, C in bt.LOSS_SHAPES)
    assert max(C for B, C in bt.LOSS_SHAPES) == 64 and set(bt.LSM_CLASSES) == {1, 64}
    for B, C in bt.LOSS_SHAPES:
        t = bt.loss_inputs(B, C, True)["target"]
        bad = (t < 0) | (t >= C)
        assert bad.any() and (B < 100 or ((t < 0).any() and (t >= C).any() and (~bad).sum() > B // 2))
        t = bt.loss_inputs(B, C, False)["target"]
        assert ((t >= 0) & (t < C)).all()


# --------------------------------------------------------------------------- the references against torch's own operators
@pytest.mark.parametrize("O,I,mnf", [(3, 5, True), (9, 33, True), (5, 4, False)])
def test_wpb_objective_is_the_existing_tests_objective(O, I, mnf):
    """The stable forms change no value: float64 gradients equal those of test_weight_pass_backward_kernel's spelling."""
    opt = bt.wpb_case("x", O, I, mnf)[3]
    d = bt.wpb_inputs(O, I, opt)
    pr = bt.priors()
    ref = bt.wpb_reference(d, opt, pr)
    ones = torch.ones(I)
    leaves = [(d[k] if d[k] is not None else ones).double().requires_grad_(True) for k in ("mu", "rho", "lam", "zf", "zk", "rc")]
    m, r, l, f, k, c = leaves
    alpha, sigma = torch.sigmoid(l), torch.log1p(torch.exp(r))
    k_eff = k if mnf else torch.ones_like(k)
    Wv = sigma ** 2 * alpha ** 2
    klw = (alpha * (math.log(pr.sigma_prior) - sigma.log() - 0.5 + (alpha / pr.alpha_prior).log()
                    + (sigma ** 2 + (m * k_eff - pr.mu_prior) ** 2) / (2 * pr.sigma_prior ** 2))
           + (1 - alpha) * ((1 - alpha) / (1 - pr.alpha_prior)).log()).sum()
    obj = (d["dWm"].double() * (m * alpha * (f if mnf else 1))).sum() + (d["dWv"].double() * Wv).sum() + d["gk"].double() * klw
    if mnf:
        obj = obj + (d["dam"].double() * (c @ (k * m * alpha).T)).sum() + (d["dav"].double() * (c ** 2 @ Wv.T)).sum()
    old = torch.autograd.grad(obj, leaves, allow_unused=True)
    for name, g in zip(bt.WPB_NAMES, old):
        if ref[name] is None:
            assert not mnf
            continue
        assert bt.rel_err(ref[name], g) < 1e-12, name


def test_wpb_objective_sums_slabs_in_float64():
    cid, O, I, opt = bt.WPB_SLAB_CASES[2]
    d = bt.wpb_inputs(O, I, opt)
    one = dict(d, dWm=d["dWm"].double().sum(0), dWv=d["dWv"].double().sum(0))
    pr = bt.priors()
    a, b = bt.wpb_reference(d, opt, pr), bt.wpb_reference(one, dict(opt, S=0), pr)
    for name in bt.WPB_NAMES:
        assert bt.rel_err(a[name], b[name]) < 1e-13, name


@pytest.mark.parametrize("case", bt.WPB_WIDE_CASES, ids=[c[0] for c in bt.WPB_WIDE_CASES])
def test_wide_range_reference_in_float32_is_a_decade_under_the_kernel_bar(case):
    """The evidence behind holding the kernel to 2e-5 over the ranges trained parameters reach: the same lines in float32 are
    within 5e-6 (max-norm) of float64 for every output, and every output is finite."""
    cid, O, I, opt = case
    d = bt.wpb_inputs(O, I, opt)
    assert float(d["rho"].min()) < -12 and float(d["rho"].max()) > 2 and float(d["lam"].min()) < -12 and float(d["lam"].max()) > 12
    pr = bt.priors()
    r64, r32 = bt.wpb_reference(d, opt, pr, torch.float64), bt.wpb_reference(d, opt, pr, torch.float32)
    for name in bt.WPB_NAMES:
        assert torch.isfinite(r64[name]).all() and torch.isfinite(r32[name]).all(), name
        assert float(r64[name].abs().max()) > 0
        e = bt.rel_err(r32[name], r64[name])
        print("%s %s: float32 reference %.2e off float64" % (cid, name, e))
        assert e <= bt.WPB_F32_BAR, (name, e)
    assert bt.WPB_BAR >= 4 * bt.WPB_F32_BAR


@pytest.mark.parametrize("B,C", bt.LOSS_SHAPES)
@pytest.mark.parametrize("bad", [False, True])
def test_loss_ref_is_nll_loss_with_ignored_rows(B, C, bad):
    """loss_ref == F.nll_loss(reduction='sum') + autograd on the rows whose target is in range (the others contribute nothing
    and get a zero gradient row: torch's ignore_index, for every out-of-range value)."""
    d = bt.loss_inputs(B, C, bad)
    scale = 1.0 / bt.LOSS_BATCHES
    r = bt.loss_ref(d["logp"], d["target"], bt.LOSS_KL, scale, d["g"])
    valid = r["valid"]
    assert valid.all() == (not bad)
    t = torch.where(valid, d["target"], torch.full_like(d["target"], -100))
    logits = d["logits"].double().requires_grad_(True)
    lp = torch.log_softmax(logits, dim=1)
    lp.retain_grad()
    kl = torch.tensor(bt.LOSS_KL, dtype=torch.float64, requires_grad=True)
    loss = F.nll_loss(lp, t, reduction="sum", ignore_index=-100) + kl * scale
    (loss * d["g"].double()).backward()
    # the reference reads the float32 log-probabilities, torch's run here the float64 ones of the same logits
    assert abs(float(r["loss"]) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach())) + 1e-12
    assert torch.equal(r["g_logp"], lp.grad) and abs(r["g_kl"] - float(kl.grad)) < 1e-15
    assert bt.rel_err(r["g_logits"], logits.grad) < 1e-6 or float(logits.grad.abs().max()) == 0
    assert (r["g_logp"][~valid] == 0).all() and (r["g_logits"][~valid] == 0).all()


def test_bias_ref_and_output_grad_ref_formulas():
    pr = bt.priors()
    g = torch.Generator().manual_seed(2)
    mu, rho = torch.randn(7, generator=g), -3 + torch.randn(7, generator=g)
    gs, gvs, gk = torch.randn(7, generator=g).double(), torch.randn(7, generator=g).double(), torch.tensor(0.37)
    d_mu, d_rho = bt.bias_ref(mu, rho, gs, gvs, gk, pr)
    sb = F.softplus(rho.double())
    inv = 1.0 / pr.bias_sigma_prior ** 2
    assert bt.rel_err(d_mu, gs + 0.37 * (mu.double() - pr.bias_mu_prior) * inv) < 1e-7
    assert bt.rel_err(d_rho, (gvs * 2 * sb + float(gk) * (sb * inv - 1 / sb)) * torch.sigmoid(rho.double())) < 1e-7
    z_mu, z_rho = bt.bias_ref(mu, rho, gs, None, None, pr)
    assert torch.equal(z_mu, gs) and float(z_rho.abs().max()) == 0
    assert float(orc.kl_bias_term(mu.double(), rho.double(), orc.Priors())) == float(orc.kl_bias_term(mu.double(), rho.double(), pr))
    d = bt.og_inputs(5, 3)
    d["out"][0, 0], d["out"][1, 1], d["out"][2, 2], d["out"][3, 0] = 0.0, -0.0, float("nan"), 1.4e-45
    r = bt.output_grad_ref(d["g_out"], d["out"], d["std"], d["eps"], d["gv_scale"])
    assert r["gm"][0, 0] == 0 and r["gm"][1, 1] == 0 and r["gm"][2, 2] == 0 and r["gm"][3, 0] == d["g_out"][3, 0].double()
    assert torch.isfinite(r["gv"]).all() and torch.equal(r["gvT"], r["gv"].t())
    assert bt.rel_err(r["gv_sum"], (r["gm"] * d["eps"].double() / (2 * d["std"].double()) * d["gv_scale"].double()).sum(0)) < 1e-15
