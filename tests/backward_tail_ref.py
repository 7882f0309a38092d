"""References and case tables for the kernels that finish a training step -- lbbnn_weight_pass_backward (K1b),
lbbnn_output_grad, lbbnn_head_dx, lbbnn_dx_combine, lbbnn_bias_backward[_partials] and the entries of csrc/loss_head.hip --
plain torch on CPU tensors, no GPU.  float64 of the float32 values the kernels see is the truth
(``.float().double()``); ``wpb_objective`` is dtype-generic so that the host tier can run the very same lines in float32
and show how far float32 arithmetic alone is from them.

The tables below are iterated by tests/test_backward_tail_host.py (well-formedness, the conditioning of the wide-range
inputs) and by tests/test_backward_tail_gpu.py (the kernels).  Every shape is the smallest that reaches its branch:

    K1b       8 rows x 64 column groups of 4 (or 1) columns per workgroup: O < 8 leaves row lanes idle, I = 260 is one column
              group past a 256-column workgroup; slabs are added 4 per loop trip after slab 0 (S = 5: one full trip, S = 6: a
              trip and a ragged one, S = 16: the head's own count)
    output    64 x 64 tiles; the second level gives each of 16 waves every 16th row tile: 17 and 33 tiles reach its second
              and third trip, 16 tiles fill the first exactly
    head_dx   16 rows x 256 columns per workgroup; C == 10 with G_v takes the register kernel, everything else the LDS one
    loss      one 1024-thread workgroup forward (B = 1025: second trip); 512 x 256 threads backward (B C = 134400: second
              trip of the grid-stride loop); C = 64 the limit of lbbnn_log_softmax_backward
"""
import math

import torch
import torch.nn.functional as F

from oracle import lbbnn_oracle as orc

TIGHT = 5e-6             # test_parity_gpu.TIGHT: the repository's bar of an fp32 output with a short sum behind it
WPB_BAR = 2e-5           # test_weight_pass_backward_kernel's bar, every output
WPB_F32_BAR = 5e-6       # what the float32 run of the reference itself must stay under on the wide-range inputs
GV_BAR = 1e-6            # test_output_grad_kernel's bar of G_v
LOSS_BAR = 1e-6          # test_fused_elbo_loss_and_log_softmax_backward_vs_torch: loss and its gradients
LSM_BAR = 2e-6           # ... and lbbnn_log_softmax_backward
U32 = 2.0 ** -24         # unit roundoff of float32

WPB_NAMES = ("dmu", "drho", "dlambdal", "dz_fwd", "dz_kl", "dr0_c")


def rel_err(a, b):
    """conftest.rel_err (max-norm), restated so that the module imports without pytest's path set-up."""
    a = torch.as_tensor(a, dtype=torch.float64).cpu()
    b = torch.as_tensor(b, dtype=torch.float64).cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def priors():
    import bnn_amd
    return bnn_amd.Priors()


# --------------------------------------------------------------------------- K1b: lbbnn_weight_pass_backward
# (id, O, I, options).  Options: mnf (z_fwd, z_kl, r0_c given), with_var (dWv given), with_kl (g_kl given), with_act (da_mu /
# da_var given), S (slabs of dWm / dWv; 0: a plain (O, I) gradient), wide (the ranges of trained parameters), unaligned
WPB_SHAPES = [(1, 1), (3, 5), (5, 4), (4, 252), (8, 256), (9, 260), (1, 260)]


def wpb_case(tag, O, I, mnf, **kw):
    opt = dict(mnf=mnf, with_var=True, with_kl=True, with_act=mnf, S=0, wide=False, unaligned=False)
    opt.update(kw)
    return ("%s-%dx%d-%s" % (tag, O, I, "mnf" if mnf else "lrt"), O, I, opt)


WPB_CASES = [wpb_case("shape", O, I, mnf) for (O, I) in WPB_SHAPES for mnf in (True, False)]
for _O, _I in [(9, 260), (3, 5)]:
    WPB_CASES += [
        wpb_case("novar", _O, _I, True, with_var=False),
        wpb_case("nokl", _O, _I, False, with_kl=False),
        wpb_case("novar-nokl", _O, _I, False, with_var=False, with_kl=False),       # drho is identically zero
        wpb_case("act-nokl", _O, _I, True, with_kl=False),
        wpb_case("z-noact", _O, _I, True, with_act=False),
        wpb_case("z-noact-nokl", _O, _I, True, with_act=False, with_kl=False),      # dz_kl, dr0_c: None
    ]
WPB_SLABS = (2, 4, 5, 6, 16)
WPB_SLAB_SHAPES = [(8, 256), (4, 5)]              # the vector kernel; the scalar kernel (O * I % 4 == 0, I % 4 != 0)
WPB_SLAB_CASES = [wpb_case("slabs%d" % S, O, I, True, S=S) for (O, I) in WPB_SLAB_SHAPES for S in WPB_SLABS]
WPB_UNALIGNED_CASES = [wpb_case("unaligned", 8, 256, True, unaligned=True)]
WPB_WIDE_CASES = [wpb_case("wide", O, I, True, wide=True) for (O, I) in [(9, 33), (8, 260)]]
WPB_ALL = WPB_CASES + WPB_SLAB_CASES + WPB_UNALIGNED_CASES + WPB_WIDE_CASES


def wpb_inputs(O, I, opt):
    """float32 CPU inputs of one K1b case; what a case does not hand to the kernel is None."""
    g = torch.Generator().manual_seed(O * 1000 + I + (7 if opt["wide"] else 0))
    r = lambda *s: torch.rand(*s, generator=g)
    n = lambda *s: torch.randn(*s, generator=g)
    if opt["wide"]:
        # test_weight_pass_wide_parameter_ranges' inputs: both softplus branches, alpha from 1e-6 to 1 - 1e-6
        d = dict(mu=3 * (2 * r(O, I) - 1), rho=-14 + 18 * r(O, I), lam=-14 + 28 * r(O, I),
                 zf=1 + 0.3 * n(I), zk=1 + 0.3 * n(I), rc=n(I))
    else:
        # test_weight_pass_backward_kernel's inputs
        d = dict(mu=(r(O, I) - 0.5) * 0.4, rho=-5 + r(O, I) * 3, lam=n(O, I) * 2,
                 zf=1 + 0.1 * n(I), zk=1 + 0.1 * n(I), rc=0.1 * n(I))
    shape = (opt["S"], O, I) if opt["S"] else (O, I)
    d.update(dWm=n(*shape), dWv=n(*shape), dam=n(O), dav=n(O), gk=torch.tensor(1 / 600.))
    if not opt["mnf"]:
        d.update(zf=None, zk=None, rc=None)
    if not opt["with_act"]:
        d.update(dam=None, dav=None)
    if not opt["with_var"]:
        d["dWv"] = None
    if not opt["with_kl"]:
        d["gk"] = None
    return d


def wpb_objective(mu, rho, lam, zf, zk, rc, dWm, dWv, dam, dav, gk, pr, *, mnf, with_var=True, with_kl=True, with_act=None):
    """The scalar whose gradient K1b writes (test_weight_pass_backward_kernel's objective) in the dtype of ``mu``:

        <dWm, mu alpha z_fwd> + <dWv, sigma^2 alpha^2> + g_kl KL_w(mu z_kl, sigma, alpha)
                              + <da_mu, r0_c (z_kl mu alpha)^T> + <da_var, r0_c^2 (sigma^2 alpha^2)^T>

    in stable forms: sigma = softplus(rho), log alpha = logsigmoid(lambda), log(1 - alpha) = logsigmoid(-lambda),
    1 - alpha = sigmoid(-lambda).  Slabs of dWm / dWv are summed in float64 first."""
    dt = mu.dtype
    with_act = mnf if with_act is None else with_act
    cast = lambda t: (t.double().sum(0) if t.dim() == 3 else t.double()).to(dt)
    alpha, one_m_alpha = torch.sigmoid(lam), torch.sigmoid(-lam)
    log_alpha, log_1m_alpha = F.logsigmoid(lam), F.logsigmoid(-lam)
    sigma = F.softplus(rho)
    Wv = sigma ** 2 * alpha ** 2
    e_w = mu * alpha * zf if mnf else mu * alpha
    obj = (cast(dWm) * e_w).sum()
    if with_var:
        obj = obj + (cast(dWv) * Wv).sum()
    if with_kl:
        mu_eff = mu * zk if mnf else mu
        klw = (alpha * (math.log(pr.sigma_prior) - sigma.log() - 0.5 + (log_alpha - math.log(pr.alpha_prior))
                        + (sigma ** 2 + (mu_eff - pr.mu_prior) ** 2) / (2 * pr.sigma_prior ** 2))
               + one_m_alpha * (log_1m_alpha - math.log(1 - pr.alpha_prior))).sum()
        obj = obj + gk.to(dt) * klw
    if with_act:
        obj = obj + (dam.to(dt) * (rc @ (zk * mu * alpha).T)).sum() + (dav.to(dt) * (rc ** 2 @ Wv.T)).sum()
    return obj


def wpb_reference(d, opt, pr, dtype=torch.float64):
    """{name: gradient} of wpb_objective by autograd in ``dtype``, on the float32 values of ``d``; a leaf the objective does
    not depend on gets zeros, a leaf the case does not have None."""
    ones = lambda: torch.ones(d["mu"].shape[1])
    leaves = [d["mu"], d["rho"], d["lam"]] + [d[k] if d[k] is not None else ones() for k in ("zf", "zk", "rc")]
    leaves = [t.float().to(dtype).requires_grad_(True) for t in leaves]
    obj = wpb_objective(*leaves, d["dWm"], d["dWv"], d["dam"], d["dav"], d["gk"], pr, mnf=opt["mnf"],
                        with_var=opt["with_var"], with_kl=opt["with_kl"], with_act=opt["with_act"])
    grads = torch.autograd.grad(obj, leaves, allow_unused=True)
    out = {}
    for name, leaf, g, key in zip(WPB_NAMES, leaves, grads, ("mu", "rho", "lam", "zf", "zk", "rc")):
        out[name] = None if d[key] is None else (g if g is not None else torch.zeros_like(leaf))
    return out


# --------------------------------------------------------------------------- lbbnn_output_grad and the column sums
OG_TILE = 64
OG_SUM_SHAPES = [(1025, 1), (1025, 65), (2112, 65), (64 * 16, 64)]            # 17, 17, 33 and 16 row tiles
OG_OPTION_SHAPES = [(5, 3), (70, 6), (65, 64)]
OG_STRIDED_OFFSETS = (1, 4)          # buf[:, off:off + O] of a (B, O + 8) buffer: 4-byte / 16-byte aligned base, ld = O + 8
OG_PAD = 8
OG_PHILOX = (70, 6, 1000)            # (B, O, row_offset): two row tiles, the last Philox group of four is partial


def og_row_tiles(B):
    return (B + OG_TILE - 1) // OG_TILE


def og_sum_depth(B):
    """The longest chain of additions behind one column sum: 64 rows of a tile, then a wave's share of the tiles, then the 16
    waves' partials."""
    return OG_TILE + (og_row_tiles(B) + 15) // 16 + 16


def og_inputs(B, O, seed=0):
    g = torch.Generator().manual_seed(B * 31 + O + seed)
    return dict(g_out=torch.randn(B, O, generator=g), out=torch.randn(B, O, generator=g),
                std=0.1 + torch.rand(B, O, generator=g), eps=torch.randn(B, O, generator=g),
                gv_scale=0.5 + torch.rand(O, generator=g))


def output_grad_ref(g_out, out=None, std=None, eps=None, gv_scale=None):
    """float64: gm = where(out > 0, g, 0) (or g without ReLU), gv = gm eps / (2 std) [gv_scale], the transposes, the column
    sums and the column sums of the magnitudes (the scale of the sums' error bound).  gv* are None without ``std``."""
    g = g_out.float().double()
    gm = torch.where(out.float().double() > 0, g, torch.zeros_like(g)) if out is not None else g
    r = dict(gm=gm, gmT=gm.t().contiguous(), g_sum=gm.sum(0), g_abs=gm.abs().sum(0), gv=None, gvT=None, gv_sum=None, gv_abs=None)
    if std is not None:
        gv = gm * eps.float().double() / (2 * std.float().double())
        if gv_scale is not None:
            gv = gv * gv_scale.float().double()
        r.update(gv=gv, gvT=gv.t().contiguous(), gv_sum=gv.sum(0), gv_abs=gv.abs().sum(0))
    return r


def column_sum_bound(terms, B):
    """Per column: depth * 2^-24 * Sum_b |term| for the float32 terms the kernels add."""
    return og_sum_depth(B) * U32 * terms.double().abs().sum(0)


def bias_ref(bias_mu, bias_rho, g_sum, gv_sum, g_kl, pr):
    """float64 autograd of  Sum_o g_sum[o] bias_mu[o] + Sum_o gv_sum[o] softplus(bias_rho[o])^2 + g_kl KL_bias  (the bias adds
    to the activation mean, softplus(bias_rho)^2 to its variance; KL_bias is the oracle's).  -> (d_bias_mu, d_bias_rho)"""
    m = bias_mu.float().double().requires_grad_(True)
    r = bias_rho.float().double().requires_grad_(True)
    obj = (g_sum.double() * m).sum() + 0.0 * r.sum()
    if gv_sum is not None:
        obj = obj + (gv_sum.double() * F.softplus(r) ** 2).sum()
    if g_kl is not None:
        obj = obj + g_kl.float().double() * orc.kl_bias_term(m, r, pr)
    return torch.autograd.grad(obj, [m, r])


# --------------------------------------------------------------------------- lbbnn_head_dx, lbbnn_dx_combine
HEAD_DX_CLASSES = (1, 3, 10, 16)
HEAD_DX_SHAPES = [(1, 1), (15, 255), (16, 256), (17, 257), (33, 513)]          # around 16 rows x 256 columns
HEAD_DX_LAYOUTS = ("dense", "strided")
HEAD_DX_CASES = [(C, stoch, B, I, lay) for C in HEAD_DX_CLASSES for stoch in (True, False) for (B, I) in HEAD_DX_SHAPES
                 for lay in HEAD_DX_LAYOUTS]
HEAD_DX_G_LD, HEAD_DX_G_OFF, HEAD_DX_X_OFF, HEAD_DX_X_PAD = 24, 3, 2, 5
HEAD_DX_PAD_OUT = 3                  # the ctypes calls write into rows of I + 3 floats

DX_COMBINE_SHAPES = [(1, 1), (3, 1023), (2, 1025)]                              # around the 1024 columns of one workgroup


def head_dx_inputs(C, B, I):
    g = torch.Generator().manual_seed(C * 100003 + B * 1009 + I)
    return dict(gm=torch.randn(B, C, generator=g), gv=torch.randn(B, C, generator=g), wmT=torch.randn(I, C, generator=g),
                wvT=torch.rand(I, C, generator=g), x=torch.randn(B, I, generator=g))


def head_dx_ref(gm, gv, wmT, wvT, x, C):
    """float64 dX = gm Wm^T[:, :C]^T + 2 x (gv Wv^T[:, :C]^T); without gv the first term alone."""
    dx = gm.float().double() @ wmT[:, :C].float().double().T
    if gv is not None:
        dx = dx + 2 * x.float().double() * (gv.float().double() @ wvT[:, :C].float().double().T)
    return dx


# --------------------------------------------------------------------------- csrc/loss_head.hip
LOSS_SHAPES = [(1, 1), (1023, 2), (1025, 17), (2100, 64)]
LOSS_PAD, LOSS_OFF = 7, 1            # strided: buf[:, 1:1 + C] of a (B, C + 7) buffer
LSM_CLASSES = (1, 64)
LOSS_KL, LOSS_BATCHES = 1234.5, 600


def loss_inputs(B, C, bad_targets):
    """logits, float32 log-probabilities, int64 targets (bad_targets: ~10 % are -100, ~5 % are C) and an upstream gradient."""
    g = torch.Generator().manual_seed(B * 67 + C + (1 if bad_targets else 0))
    logits = torch.randn(B, C, generator=g)
    target = torch.randint(0, C, (B,), generator=g)
    if bad_targets:
        u = torch.rand(B, generator=g)
        target = torch.where(u < 0.10, torch.full_like(target, -100), target)
        target = torch.where((u >= 0.10) & (u < 0.15), torch.full_like(target, C), target)
        if B == 1:
            target = torch.full_like(target, -100)
    return dict(logits=logits, logp=torch.log_softmax(logits, dim=1), target=target, g=torch.tensor(0.75),
                gout=torch.randn(B, C, generator=g))


def loss_ref(logp, target, kl=None, kl_scale=1.0, g=1.0):
    """float64: loss = -Sum_{valid b} logp[b, t_b] + kl kl_scale; g_logp = -g one-hot on the valid rows (zero rows elsewhere);
    g_logits = g_logp - exp(logp) rowsum(g_logp); g_kl = g kl_scale.  A row is valid when 0 <= t_b < C."""
    lp = logp.float().double()
    B, C = lp.shape
    valid = (target >= 0) & (target < C)
    idx = torch.nonzero(valid).flatten()
    loss = -lp[idx, target[idx]].sum()
    if kl is not None:
        loss = loss + float(kl) * kl_scale
    g_logp = torch.zeros_like(lp)
    g_logp[idx, target[idx]] = -float(g)
    g_logits = lsm_backward_ref(g_logp, lp)
    return dict(loss=loss, g_logp=g_logp, g_logits=g_logits, g_kl=float(g) * kl_scale, valid=valid)


def lsm_backward_ref(g, logp):
    g, lp = g.float().double(), logp.float().double()
    return g - lp.exp() * g.sum(1, keepdim=True)
