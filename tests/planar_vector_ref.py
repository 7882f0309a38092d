"""Reference for the vector-sized backward of a planar MNF layer (csrc/vector_bwd.hip) -- plain torch, no GPU.

V2 (lbbnn_mnf_flow_planar_backward[_batch]) returns the gradient of a scalar objective F wrt every vector-sized leaf;
V1 (lbbnn_mnf_aux_backward[_batch]) that of F1 wrt the auxiliary activations' moments.  Both objectives are written out
below from the oracle's own pieces (``oracle.planar_step_1d``, ``oracle.kl_bias_term``) and differentiated by autograd, in
float64 for the truth and in float32 for the yardstick E32: what plain fp32 arithmetic of the very same formula loses.

    sd  = exp(0.5 q0_log_var)
    zF  = zflow(q0_mean + sd eps_fwd)            zK, ldq = zflow(q0_mean + sd eps_kl)            zb, ldr = rflow(zK)
    log_rb = Sum_i( -0.5 b2_i m - 0.5 (zb[-1] - b1_i m)^2 exp(-b2_i m) )                          (m = aux[0], a constant)
    F  = <dz_fwd, zF> + <g_sum, bias_mu> + <gv_sum, softplus(bias_rho)^2>
         + [has_kl] ( <dz_kl, zK> + G ( kl_bias_term(bias_mu, bias_rho) - ldq - 0.5 Sum q0_log_var - ldr - log_rb ) )

    m  = mean_o tanh(act_mu + sqrt(act_var) eps_act)            F1 = -G log_rb(m)               (zb, G constants)

The kernel picks one of three bodies for V2 by shape alone (``form``), and reaches the two chain bodies through two
different kernels; CASES holds the smallest shapes at every edge of that choice."""
import functools
import math

import torch

from oracle import lbbnn_oracle as orc

NT = 1024                      # threads of the single workgroup; thread tid owns elements tid, tid + 1024, ...
REG_MAX_I = 2 * NT             # register form: at most two elements per thread ...
REG_MAX_T = 4                  # ... and at most four transforms per flow (also the batch kernel's limit)
LDS_LIMIT = 144 * 1024         # chain workspace in LDS up to here, in a.work beyond
LDS_RAISE = 64 * 1024          # above this the dynamic-LDS attribute of the kernel is raised first
M_AUX, G_KL = 0.37, 1.0 / 60.0

# (I, O, Tz, Tr, route); route: 'single' = lbbnn_mnf_flow_planar_backward, 'batch' = deferred, then flushed in a group
CASES = {
    "reg": [(1, 1, 1, 1, "single"), (5, 7, 3, 3, "single"), (63, 1, 0, 2, "single"), (64, 3, 2, 0, "single"),
            (40, 3, 0, 0, "single"), (1023, 1024, 4, 4, "single"), (1024, 1025, 4, 1, "single"),
            (1025, 1200, 1, 4, "single"), (2047, 5, 2, 2, "single"), (2048, 5, 4, 4, "single")],
    "lds": [(1, 1, 5, 5, "single"), (100, 3, 5, 2, "single"), (257, 3, 16, 16, "single"), (1025, 3, 5, 1, "single"),
            (2049, 3, 1, 1, "batch"), (4096, 3, 1, 1, "batch")],
    "global": [(4097, 3, 1, 1, "batch"), (2049, 3, 4, 4, "batch"), (2500, 3, 16, 16, "single")],
}
ALL_CASES = [(f,) + c for f in ("reg", "lds", "global") for c in CASES[f]]
V1_CASES = [(1, 1), (7, 5), (1024, 1025), (1025, 2049), (1200, 784)]          # (O, I)

VEC_BAR = 5e-5                 # max-norm bar of a vector leaf (the bar of test_planar_backward_all_hip_vs_oracle_autograd)
ELEM_RTOL = 1e-4               # element-wise: |got - ref| <= ELEM_RTOL |ref| + A_ELEM max|ref|
A_ELEM = 1.1e-5                # three times the worst remainder of the float32 reference over the table (measured 3.6e-6): the
#                                margin is for the hardware exp / rcp of tanh_fast; may not exceed 5e-5
SCALAR_FLOOR = 5e-5            # a one-element leaf: max(SCALAR_FLOOR, 4 E32) of that leaf on those inputs ...
SCALAR_CEIL = 1e-3             # ... which no leaf may push above this, and at most SCALAR_WIDE_FRAC of them above the floor
SCALAR_WIDE_FRAC = 0.01


def workspace_floats(I, Tz, Tr):
    """lbbnn_mnf_flow_backward_workspace, from the library itself."""
    from bnn_amd import _lib
    return int(_lib.lib().lbbnn_mnf_flow_backward_workspace(I, Tz, Tr))


def form(I, Tz, Tr, workspace=workspace_floats):
    """'reg' | 'lds' | 'global': the body lbbnn_mnf_flow_planar_backward[_batch] runs at this shape."""
    if I <= REG_MAX_I and Tz <= REG_MAX_T and Tr <= REG_MAX_T:
        return "reg"
    return "lds" if 4 * workspace(I, Tz, Tr) <= LDS_LIMIT else "global"


def leaf_names(Tz, Tr):
    names = ["q0_mean", "q0_log_var", "r0_b1", "r0_b2", "bias_mu", "bias_rho"]
    for fl, T in (("z_flow", Tz), ("r_flow", Tr)):
        for t in range(T):
            names += ["%s.%d.%s" % (fl, t, k) for k in ("u", "w", "b")]
    return names


def draw_inputs(I, O, Tz, Tr, gen_seed):
    """One draw of the inputs of a V2 call, float32 on the CPU: the leaves (leaf_names) and the constants."""
    g = torch.Generator().manual_seed(gen_seed)
    n = lambda k: torch.randn(k, generator=g)
    d = {"q0_mean": 1 + 0.3 * n(I), "q0_log_var": -2 + 0.3 * n(I), "r0_b1": 0.5 * n(I), "r0_b2": 0.5 * n(I),
         "bias_mu": 0.1 * n(O), "bias_rho": -3 + n(O)}
    for fl, T in (("z_flow", Tz), ("r_flow", Tr)):
        for t in range(T):
            d["%s.%d.u" % (fl, t)] = n(I) / math.sqrt(I)
            d["%s.%d.w" % (fl, t)] = n(I) / math.sqrt(I)
            d["%s.%d.b" % (fl, t)] = 0.3 * n(1)
    for k in ("dz_fwd", "dz_kl", "eps_fwd", "eps_kl"):
        d[k] = n(I)
    d["g_sum"], d["gv_sum"] = n(O), n(O)
    d["aux"] = torch.tensor([M_AUX, 0.0, 0.0, 0.0])
    d["g_kl"] = torch.tensor([G_KL])
    return d


# The argument variants every draw is rehearsed in: (has_kl, which optional cotangents are handed in)
FULL = (("dz_fwd", True), ("dz_kl", True), ("gv_sum", True))
VARIANTS = [FULL] + [tuple((k, k != off) for k, _ in FULL) for off in ("dz_fwd", "dz_kl", "gv_sum")]
CONFIGS = [(True, v) for v in VARIANTS] + [(False, v) for v in VARIANTS if dict(v)["dz_kl"]]

# A gradient of a flow bias is a sum over I products that cancels (|sum| ~ 1 out of ~ sqrt(I) of absolute mass), and the w
# gradient of the same transform is that scalar times z.  Now and then a draw cancels so far that plain float32 arithmetic
# of F itself is off by 1e-4 or more on a whole vector (seen: 8.7e-5 at (1025, 1200, 1, 4), 5.1e-4 elsewhere): such a draw
# measures the inputs, not the kernel, like a u / w scale at which tanh saturates.  So a draw is kept only if the float32
# reference holds, in every argument variant, the yardstick the bars were derived from; otherwise the next one is taken
# (generator seed + 1000, + 2000, ...).  The rule looks at the reference alone, never at a kernel.
E32_VEC = 1.6e-5               # max-norm of a vector leaf, float32 reference against float64
E32_REM = 5.5e-6               # its element-wise remainder beyond ELEM_RTOL |ref|, as a fraction of max|ref|
MAX_REDRAWS = 64


def e32_of(d, Tz, Tr, has_kl, variant=FULL):
    """(worst vector max-norm, worst remainder, [E32 of every one-element leaf]) of the float32 reference on d."""
    r64, r32 = v2_reference(d, Tz, Tr, has_kl, **dict(variant)), v2_reference(d, Tz, Tr, has_kl, torch.float32, **dict(variant))
    vec = rem = 0.0
    scal = []
    for k, ref in r64.items():
        if float(ref.abs().max()) == 0.0:
            continue
        if ref.numel() == 1:
            scal.append(max_norm_err(r32[k], ref))
        else:
            vec, rem = max(vec, max_norm_err(r32[k], ref)), max(rem, elem_remainder(r32[k], ref))
    return vec, rem, scal


def well_conditioned(d, Tz, Tr):
    for has_kl, variant in CONFIGS:
        vec, rem, scal = e32_of(d, Tz, Tr, has_kl, variant)
        if vec > E32_VEC or rem > E32_REM or any(4.0 * e > SCALAR_CEIL for e in scal):
            return False
    return True


@functools.lru_cache(maxsize=None)
def _kept_draw(I, O, Tz, Tr, seed):
    for redraw in range(MAX_REDRAWS):
        d = draw_inputs(I, O, Tz, Tr, seed + 1000 * redraw)
        if well_conditioned(d, Tz, Tr):
            return d, redraw
    raise RuntimeError("no well-conditioned draw at %r" % ((I, O, Tz, Tr, seed),))


def make_inputs(I, O, Tz, Tr, seed):
    """The inputs of one V2 call at this seed (shared: do not write to them)."""
    return _kept_draw(I, O, Tz, Tr, seed)[0]


def redraws(I, O, Tz, Tr, seed):
    return _kept_draw(I, O, Tz, Tr, seed)[1]


@functools.lru_cache(maxsize=None)
def references(I, O, Tz, Tr, seed, has_kl, variant=FULL):
    """(float64 reference, float32 reference) of make_inputs(I, O, Tz, Tr, seed): computed once, shared, left unchanged."""
    d = make_inputs(I, O, Tz, Tr, seed)
    return (v2_reference(d, Tz, Tr, has_kl, **dict(variant)),
            v2_reference(d, Tz, Tr, has_kl, torch.float32, **dict(variant)))


def _flow(z, d, fl, T):
    ld = z.new_zeros(())
    for t in range(T):
        z, l = orc.planar_step_1d(z, d["%s.%d.u" % (fl, t)], d["%s.%d.w" % (fl, t)], d["%s.%d.b" % (fl, t)])
        ld = ld + l.sum()
    return z, ld


def _log_rb(zb_last, b1, b2, m):
    return (-0.5 * b2 * m - 0.5 * (zb_last - b1 * m) ** 2 * torch.exp(-b2 * m)).sum()


def v2_objective(d, Tz, Tr, has_kl, dz_fwd=True, dz_kl=True, gv_sum=True):
    sd = torch.exp(0.5 * d["q0_log_var"])
    zF, _ = _flow(d["q0_mean"] + sd * d["eps_fwd"], d, "z_flow", Tz)
    F = torch.dot(d["g_sum"], d["bias_mu"])
    if dz_fwd:
        F = F + torch.dot(d["dz_fwd"], zF)
    if gv_sum:
        F = F + torch.dot(d["gv_sum"], orc.sigma_of(d["bias_rho"]) ** 2)
    if has_kl:
        m, G = d["aux"][0], d["g_kl"][0]
        zK, ldq = _flow(d["q0_mean"] + sd * d["eps_kl"], d, "z_flow", Tz)
        zb, ldr = _flow(zK, d, "r_flow", Tr)
        if dz_kl:
            F = F + torch.dot(d["dz_kl"], zK)
        F = F + G * (orc.kl_bias_term(d["bias_mu"], d["bias_rho"], orc.Priors()) - ldq - 0.5 * d["q0_log_var"].sum()
                     - ldr - _log_rb(zb[-1], d["r0_b1"], d["r0_b2"], m))
    return F


def v2_reference(d, Tz, Tr, has_kl, dtype=torch.float64, **variant):
    """{leaf: dF/dleaf} by autograd in ``dtype``; a leaf F does not depend on gets exact zeros."""
    names = leaf_names(Tz, Tr)
    c = {k: v.detach().to(dtype).clone() for k, v in d.items()}
    for k in names:
        c[k].requires_grad_(True)
    grads = torch.autograd.grad(v2_objective(c, Tz, Tr, has_kl, **variant), [c[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(c[k]) if g is None else g).detach() for k, g in zip(names, grads)}


def draw_v1_inputs(O, I, gen_seed):
    g = torch.Generator().manual_seed(gen_seed)
    n = lambda k: torch.randn(k, generator=g)
    return {"act_mu": 0.5 * n(O), "act_var": torch.exp(-2 + 0.3 * n(O)), "eps_act": n(O), "r0_b1": 0.5 * n(I),
            "r0_b2": 0.5 * n(I), "zb_last": 1 + 0.3 * n(1), "g_kl": torch.tensor([G_KL])}


def v1_e32_of(d):
    """(worst vector max-norm, worst remainder, worst one-element E32) of the float32 reference of V1 on d."""
    r64, r32 = v1_reference(d), v1_reference(d, torch.float32)
    vec = rem = scal = 0.0
    for k, ref in r64.items():
        if ref.numel() == 1:
            scal = max(scal, max_norm_err(r32[k], ref))
        else:
            vec, rem = max(vec, max_norm_err(r32[k], ref)), max(rem, elem_remainder(r32[k], ref))
    return vec, rem, scal


@functools.lru_cache(maxsize=None)
def make_v1_inputs(O, I, seed):
    """The inputs of one V1 call at this seed (shared: do not write to them), kept by the same rule as V2's: the sum S
    behind da_mu = -G S (1 - a^2) / O cancels, and all of da_mu carries what float32 loses on it."""
    for redraw in range(MAX_REDRAWS):
        d = draw_v1_inputs(O, I, seed + 1000 * redraw)
        vec, rem, scal = v1_e32_of(d)
        if vec <= E32_VEC and rem <= E32_REM and 4.0 * scal <= SCALAR_FLOOR:
            return d
    raise RuntimeError("no well-conditioned draw at %r" % ((O, I, seed),))


def v1_reference(d, dtype=torch.float64):
    """{'da_mu', 'da_var': dF1/d., 'aux0': m} in ``dtype``."""
    c = {k: v.detach().to(dtype).clone() for k, v in d.items()}
    c["act_mu"].requires_grad_(True)
    c["act_var"].requires_grad_(True)
    m = torch.tanh(c["act_mu"] + torch.sqrt(c["act_var"]) * c["eps_act"]).mean()
    F1 = -c["g_kl"][0] * _log_rb(c["zb_last"][0], c["r0_b1"], c["r0_b2"], m)
    da_mu, da_var = torch.autograd.grad(F1, [c["act_mu"], c["act_var"]])
    return {"da_mu": da_mu.detach(), "da_var": da_var.detach(), "aux0": m.detach().reshape(1)}


# --------------------------------------------------------------------------- the bars
def max_norm_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def elem_remainder(got, ref):
    """Worst (|got - ref| - ELEM_RTOL |ref|) / max|ref| over the elements: the `a` the element-wise bar would need."""
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() - ELEM_RTOL * ref.abs()).max().clamp_min(0) / ref.abs().max().clamp_min(1e-300))


def scalar_bar(r32, r64):
    """Bar of a one-element leaf: it is a sum that cancels, so four times what plain fp32 loses on these very inputs,
    and never below SCALAR_FLOOR."""
    return max(SCALAR_FLOOR, 4.0 * max_norm_err(r32, r64))


def check_leaves(got, r64, r32, a_elem, tag, tally=None):
    """The bars of one call: ``got`` against the float64 reference ``r64``; ``r32`` (the same formula in float32) sets the
    bars of the one-element leaves.  Returns the failures as strings; ``tally`` collects (bar, error) of every
    one-element leaf and (max-norm error, remainder) of every vector leaf."""
    bad = []
    for k, ref in r64.items():
        g = got[k].double().reshape(ref.shape)
        if not bool(torch.isfinite(g).all()):
            bad.append("%s %s: not finite" % (tag, k))
        elif float(ref.abs().max()) == 0.0:
            if float(g.abs().max()) != 0.0:
                bad.append("%s %s: reference is exactly zero, got max %.3g" % (tag, k, float(g.abs().max())))
        elif ref.numel() == 1:
            bar, err = scalar_bar(r32[k], ref), max_norm_err(g, ref)
            if tally is not None:
                tally.setdefault("scalar", []).append((bar, err, tag, k))
            if bar > SCALAR_CEIL:
                bad.append("%s %s: the reference itself needs a bar of %.3g" % (tag, k, bar))
            if err > bar:
                bad.append("%s %s: %.3g of the value (bar %.3g)" % (tag, k, err, bar))
        else:
            err, rem = max_norm_err(g, ref), elem_remainder(g, ref)
            if tally is not None:
                tally.setdefault("vector", []).append((err, rem, tag, k))
            if not err < VEC_BAR:
                bad.append("%s %s: max-norm %.3g (bar %.3g)" % (tag, k, err, VEC_BAR))
            if rem > a_elem:
                bad.append("%s %s: element-wise remainder %.3g of the max (bar %.3g)" % (tag, k, rem, a_elem))
    return bad
