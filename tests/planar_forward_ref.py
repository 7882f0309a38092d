"""Reference for the planar-flow forward (K3, lbbnn_mnf_flow_planar) and the KL tail (K5, lbbnn_kl_finalize /
lbbnn_layers_finalize) of csrc/mnf_flow.hip -- plain torch, no GPU.

K3 and K5 are restated below from the oracle's own pieces (``oracle.planar_step_1d``, ``oracle.kl_bias_term``, the log_q0 and
log_rb lines of ``oracle.mnf_forward``) so that every output the kernels write is a return value of its own:

    z0 = q0_mean + exp(q0_log_var)^.5 eps        z_fwd = zflow(z0(eps_fwd))        z_kl, ldq = zflow(z0(eps_kl))
    log_q0 = Sum_i( -0.5 log pi - 0.5 lv_i - 0.5 (z0_i - q0_mean_i)^2 / exp(lv_i) )        zb, ldr = rflow(z_kl)
    scal = [ldq, log_q0, ldr, zb[-1], log-det of the forward draw's zflow]
    m = mean_o tanh(act_mu + sqrt(act_var) eps_act)
    log_rb = Sum_i( -0.5 log pi - 0.5 b2_i m - 0.5 (zb[-1] - b1_i m)^2 / exp(b2_i m) )
    kl = Sum kl_rows + kl_bias + (-ldq + log_q0) - (ldr + log_rb)                          (LRT: the first two terms)

float64 is the truth, float32 of the very same lines the yardstick E32.  The inputs are scaled so that the flows visibly act
(the reference initialisation, u, w ~ U(+-0.01), leaves every log-det at 1e-7 of the KL): u has elements of order one, w is
built so that u.w of transform t is a chosen value UW[t % 4] -- one of them below -1, the abs() branch of the log-det -- and
every bias so that w.z + b on the KL draw is a chosen value INNER[t % 5].  Marked cases give one r-flow transform a saturated
tanh (|w.z + b| > 6, with u.w large enough that its log-det still counts) and one a tiny argument (< 1e-3).  A draw is kept
only if the float64 reference shows the conditioning the bars assume (``conditioned``); otherwise the next one is taken (seed
+ 1000, + 2000, ...).  The rule looks at the reference alone, never at a kernel."""
import functools
import math

import torch

from oracle import lbbnn_oracle as orc

LDS_BUDGET = 144 * 1024        # kFlowLdsBudget: dynamic LDS of the lds / fast forms of K3 and the staged forms of K5
LDS_RAISE = 64 * 1024          # above this the launcher raises the kernel's dynamic-LDS attribute first
GENERIC, LDS, FAST, VEC = 0, 1, 2, 3          # LBBNN_K3_*
K5_GENERIC, K5_LDS = 0, 1                     # LBBNN_K5_* (per-layer launch); all-layers launch: 0 unstaged, 1 staged
FORM_NAME = {GENERIC: "generic", LDS: "lds", FAST: "fast", VEC: "vec"}

TIGHT = 5e-6                   # test_parity_gpu.TIGHT: the bar of a z vector (max-norm) and the floor of a one-number bar, in units of S
TOL = 1e-4                     # test_parity_gpu.TOL, the contract: no one-number bar may need more than TOL * S
WIDE_FRAC = 0.01               # at most this share of the one-number bars may lie above the floor

UW = (0.8, -4.0, 1.5, -0.45)                   # u.w of transform t (index t % 4); -4: 1 + (1 - th^2) u.w < 0 for |th| < 0.86
INNER = (0.9, -0.35, 0.25, -0.8, 0.6)          # w.z + b of transform t on the KL draw (index t % 5)
SAT_INNER, SAT_UW = 6.1, 2.0e4                 # saturated: 1 - th^2 = 2.0e-5, (1 - th^2) u.w = 0.40
TINY_INNER = 5.0e-4
MIN_DISPLACEMENT, MIN_LD, MIN_ARG = 0.1, 1e-2, 0.1
MAX_REDRAWS = 64


def need_bytes(I, Tz, Tr, want_kl):
    """Dynamic LDS of the lds / fast forms for one layer (launch_flow_planar)."""
    return 4 * (4 + 2 * (Tz + (Tr if want_kl else 0))) * (((I + 63) // 64) * 64)


# ------------------------------------------------------------------------------------------------ the tables
# K3, single entry: (form, I, Tz, Tr, want_kl, offset, special).  offset: the one input handed in as a contiguous view one float
# past a 16-byte boundary; special: the r-flow transforms given the saturated / tiny argument.
def _k3_table():
    rows = []

    def add(form, I, Tz, Tr, kl, offset=None, special=None):
        rows.append((form, I, Tz, Tr, kl, offset, special))

    for I in (4, 8, 252, 256, 260, 2048):
        for Tz, Tr in ((2, 2), (1, 3), (3, 1), (0, 4)):
            add(VEC, I, Tz, Tr, True, None, {"sat": 0, "tiny": 2} if (I, Tz, Tr) == (256, 1, 3) else None)
            add(VEC, I, Tz, Tr, False)
        for Tz in (4, 0, 1):
            add(VEC, I, Tz, 0, False)
    for I in (1, 2, 3, 5, 63, 65, 513, 2049, 2052):
        for Tz, Tr in ((2, 2), (1, 3), (0, 2)):
            add(FAST, I, Tz, Tr, True, None, {"sat": 1, "tiny": 0} if (I, Tz, Tr) == (65, 1, 3) else None)
            add(FAST, I, Tz, Tr, False)
        add(FAST, I, 4, 0, False)
    for I in (256, 2048):
        for off in ("q0_mean", "z.1.u", "r.0.w", "eps_kl", "z_fwd", "z_kl"):
            add(FAST, I, 2, 2, True, off)
    add(FAST, 3072, 2, 2, True)
    for I in (1, 5, 64, 257, 1025):
        add(LDS, I, 3, 2, True, None, {"sat": 0, "tiny": 1} if I == 257 else None)
        add(LDS, I, 5, 0, False)
    add(LDS, 512, 16, 16, True)
    add(LDS, 512, 16, 16, False)
    add(LDS, 1025, 8, 6, True)
    add(LDS, 1025, 8, 6, False)
    add(GENERIC, 3073, 2, 2, True, None, {"sat": 1, "tiny": 0})
    add(GENERIC, 513, 16, 16, True)
    add(GENERIC, 1025, 16, 0, False)
    add(GENERIC, 1025, 8, 7, True)
    add(GENERIC, 16384, 2, 2, True)
    add(GENERIC, 16384, 2, 2, False)
    return rows


K3_CASES = _k3_table()
K3_O = 3                                       # the K5 half of a K3 case's inputs is not used: any O


def k3_id(c):
    form, I, Tz, Tr, kl, off, sp = c
    return "%s-%d-%dx%d-%s%s%s" % (FORM_NAME[form], I, Tz, Tr, "kl" if kl else "nokl", "-off:" + off if off else "",
                                   "-special" if sp else "")


# K5, single entry: (form, O, I, mnf)
K5_CASES = ([(K5_LDS, O, I, True) for O in (1, 3, 64, 65, 257) for I in (1, 5, 300)]
            + [(K5_LDS, O, 0, False) for O in (1, 3, 64, 65, 257)]
            + [(K5_LDS, 3000, 300, True), (K5_LDS, 3000, 0, False), (K5_LDS, 6080, 0, False), (K5_GENERIC, 6081, 0, False),
               (K5_GENERIC, 6145, 0, False), (K5_GENERIC, 700, 16384, True)])
K5_VARIANT_CASES = [(K5_LDS, 65, 300, True), (K5_LDS, 257, 0, False), (K5_LDS, 3000, 300, True), (K5_GENERIC, 6145, 0, False),
                    (K5_GENERIC, 700, 16384, True)]

# Batched launches through lbbnn_layers_prepare: name -> (form of the K3 launch, [(I, O, Tz, Tr, want_kl, mnf)]).  Weights are
# O <= 8 rows.  An LRT layer (mnf False) takes no part in K3.
PREPARE_GROUPS = {
    "n2-vec": (VEC, [(256, 3, 2, 2, True, True), (8, 8, 1, 3, True, True)]),
    "n3-fast-lrt": (FAST, [(256, 3, 2, 2, True, True), (40, 5, 0, 0, True, False), (5, 4, 2, 2, True, True)]),
    "n4-fast": (FAST, [(63, 3, 2, 2, True, True), (2052, 2, 1, 3, True, True), (1, 8, 0, 2, True, True), (260, 1, 2, 2, True, True)]),
    "n2-lds": (LDS, [(256, 3, 2, 2, True, True), (257, 3, 3, 2, True, True)]),
    "n3-generic": (GENERIC, [(256, 3, 2, 2, True, True), (3073, 2, 2, 2, True, True), (5, 4, 1, 3, True, True)]),
    "n3-nokl-between": (VEC, [(256, 3, 2, 2, True, True), (260, 4, 2, 2, False, True), (8, 8, 1, 3, True, True)]),
}

# All-layers tail through lbbnn_layers_finalize: name -> (staged, [(O, I, mnf, active)], in-kernel eps_act, advance)
FINALIZE_GROUPS = {
    "n1": (1, [(65, 300, True, True)], False, 0),
    "n2-lrt": (1, [(257, 5, True, True), (64, 0, False, True)], False, 3),
    "n3-inactive": (1, [(3, 300, True, True), (65, 5, True, False), (1, 1, True, True)], False, 0),
    "n4": (1, [(64, 1, True, True), (257, 0, False, True), (65, 300, True, True), (3, 5, True, True)], False, 1),
    "n4-draws": (1, [(65, 300, True, True), (257, 0, False, True), (3, 5, True, True), (1030, 64, True, True)], True, 5),
    "n4-unstaged": (0, [(1600, 300, True, True), (1600, 0, False, True), (1600, 5, True, True), (1600, 64, True, True)], False, 2),
    "n3-unstaged-lrt": (0, [(2100, 5, True, True), (2100, 0, False, True), (2100, 64, True, True)], False, 0),
    "n4-unstaged-draws": (0, [(1600, 300, True, True), (1600, 0, False, True), (1600, 5, True, True), (1600, 64, True, True)],
                          True, 7),
}


# ------------------------------------------------------------------------------------------------ inputs
def _names(fl, T):
    return [("%s.%d.u" % (fl, t), "%s.%d.w" % (fl, t), "%s.%d.b" % (fl, t)) for t in range(T)]


def flow_params(d, fl, T):
    return [tuple(d[k] for k in n3) for n3 in _names(fl, T)]


def _draw(I, O, Tz, Tr, gen_seed, special):
    """One draw, float32 on the CPU.  u, w, b are built transform by transform along the float64 chain of the KL draw."""
    g = torch.Generator().manual_seed(gen_seed)
    n = lambda k: torch.randn(k, generator=g)
    U = lambda k, lo, hi: torch.empty(k).uniform_(lo, hi, generator=g)
    d = {"q0_mean": 0.3 + 0.5 * n(I), "q0_log_var": U(I, -9.0, 1.0), "eps_fwd": n(I), "eps_kl": n(I)}
    z = d["q0_mean"].double() + torch.exp(0.5 * d["q0_log_var"].double()) * d["eps_kl"].double()
    sat = (special or {}).get("sat", -1)
    tiny = (special or {}).get("tiny", -1)
    for fl, T in (("z", Tz), ("r", Tr)):
        for t in range(T):
            k = t + (Tz if fl == "r" else 0)
            u = n(I)
            uw, inner = UW[k % 4], INNER[k % 5]
            if fl == "r" and t == sat:
                uw, inner = SAT_UW, SAT_INNER
            if fl == "r" and t == tiny:
                inner = TINY_INNER
            noise = 0.3 * n(I) / math.sqrt(I)
            c = uw - float(torch.dot(u.double(), noise.double()))
            w = (noise.double() + c * u.double() / torch.dot(u.double(), u.double())).float()
            b = torch.tensor([inner - float(torch.dot(w.double(), z))], dtype=torch.float32)
            d["%s.%d.u" % (fl, t)], d["%s.%d.w" % (fl, t)], d["%s.%d.b" % (fl, t)] = u, w, b
            z = z + u.double() * torch.tanh(torch.dot(w.double(), z) + b.double())
    d.update(_draw_k5(O, I, g))
    return d


def _draw_k5(O, I, g, mnf=True):
    """The K5 half: vectors at natural scales, then bias_mu, scal[3] (z_b[-1]), kl_rows and scal[0..2] sized so that every
    term of the KL is a visible share of the whole."""
    n = lambda k: torch.randn(k, generator=g)
    d = {"bias_mu": 0.1 * n(O), "bias_rho": -3 + n(O), "kl_rows": torch.rand(O, generator=g) + 0.5}
    I = max(I, 1)
    d.update({"act_mu": 0.5 * n(O), "act_var": torch.exp(-2 + 0.3 * n(O)), "eps_act": n(O), "r0_b1": 0.5 * n(I), "r0_b2": 0.5 * n(I)})
    pr = orc.Priors()
    kb = abs(float(orc.kl_bias_term(d["bias_mu"].double(), d["bias_rho"].double(), pr)))
    zb = 0.8
    if mnf:
        rb = abs(float(_log_rb(torch.tensor(zb, dtype=torch.float64), d["r0_b1"].double(), d["r0_b2"].double(), _act_mean(d, torch.float64))))
        if rb < 0.3 * kb:                         # few inputs, many outputs: move z_b[-1] away from the mean
            zb = math.sqrt(2.0 * 0.3 * kb / I + zb * zb)
        elif kb < 0.3 * rb:                       # few outputs, many inputs: move bias_mu away from its prior
            d["bias_mu"] = d["bias_mu"] + math.sqrt(2.0 * 0.3 * rb / O) * torch.sign(d["bias_mu"])
            kb = abs(float(orc.kl_bias_term(d["bias_mu"].double(), d["bias_rho"].double(), pr)))
        rb = abs(float(_log_rb(torch.tensor(zb, dtype=torch.float64), d["r0_b1"].double(), d["r0_b2"].double(), _act_mean(d, torch.float64))))
    else:
        rb = 0.0
    M = max(kb, rb, 1.0)
    d["kl_rows"] = d["kl_rows"] * (0.7 * M / float(d["kl_rows"].sum()))
    d["scal_k5"] = torch.tensor([0.3 * M, -0.5 * M, 0.4 * M, zb, 0.0, 0.0, 0.0, 0.0])
    return d


def conditioned(d, Tz, Tr):
    """The conditioning the bars assume, from the float64 reference alone: returns the list of what is violated."""
    bad = []
    r = k3_reference(d, True, torch.float64)
    for path in ("fwd", "kl"):
        for (fl, t, inner, arg, ld) in r["diag"][path]:
            if abs(ld) < MIN_LD:
                bad.append("%s %s.%d: |log-det| %.3g" % (path, fl, t, abs(ld)))
            if abs(arg) < MIN_ARG:
                bad.append("%s %s.%d: |1 + (1 - th^2) u.w| %.3g" % (path, fl, t, abs(arg)))
        if Tz and r["disp_" + path] < MIN_DISPLACEMENT:
            bad.append("%s: displacement %.3g of max|z0|" % (path, r["disp_" + path]))
    return bad


@functools.lru_cache(maxsize=None)
def _kept_draw(I, O, Tz, Tr, seed, special):
    for redraw in range(MAX_REDRAWS):
        d = _draw(I, O, Tz, Tr, seed + 1000 * redraw, dict(special) if special else None)
        if not conditioned(d, Tz, Tr):
            return d
    raise RuntimeError("no well-conditioned draw at %r" % ((I, O, Tz, Tr, seed, special),))


def make_inputs(I, O, Tz, Tr, seed, special=None):
    """The inputs of one K3 call and of one K5 call at this seed, float32 on the CPU (shared: do not write to them)."""
    return _kept_draw(I, O, Tz, Tr, seed, tuple(sorted(special.items())) if special else None)


@functools.lru_cache(maxsize=None)
def make_k5_inputs(O, I, seed, mnf=True):
    """The inputs of one K5 call alone (no flow), float32 on the CPU (shared: do not write to them)."""
    return _draw_k5(O, I, torch.Generator().manual_seed(seed), mnf)


# ------------------------------------------------------------------------------------------------ K3
def _flow(z, d, fl, T, diag, S):
    """(z after the flow, sum of log-dets); appends (flow, t, inner, 1 + (1 - th^2) u.w, log-det) per transform to diag and adds
    Sum |u_i w_i| to S["uw_" + fl] and |u[-1] th| to S["last"]."""
    ld = z.new_zeros(())
    for t, (u, w, b) in enumerate(flow_params(d, fl, T)):
        inner = torch.dot(w, z) + b[0]
        z_new, l = orc.planar_step_1d(z, u, w, b)
        th = torch.tanh(inner)
        diag.append((fl, t, float(inner), float(1 + (1 - th * th) * torch.dot(u, w)), float(l.sum())))
        S["uw_" + fl] = S.get("uw_" + fl, 0.0) + float((u * w).abs().sum())
        S["last"] = S.get("last", 0.0) + float((u[-1] * th).abs())
        z, ld = z_new, ld + l.sum()
    return z, ld


def k3_reference(inputs, want_kl, dtype=torch.float64):
    """{'z_fwd', 'z_kl' (None without the KL branch), 'scal': 5 values (NaN where the kernel writes nothing)} in ``dtype``, and,
    for the bars, 'S': the magnitude sums of the one-number outputs, 'diag', 'disp_fwd' / 'disp_kl'."""
    d = {k: v.to(dtype) for k, v in inputs.items()}
    Tz = sum(1 for k in d if k.startswith("z.") and k.endswith(".u"))
    Tr = sum(1 for k in d if k.startswith("r.") and k.endswith(".u"))
    sd = d["q0_log_var"].exp().sqrt()                                  # oracle.mnf_sample_z
    out = {"diag": {"fwd": [], "kl": []}, "z_kl": None}
    nan = float("nan")
    z0 = d["q0_mean"] + sd * d["eps_fwd"]
    Sf = {}
    zf, ld_f = _flow(z0, d, "z", Tz, out["diag"]["fwd"], Sf)
    out["z_fwd"] = zf
    out["disp_fwd"] = float((zf - z0).abs().max() / z0.abs().max())
    scal = [nan, nan, nan, nan, float(ld_f)]
    S = {"ld_fwd": max(1.0, Sf.get("uw_z", 0.0))}
    if want_kl:
        z0 = d["q0_mean"] + sd * d["eps_kl"]
        Sk = {}
        z2, ldq = _flow(z0, d, "z", Tz, out["diag"]["kl"], Sk)
        terms = -0.5 * math.log(math.pi) - 0.5 * d["q0_log_var"] - 0.5 * ((z0 - d["q0_mean"]) ** 2 / d["q0_log_var"].exp())
        zb, ldr = _flow(z2, d, "r", Tr, out["diag"]["kl"], Sk)
        out["z_kl"] = z2
        out["disp_kl"] = float((z2 - z0).abs().max() / z0.abs().max())
        scal[:4] = [float(ldq), float(terms.sum()), float(ldr), float(zb[-1])]
        S.update(ldq=max(1.0, Sk.get("uw_z", 0.0)), log_q0=float(terms.abs().sum()), ldr=max(1.0, Sk.get("uw_r", 0.0)),
                 zb=float(d["q0_mean"][-1].abs() + (sd[-1] * d["eps_kl"][-1]).abs()) + Sk.get("last", 0.0))
    out["scal"] = scal
    out["S"] = S
    return out


SCAL_NAMES = ("ldq", "log_q0", "ldr", "zb", "ld_fwd")


def one_number_bar(S, r32, r64):
    """|got - r64| <= max(TIGHT S, 4 E32): S the sum of the magnitudes of the terms, E32 what plain float32 of the same
    formula loses on these inputs."""
    return max(TIGHT * S, 4.0 * abs(r32 - r64))


@functools.lru_cache(maxsize=None)
def k3_references(I, Tz, Tr, seed, want_kl, special=None):
    """(float64 reference, float32 reference) of make_inputs(I, K3_O, Tz, Tr, seed, special): computed once, shared."""
    d = make_inputs(I, K3_O, Tz, Tr, seed, dict(special) if special else None)
    return k3_reference(d, want_kl), k3_reference(d, want_kl, torch.float32)


def k3_bars(r64, r32):
    """{name: (bar, S)} of the scal values the call writes."""
    bars = {}
    for i, name in enumerate(SCAL_NAMES):
        if not math.isnan(r64["scal"][i]):
            S = r64["S"][name]
            bars[name] = (one_number_bar(S, r32["scal"][i], r64["scal"][i]), S)
    return bars


# ------------------------------------------------------------------------------------------------ K5
def _act_mean(d, dtype):
    return torch.tanh(d["act_mu"].to(dtype) + d["act_var"].to(dtype).sqrt() * d["eps_act"].to(dtype)).mean()


def _rb_terms(zb_last, b1, b2, m):
    mean_r, log_var_r = b1 * m, b2 * m                                 # outer(b, act).mean(-1) = b mean(act)
    return -0.5 * math.log(math.pi) - 0.5 * log_var_r - 0.5 * ((zb_last - mean_r) ** 2 / log_var_r.exp())


def _log_rb(zb_last, b1, b2, m):
    return _rb_terms(zb_last, b1, b2, m).sum()


def k5_reference(inputs, scal, dtype=torch.float64, priors=None):
    """The layer KL and its terms in ``dtype``; scal = None: an LRT layer.  'S': the sum of the magnitudes of everything the
    KL is a sum of; 'terms': the five terms as they enter."""
    d = {k: v.to(dtype) for k, v in inputs.items() if torch.is_tensor(v)}
    pr = priors or orc.Priors()
    sb = orc.sigma_of(d["bias_rho"])
    bias_terms = (torch.log(pr.bias_sigma_prior / sb) - 0.5
                  + (sb ** 2 + (d["bias_mu"] - pr.bias_mu_prior) ** 2) / (2 * pr.bias_sigma_prior ** 2))
    rows, bias = d["kl_rows"].sum(), orc.kl_bias_term(d["bias_mu"], d["bias_rho"], pr)
    out = {"rows": float(rows), "bias": float(bias), "log_q": 0.0, "log_det_r": 0.0, "log_rb": 0.0}
    S = float(d["kl_rows"].abs().sum() + bias_terms.abs().sum())
    kl = bias + rows                                                   # oracle.mnf_forward: kl_b + kl_w ...
    if scal is not None:
        s = torch.as_tensor(scal, dtype=torch.float32)[:4].to(dtype)   # the kernel reads them as float32
        m = _act_mean(d, dtype)
        rb_terms = _rb_terms(s[3], d["r0_b1"], d["r0_b2"], m)
        log_q = -s[0] + s[1]
        log_r = s[2] + rb_terms.sum()
        kl = kl + log_q - log_r                                        # ... + log_q - log_r
        out.update(log_q=float(log_q), log_det_r=float(s[2]), log_rb=float(rb_terms.sum()), m=float(m))
        S += float(s[0].abs() + s[1].abs() + s[2].abs() + rb_terms.abs().sum())
    out["kl"] = float(kl)
    out["S"] = S
    out["terms"] = [out["rows"], out["bias"], out["log_q"], -out["log_det_r"], -out["log_rb"]]
    return out


def k5_bar(r64, r32):
    return one_number_bar(r64["S"], r32["kl"], r64["kl"])


def smallest_term_share(r):
    """min |term| / Sum |term| over the terms of the KL (two for an LRT layer, five for an MNF one)."""
    t = [abs(v) for v in r["terms"] if v != 0.0]
    return min(t) / sum(t)


# ------------------------------------------------------------------------------------------------ the forms, from the library
def k3_form(layers, members=1):
    """lbbnn_flow_planar_form for [(I, Tz, Tr, want_kl, aligned16)]: the form of the launch, or its LBBNN_E_* code."""
    from bnn_amd import ops
    return ops.flow_planar_form(layers, members)


def k5_form(layers, all_layers=False):
    """lbbnn_kl_finalize_form for [(O, I, mnf, active)]."""
    from bnn_amd import ops
    return ops.kl_finalize_form(layers, all_layers)


def k3_case_form(c):
    form, I, Tz, Tr, kl, off, sp = c
    return k3_form([(I, Tz, Tr, kl, off is None)])


def rel_err(got, ref):
    """conftest.rel_err: max-norm."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))
