"""Baseline LBBNN (explicit latent-binary gate x Gaussian weight sampling), names as in LBBNN-GP-MF.py:

``BayesianLinear(in_features, out_features, layer_id)`` :182-255 -- ``forward(input, cgamma, sample=False,
medimean=False, calculate_log_probs=False)``, attributes ``log_prior``, ``log_variational_posterior``,
``alpha``, ``gammas``, ``gamma``, ``weight_prior``, ``bias_prior``, ``gamma_prior`` (each with ``.exact``);
``BayesianNetwork`` :259-319 with ``sample_elbo``.  The fused pass (sample W = gamma*(mu+sigma*eps), all four
Monte-Carlo log-probability sums) and ``F.linear`` run in HIP (lbbnn_gate_sample + lbbnn_lrt_gemm).
"""
import ctypes
import itertools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .distributions import Bernoulli, Gaussian, TEMPER_PRIOR  # noqa: F401  (TEMPER_PRIOR re-exported: the reference scripts read it here)

_ids = itertools.count(32)
SAMPLES = 1              # LBBNN-GP-MF.py:38
# torch.distributions' argument checks of the Gamma / Beta / RelaxedBernoulli draws below: each is a compare + reduce + a
# host read-back of one bool -- ~35 device-to-host syncs and ~60 launches per sample_elbo step on a GPU (the reference runs on the
# CPU, where they cost nothing).  The parameters checked are softplus / sigmoid outputs and the positive prior constants: a
# check can only fire on NaN parameters.  True restores torch's default behaviour (a ValueError at the draw).
VALIDATE_ARGS = False
MAX_DEPTH = _lib.MAX_DEPTH   # layers per network: layer i takes Philox stream id 32 + i (LRT / MNF: 0..15, VD: 48..63)
NUM_BATCHES = 600        # len(train_loader) with BATCH_SIZE = 100 on MNIST (LBBNN-GP-MF.py:34,67)


class GaussGamma(object):
    """Normal-Gamma prior helper (LBBNN-GP-MF.py:132-151): a, b and the ``exact`` switch.  On the hot path the density is
    evaluated inside the HIP pass (lbbnn_gate_sample) with the Gamma(a, b) draw of :141 taken by ``rsample_tau``;
    ``log_prob`` is the same density as torch ops, for callers that evaluate the prior outside ``forward`` and for the
    differentiable posterior-mean branches of the layer."""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.exact = False

    def rsample_tau(self):
        return torch.distributions.Gamma(self.a, self.b, validate_args=VALIDATE_ARGS).rsample()

    def log_prob(self, input, gamma, tau=None):
        """:140-151.  ``tau``: the Gamma(a, b) draw (default: a fresh ``rsample``, as the reference draws one per call)."""
        if tau is None:
            tau = self.rsample_tau()                                                     # :141
        g = torch.round(gamma.detach()) if self.exact else gamma                         # :142-143
        a, b = self.a, self.b
        return (g * (a * torch.log(b) + (a - 0.5) * tau - b * tau - torch.lgamma(a)
                     - 0.5 * math.log(2 * math.pi)) - tau * torch.pow(input, 2) + (1 - g) + 1e-8).sum()   # :144-150


class BetaBinomial(object):
    """LBBNN-GP-MF.py:155-179."""

    def __init__(self, pa, pb):
        self.pa, self.pb = pa, pb
        self.exact = False

    def log_prob(self, input, pa=None, pb=None):
        """:162-173 (the reference takes pa / pb arguments and ignores them in favour of the attributes; so does this)."""
        g = torch.round(input.detach()) if self.exact else input
        one = torch.ones_like(input)
        pa_, pb_ = self.pa, self.pb
        return (torch.lgamma(one) + torch.lgamma(g + one * pa_) + torch.lgamma(one * (1 + pb_) - g)
                + torch.lgamma(one * (pa_ + pb_)) - torch.lgamma(one * pa_ + g) - torch.lgamma(one * 2 - g)
                - torch.lgamma(one * (1 + pa_ + pb_)) - torch.lgamma(one * pa_) - torch.lgamma(one * pb_)).sum()

    def rsample(self):
        p = torch.distributions.Beta(self.pa, self.pb, validate_args=VALIDATE_ARGS).rsample()
        return torch.distributions.RelaxedBernoulli(probs=p, temperature=0.001, validate_args=VALIDATE_ARGS).rsample()


class _BaseFn(torch.autograd.Function):
    """Forward: lbbnn_gate_sample + the mean-only GEMM.  Backward (round 2: all on the HIP kernels; round 1 recomputed the
    layer with torch ops): lbbnn_output_grad (G^T, column sums) -> dW = G^T x on the GEMM kernel -> lbbnn_gate_backward
    (K6b: every (O,I)-, (O)- and scalar-sized gradient in one pass + tail, and the sampled W as a dense matrix) ->
    dX = G W on the GEMM kernel.  ``galpha`` is ``layer.gamma.alpha`` as an autograd input: Bernoulli.log_prob
    differentiates through it (LBBNN-GP-MF.py:125-127, alpha = sigmoid(lambdal) set by sample_elbo :292-297)."""

    @staticmethod
    def forward(ctx, layer, x, cgamma, tau_w, tau_b, galpha, cfg, *params):
        out, lp, lq, saved = layer._forward_hip(x, cgamma, tau_w, tau_b, cfg, save_rng=True)
        ctx.layer, ctx.cfg, ctx.saved = layer, cfg, saved
        from . import graphs
        graphs.mark_autograd_node(ctx, layer)          # capture guard: graphs.assert_no_live_graph
        ctx.save_for_backward(x, tau_w, tau_b, *params)
        z = out.new_zeros(())
        return out, (lp if lp is not None else z), (lq if lq is not None else z)

    @staticmethod
    def backward(ctx, g_out, g_lp, g_lq):
        from .layers import _hip_matmul_nt
        layer, cfg, saved = ctx.layer, ctx.cfg, ctx.saved
        x, tau_w, tau_b, *params = ctx.saved_tensors
        P = dict(zip(layer._names, params))
        O, I, dev = layer.out_features, layer.in_features, x.device
        f = dict(dtype=torch.float32, device=dev)
        noise = saved.get("noise") or {}
        gm, _, gmT, _, g_sum, _ = ops.output_grad(g_out.contiguous())
        dW = _hip_matmul_nt(gmT, ops.transpose_operand, x)                       # (O,I) = G^T x
        a = _lib.GateBwdArgs()
        keep = []

        def dptr(t):
            if t is None:
                return None
            u = t.detach()
            if u.dtype != torch.float32 or not u.is_contiguous():
                u = u.float().contiguous()
            keep.append(u)
            return ops._ptr(u, "tensor")
        a.mu, a.rho = dptr(P["weight_mu"]), dptr(P["weight_rho"])
        a.gamma_alpha, a.cgamma = dptr(saved["gamma_alpha"]), dptr(saved["cg"])
        a.eps_w, a.eps_b = dptr(noise.get("eps_w")), dptr(noise.get("eps_b"))
        a.bias_mu, a.bias_rho, a.bias_a, a.bias_b = dptr(P["bias_mu"]), dptr(P["bias_rho"]), dptr(P["bias_a"]), dptr(P["bias_b"])
        a.tau_b, a.tau_w = dptr(tau_b), dptr(tau_w)
        a.weight_a, a.weight_b, a.pa, a.pb = dptr(P["weight_a"]), dptr(P["weight_b"]), dptr(P["pa"]), dptr(P["pb"])
        a.dW, a.g_sum = dW.data_ptr(), g_sum.data_ptr()
        a.g_lp, a.g_lq = dptr(g_lp.reshape(1)), dptr(g_lq.reshape(1))
        outs = {n: torch.empty((O, I), **f) for n in ("d_mu", "d_rho", "d_cgamma", "d_alpha", "w_out")}
        vecs = {n: torch.empty(O, **f) for n in ("d_bias_mu", "d_bias_rho", "d_bias_a", "d_bias_b", "d_tau_b")}
        scal, rows = torch.empty(5, **f), torch.empty(3 * O, **f)
        for n, t in list(outs.items()) + list(vecs.items()):
            setattr(a, n, t.data_ptr())
        a.d_scalars, a.rows = scal.data_ptr(), rows.data_ptr()
        a.O, a.I, a.exact, a.layer_id = O, I, cfg[2], layer._layer_id
        rng = saved.get("rng")
        _lib.check(_lib.lib().lbbnn_gate_backward(ctypes.byref(a), rng.data_ptr() if rng is not None else None, ops._stream()),
                   "lbbnn_gate_backward")
        del keep
        gx = _hip_matmul_nt(gm, ops.transpose_operand, outs["w_out"]) if ctx.needs_input_grad[1] else None   # G W
        grads = {"weight_mu": outs["d_mu"], "weight_rho": outs["d_rho"], "weight_a": scal[0:1], "weight_b": scal[1:2],
                 "lambdal": None, "pa": scal[3:4], "pb": scal[4:5], "bias_mu": vecs["d_bias_mu"],
                 "bias_rho": vecs["d_bias_rho"], "bias_a": vecs["d_bias_a"], "bias_b": vecs["d_bias_b"]}
        return (None, gx, outs["d_cgamma"], scal[2:3].reshape(tau_w.shape), vecs["d_tau_b"].reshape(tau_b.shape),
                outs["d_alpha"], None, *[grads[n] for n in layer._names])


class _BaseDrawFn(torch.autograd.Function):
    """``sample_elbo(draws="hip")``: one node per layer, parameters in, (out, log_prior, log_q) out.  Forward:
    lbbnn_gate_sample_draw (gates, tau_w, tau_b and eps from the Philox snapshot ``rng``; W and the four log-probability sums)
    + the mean-only GEMM with the layer's activation in its epilogue (ReLU, or the head's log_softmax).  Backward: the
    log_softmax / ReLU mask + G^T + column sums (lbbnn_output_grad, or the loss's own logits gradient) -> dW = G^T x ->
    lbbnn_gate_backward_draw (every parameter gradient, d lambdal through the gate and through alpha, the Gamma
    reparameterisation terms) -> dX = G W.  No torch distribution and no sigmoid autograd on the path."""

    @staticmethod
    def forward(ctx, layer, x, rng, act, slot, *params):
        out, lp, lq, keep = layer._forward_hip_draws(x, rng, act, slot)
        ctx.layer, ctx.act, ctx.rng, ctx.keep = layer, act, rng, keep
        from . import graphs
        graphs.mark_autograd_node(ctx, layer)          # capture guard: graphs.assert_no_live_graph
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, out, keep["tau_w"], keep["tau_b"], *params)
        return out, lp, lq

    @staticmethod
    def backward(ctx, g_out, g_lp, g_lq):
        from .layers import _hip_matmul_nt
        layer, act, keep = ctx.layer, ctx.act, ctx.keep
        x, out, tau_w, tau_b, *params = ctx.saved_tensors
        P = dict(zip(layer._names, params))
        O, I, dev = layer.out_features, layer.in_features, x.device
        f = dict(dtype=torch.float32, device=dev)
        if g_out is None:
            g_out = torch.zeros_like(out)
        if act == "log_softmax":
            from . import losses
            left = losses._HEAD_GRAD.take(out, g_out)          # formed by the loss's own backward launch (losses._Handover)
            g_out = left if left is not None else ops.log_softmax_backward(g_out, out)
        relu = act == "relu"
        want_gx = bool(ctx.needs_input_grad[1])
        gm, _, gmT, _, g_sum, _ = ops.output_grad(g_out.contiguous(), out=out if relu else None, relu=relu, want_g=want_gx)
        dW = _hip_matmul_nt(gmT, ops.transpose_operand, x)                       # (O,I) = G^T x
        a = _lib.GateBwdDrawArgs()
        b = a.g
        kept = []

        def dptr(t):
            if t is None:
                return None
            u = t.detach()
            if u.dtype != torch.float32 or not u.is_contiguous():
                u = u.float().contiguous()
            kept.append(u)
            return ops._ptr(u, "tensor")
        b.mu, b.rho = dptr(P["weight_mu"]), dptr(P["weight_rho"])
        b.bias_mu, b.bias_rho, b.bias_a, b.bias_b = dptr(P["bias_mu"]), dptr(P["bias_rho"]), dptr(P["bias_a"]), dptr(P["bias_b"])
        b.tau_b, b.tau_w = dptr(tau_b), dptr(tau_w)
        b.weight_a, b.weight_b, b.pa, b.pb = dptr(P["weight_a"]), dptr(P["weight_b"]), dptr(P["pa"]), dptr(P["pb"])
        b.dW, b.g_sum = dW.data_ptr(), g_sum.data_ptr()
        b.g_lp = dptr(g_lp.reshape(1)) if g_lp is not None else None
        b.g_lq = dptr(g_lq.reshape(1)) if g_lq is not None else None
        d_mu, d_rho, d_lam = (torch.empty((O, I), **f) for _ in range(3))
        w_out = torch.empty((O, I), **f) if want_gx else None
        vecs = {n: torch.empty(O, **f) for n in ("d_bias_mu", "d_bias_rho", "d_bias_a", "d_bias_b")}
        scal, rows = torch.empty(5, **f), torch.empty(3 * O, **f)
        b.d_mu, b.d_rho = d_mu.data_ptr(), d_rho.data_ptr()
        b.w_out = w_out.data_ptr() if w_out is not None else None
        for n, t in vecs.items():
            setattr(b, n, t.data_ptr())
        b.d_scalars, b.rows = scal.data_ptr(), rows.data_ptr()
        b.O, b.I, b.exact, b.layer_id = O, I, keep["exact"], layer._layer_id
        a.lambdal, a.d_lambdal, a.temperature = dptr(P["lambdal"]), d_lam.data_ptr(), keep["T"]
        _lib.check(_lib.lib().lbbnn_gate_backward_draw(ctypes.byref(a), ctx.rng.data_ptr(), ops._stream()),
                   "lbbnn_gate_backward_draw")
        del kept
        gx = _hip_matmul_nt(gm, ops.transpose_operand, w_out) if want_gx else None   # G W
        grads = {"weight_mu": d_mu, "weight_rho": d_rho, "weight_a": scal[0:1], "weight_b": scal[1:2], "lambdal": d_lam,
                 "pa": scal[3:4], "pb": scal[4:5], "bias_mu": vecs["d_bias_mu"], "bias_rho": vecs["d_bias_rho"],
                 "bias_a": vecs["d_bias_a"], "bias_b": vecs["d_bias_b"]}
        return (None, gx, None, None, None, *[grads[n] for n in layer._names])


class BayesianLinear(nn.Module):
    _names = ("weight_mu", "weight_rho", "weight_a", "weight_b", "lambdal", "pa", "pb",
              "bias_mu", "bias_rho", "bias_a", "bias_b")

    def __init__(self, in_features, out_features, layer_id, *, weight_mu_init=(-0.2, 0.2), lambdal_init=(0, 1)):
        """``weight_mu_init`` / ``lambdal_init``: the uniform ranges of the two initial draws that differ between the scripts
        (LBBNN-GP-MF.py:192,201: the defaults; LBBNN-GP-MFsim_study.py:182,190: (-0.01, 0.01) and (-0.5, 0.5))."""
        super().__init__()
        self.layer = layer_id
        self.in_features, self.out_features = in_features, out_features
        O, I = out_features, in_features
        # creation order == LBBNN-GP-MF.py:192-219 (seeded construction reproduces the reference's values)
        self.weight_mu = nn.Parameter(torch.Tensor(O, I).uniform_(*weight_mu_init))
        self.weight_rho = nn.Parameter(torch.Tensor(O, I).uniform_(-5, -4))
        self.weight = Gaussian(self.weight_mu, self.weight_rho)
        self.weight_a = nn.Parameter(torch.Tensor(1).uniform_(1, 1.1))
        self.weight_b = nn.Parameter(torch.Tensor(1).uniform_(1, 1.1))
        self.weight_prior = GaussGamma(self.weight_a, self.weight_b)
        self.lambdal = nn.Parameter(torch.Tensor(O, I).uniform_(*lambdal_init))
        self.gammas = torch.Tensor(O, I).uniform_(0.99, 1)
        self.alpha = torch.Tensor(O, I).uniform_(0.999, 0.9999)
        self.gamma = Bernoulli(self.alpha, exact=False)
        self.pa = nn.Parameter(torch.Tensor(1).uniform_(1, 1.1))
        self.pb = nn.Parameter(torch.Tensor(1).uniform_(1, 1.1))
        self.gamma_prior = BetaBinomial(pa=self.pa, pb=self.pb)
        self.bias_mu = nn.Parameter(torch.Tensor(O).uniform_(-0.2, 0.2))
        self.bias_rho = nn.Parameter(torch.Tensor(O).uniform_(-5, -4))
        self.bias = Gaussian(self.bias_mu, self.bias_rho)
        self.bias_a = nn.Parameter(torch.Tensor(O).uniform_(1, 1.1))
        self.bias_b = nn.Parameter(torch.Tensor(O).uniform_(1, 1.1))
        self.bias_prior = GaussGamma(self.bias_a, self.bias_b)
        self.log_prior = 0
        self.log_variational_posterior = 0
        self.lagrangian = 0
        self.noise = None              # parity tests: {"eps_w","eps_b","tau_w","tau_b"}
        self._layer_id = next(_ids) % 64
        self._ws = None

    def _workspace(self):
        dev = self.weight_mu.device
        if self._ws is None or self._ws["dev"] != dev:
            O, ld = self.out_features, ops.operand_ld(self.in_features)
            f = dict(dtype=torch.float32, device=dev)
            self._ws = {"dev": dev, "w": torch.empty((O, ld), **f), "rows": torch.empty(4 * O, **f)}
        return self._ws

    def _exact_bits(self):
        return ((1 if self.weight_prior.exact else 0) | (2 if self.bias_prior.exact else 0)
                | (4 if self.gamma_prior.exact else 0) | (8 if self.gamma.exact else 0))

    def _forward_hip(self, x, cgamma, tau_w, tau_b, cfg, save_rng=False):
        mode, want_lp, exact = cfg
        ws = self._workspace()
        dev = x.device
        noise = self.noise or {}
        O, I = self.out_features, self.in_features
        split = (ops.split_precision() and ops.split_eligible(I, O)
                 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)
        a = _lib.GateArgs()
        P = lambda t: None if t is None else ops._ptr(t.detach() if t.requires_grad else t, "tensor")
        gamma_alpha = self.gamma.alpha
        gamma_alpha = gamma_alpha.detach().to(dev).float().contiguous() if torch.is_tensor(gamma_alpha) else None
        alpha_attr = self.alpha.detach().to(dev).float().contiguous() if torch.is_tensor(self.alpha) else None
        cg = None if cgamma is None else cgamma.detach().to(dev).float().contiguous()
        eps_w, eps_b = noise.get("eps_w"), noise.get("eps_b")
        rng, st, saved = None, None, {"noise": self.noise, "alpha_attr": alpha_attr, "gamma_alpha": gamma_alpha}
        if mode == 0 and (eps_w is None or eps_b is None):
            st = ops.RngState.get(dev)
            rng = st.t
            saved["rng"] = rng.clone() if save_rng else None
        bias = torch.empty(O, dtype=torch.float32, device=dev)
        lp = torch.empty((), dtype=torch.float32, device=dev) if want_lp else None
        lq = torch.empty((), dtype=torch.float32, device=dev) if want_lp else None
        a.mu, a.rho, a.gamma_alpha, a.cgamma = P(self.weight_mu), P(self.weight_rho), P(gamma_alpha), P(cg)
        a.eps_w, a.alpha_attr = P(eps_w), P(alpha_attr)
        a.bias_mu, a.bias_rho, a.eps_b = P(self.bias_mu), P(self.bias_rho), P(eps_b)
        a.bias_a, a.bias_b, a.tau_b = P(self.bias_a), P(self.bias_b), P(tau_b)
        a.weight_a, a.weight_b, a.tau_w, a.pa, a.pb = P(self.weight_a), P(self.weight_b), P(tau_w), P(self.pa), P(self.pb)
        a.w_out, a.bias_out, a.rows = ws["w"].data_ptr(), bias.data_ptr(), ws["rows"].data_ptr()
        a.log_prior, a.log_q = P(lp), P(lq)
        a.O, a.I, a.ld, a.mode, a.exact, a.want_lp = O, I, ops.operand_ld(I), mode, exact, int(want_lp)
        a.flags, a.layer_id = (ops.F_SPLIT16 if split else 0), self._layer_id
        _lib.check(_lib.lib().lbbnn_gate_sample(ctypes.byref(a), rng.data_ptr() if rng is not None else None,
                                                ops._stream()), "lbbnn_gate_sample")
        out = ops.lrt_gemm(x, ws["w"], None, I=I, O=O, bias_mean=bias, mean_only=True, split=split)   # F.linear :255
        if st is not None:
            st.advance(1)
        saved["cg"] = cg
        return out, lp, lq, saved

    def _forward_hip_draws(self, x, rng, act, slot=None):
        """lbbnn_gate_sample_draw + the mean-only GEMM (act: None, "relu" or "log_softmax" in its epilogue).  Returns out,
        lp, lq and the kernel-written buffers; every draw comes from the Philox state ``rng`` (2 int64 words on the device).
        ``slot``: the two 0-dim fp32 device tensors the kernel writes log_prior and log_q into (a network deeper than three
        layers passes slots of its [2][n] buffer); default: fresh ones."""
        from . import distributions
        ws = self._workspace()
        dev = x.device
        O, I = self.out_features, self.in_features
        split = (ops.split_precision() and ops.split_eligible(I, O)
                 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)
        f = dict(dtype=torch.float32, device=dev)
        P = lambda t: ops._ptr(t.detach(), "tensor")
        keep = {"gammas": torch.empty((O, I), **f), "alpha": torch.empty((O, I), **f), "tau_w": torch.empty(1, **f),
                "tau_b": torch.empty(O, **f), "T": float(distributions.TEMPER_PRIOR), "exact": self._exact_bits()}
        bias = torch.empty(O, **f)
        lp, lq = slot if slot is not None else (torch.empty((), **f), torch.empty((), **f))
        a = _lib.GateDrawArgs()
        g = a.g
        g.mu, g.rho, g.bias_mu, g.bias_rho = P(self.weight_mu), P(self.weight_rho), P(self.bias_mu), P(self.bias_rho)
        g.bias_a, g.bias_b = P(self.bias_a), P(self.bias_b)
        g.weight_a, g.weight_b, g.pa, g.pb = P(self.weight_a), P(self.weight_b), P(self.pa), P(self.pb)
        g.w_out, g.bias_out, g.rows = ws["w"].data_ptr(), bias.data_ptr(), ws["rows"].data_ptr()
        g.log_prior, g.log_q = lp.data_ptr(), lq.data_ptr()
        g.O, g.I, g.ld, g.mode, g.exact, g.want_lp = O, I, ops.operand_ld(I), 0, keep["exact"], 1
        g.flags, g.layer_id = (ops.F_SPLIT16 if split else 0), self._layer_id
        a.lambdal = P(self.lambdal)
        a.gammas, a.alpha = keep["gammas"].data_ptr(), keep["alpha"].data_ptr()
        a.tau_w, a.tau_b, a.temperature = keep["tau_w"].data_ptr(), keep["tau_b"].data_ptr(), keep["T"]
        _lib.check(_lib.lib().lbbnn_gate_sample_draw(ctypes.byref(a), rng.data_ptr(), ops._stream()), "lbbnn_gate_sample_draw")
        self._last_keep = keep
        out = ops.lrt_gemm(x, ws["w"], None, I=I, O=O, bias_mean=bias, mean_only=True, split=split,
                           relu=(act == "relu"), log_softmax=(act == "log_softmax"))                       # F.linear :255
        return out, lp, lq, keep

    def sample_forward(self, input, *, activation=None, rng=None):
        """The training-mode forward (sample=True, with log-probabilities) of ``sample_elbo(draws="hip")`` for one layer: the
        gates, tau_w, tau_b and the weight / bias noise are drawn inside the HIP kernels from the layer's Philox state.
        ``activation``: None, "relu" or "log_softmax" (out_features <= 16), applied in the GEMM epilogue.  ``rng``: a
        {seed, offset} snapshot (2 int64 on the device) to draw from; default: the device's ``ops.RngState``, which this call
        then advances by one.  Sets ``gammas``, ``alpha``, ``gamma.alpha``, ``tau_w``, ``tau_b``, ``log_prior`` and
        ``log_variational_posterior`` (detached tensors the kernels wrote).  Returns (out, log_prior, log_q), autograd-visible."""
        if not input.is_cuda:
            raise RuntimeError("bnn_amd: forward needs a HIP device tensor (input is on %s); there is no CPU path"
                               % input.device)
        if activation not in (None, "relu", "log_softmax"):
            raise ValueError("bnn_amd: activation must be None, 'relu' or 'log_softmax', got %r" % (activation,))
        if activation == "log_softmax" and self.out_features > 16:
            raise ValueError("bnn_amd: the fused log_softmax needs out_features <= 16")
        if rng is None:
            st = ops.RngState.get(input.device)
            rng = st.t[:2].clone()
            st.advance(1)
        x = input.float()
        params = [getattr(self, n) for n in self._names]
        out, lp, lq = _BaseDrawFn.apply(self, x, rng, activation, None, *params)
        self._publish_draws(lp, lq)
        return out, lp, lq

    def _fill_member_desc(self, d, S, split, rows=False, keep_gates=False):
        """lbbnn_gate_member_desc_t of this layer for an S-member evaluation draw; returns the buffers it points to."""
        O, I, ld = self.out_features, self.in_features, ops.operand_ld(self.in_features)
        f = dict(dtype=torch.float32, device=self.weight_mu.device)
        P = lambda t: ops._ptr(t.detach(), "tensor")
        buf = {"w": torch.empty((S, O, ld), **f), "bias": torch.empty((S, O), **f),
               "rows": torch.empty((S, O), **f) if rows else None,
               "gates": torch.empty((S, O, I), **f) if keep_gates else None}
        d.mu, d.rho, d.lambdal = P(self.weight_mu), P(self.weight_rho), P(self.lambdal)
        d.bias_mu, d.bias_rho = P(self.bias_mu), P(self.bias_rho)
        d.w_out, d.bias_out = buf["w"].data_ptr(), buf["bias"].data_ptr()
        d.gate_rows = buf["rows"].data_ptr() if rows else None
        d.gates = buf["gates"].data_ptr() if keep_gates else None
        d.O, d.I, d.ld, d.flags, d.exact = O, I, ld, (ops.F_SPLIT16 if split else 0), self._exact_bits()
        d.layer_id = self._layer_id
        return buf

    def _publish_draws(self, lp, lq):
        keep = self._last_keep
        self.gammas, self.alpha, self.tau_w, self.tau_b = keep["gammas"], keep["alpha"], keep["tau_w"], keep["tau_b"]
        self.gamma.alpha = keep["alpha"]
        self.log_prior, self.log_variational_posterior = lp.detach(), lq.detach()

    def _mean_branch_autograd(self, x, cgamma, tau_w, tau_b, mode):
        """LBBNN-GP-MF.py:236-255 for the two deterministic branches, as autograd-visible torch ops (GPU tensors)."""
        alpha_attr = self.alpha.to(x.device) if torch.is_tensor(self.alpha) else self.alpha
        weight = cgamma * self.weight.mu if mode == 1 else alpha_attr * self.weight.mu           # :236-242
        bias = self.bias.mu
        alpha_new = 1 / (1 + torch.exp(-self.lambdal))                                             # :246
        lp = (self.weight_prior.log_prob(weight, cgamma, tau=tau_w) + self.bias_prior.log_prob(bias, torch.ones_like(bias), tau=tau_b)
              + self.gamma_prior.log_prob(cgamma, pa=self.pa, pb=self.pb))                         # :247-249
        galpha = self.gamma.alpha
        gm = Bernoulli(galpha.to(x.device) if torch.is_tensor(galpha) else galpha, exact=self.gamma.exact)
        lq = self.weight.full_log_prob(input=weight, gamma=cgamma) + gm.log_prob(cgamma) + self.bias.log_prob(bias)   # :250-251
        del alpha_new
        return F.linear(x, weight, bias), lp, lq                                                   # :255

    def _noise_for_backward(self, saved):
        n = dict(saved.get("noise") or {})
        if "eps_w" not in n and saved.get("rng") is not None:
            O, I, L = self.out_features, self.in_features, self._layer_id
            n["eps_w"] = ops.philox_normal(saved["rng"], ops.STREAM_EPS_W * 64 + L, O, I)
            n["eps_b"] = ops.philox_normal(saved["rng"], ops.STREAM_EPS_B * 64 + L, 0, O)
        return n

    def forward(self, input, cgamma, sample=False, medimean=False, calculate_log_probs=False):
        if not input.is_cuda:
            raise RuntimeError("bnn_amd: forward needs a HIP device tensor (input is on %s); there is no CPU path"
                               % input.device)
        if self.training or sample:
            self.gammas = cgamma                                      # :231
            mode = 0
        elif medimean:
            mode = 1
        else:
            mode = 2
        want_lp = bool(self.training or calculate_log_probs)
        noise = self.noise or {}
        dev = input.device
        tau_w = tau_b = None
        if want_lp:
            tau_w = noise["tau_w"] if "tau_w" in noise else self.weight_prior.rsample_tau()      # :141
            tau_b = noise["tau_b"] if "tau_b" in noise else self.bias_prior.rsample_tau()
        cfg = (mode, want_lp, self._exact_bits())
        x = input.float()
        params = [getattr(self, n) for n in self._names]
        needs = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        if needs and want_lp and mode == 0:
            galpha = self.gamma.alpha if torch.is_tensor(self.gamma.alpha) else torch.as_tensor(self.gamma.alpha)
            out, lp, lq = _BaseFn.apply(self, x, cgamma.to(dev), tau_w, tau_b, galpha.to(dev), cfg, *params)
        else:
            if needs and want_lp:
                # medimean / joint-mean branch with calculate_log_probs under autograd (LBBNN-GP-MF.py:236-251): not a path
                # the reference's train() differentiates (:331-337 samples), so it is composed from differentiable torch
                # ops on the GPU tensors (the helper objects' densities); every other combination runs the HIP pass
                out, lp, lq = self._mean_branch_autograd(x, cgamma.to(dev), tau_w, tau_b, mode)
                self.alpha = 1 / (1 + torch.exp(-self.lambdal))
                self.log_prior, self.log_variational_posterior = lp, lq
                return out
            out, lp, lq, _ = self._forward_hip(x, cgamma, tau_w, tau_b, cfg)
        if want_lp:
            self.alpha = 1 / (1 + torch.exp(-self.lambdal))           # :246
            self.log_prior, self.log_variational_posterior = lp, lq
        else:
            self.log_prior, self.log_variational_posterior = 0, 0     # :253
        return out


class _FoldTotalsFn(torch.autograd.Function):
    """log_prior and log_q of a network of more than three layers: the layers' kernels wrote their values into the slots of one
    [2][n] buffer (the ``slot`` argument of ``_BaseDrawFn``), ONE lbbnn_fold_rows launch forms both totals as the fp32 left
    fold in layer order.  The
    backward hands every layer's node the upstream g_lp / g_lq tensor itself (lbbnn_gate_backward_draw reads it through a
    pointer): no expand and no add kernel at any depth."""

    @staticmethod
    def forward(ctx, buf, *vals):
        ctx.n = len(vals) // 2
        ctx.set_materialize_grads(False)
        tot = ops.fold_rows(buf, 2, ctx.n)
        return tot[0], tot[1]

    @staticmethod
    def backward(ctx, g_lp, g_lq):
        return (None,) + (g_lp,) * ctx.n + (g_lq,) * ctx.n


_NOT_GIVEN = object()     # forward's sample / medimean may arrive positionally after the gates: tells "not passed" from False


class BayesianNetwork(nn.Module):
    """LBBNN-GP-MF.py:259-319 (reference dims 784-400-600-10; ``dims=`` added): an MLP of 1 to MAX_DEPTH layers l1 .. lN
    (``2 <= len(dims) <= MAX_DEPTH + 1``), ReLU between them, log_softmax after the last.  Layer i draws from the Philox streams
    ``kind * 64 + 32 + i``.

    ``head="sigmoid"`` (LBBNN-GP-MFsim_study.py:259-262, with ``dims=(20, 1), weight_mu_init=(-0.01, 0.01),
    lambdal_init=(-0.5, 0.5)``): the last layer's logits go through one lbbnn_binary_head launch, ``forward`` returns the (B,
    units <= 16) probabilities, ``sample_elbo`` takes the BCE loss and returns the script's five values, and the evaluation
    functions treat one unit as two classes (``bnn_amd.evaluate``)."""
    _logp2_now = False       # set by bnn_amd.evaluate around a forward: a sigmoid head (one unit) returns the 2-class log-probabilities
    _fold_totals = True      # False: log_prior / log_q of sample_elbo(draws="hip") by torch adds at every depth (as up to 3 layers)

    def __init__(self, dims=(28 * 28, 400, 600, 10), head="log_softmax", *, weight_mu_init=(-0.2, 0.2), lambdal_init=(0, 1)):
        super().__init__()
        dims = tuple(dims)
        if head not in ("log_softmax", "sigmoid"):
            raise ValueError("bnn_amd: head must be 'log_softmax' or 'sigmoid', got %r" % (head,))
        if head == "sigmoid" and dims[-1] > 16:
            raise ValueError("bnn_amd: a sigmoid head takes at most 16 output units, got dims[-1] = %d" % dims[-1])
        self.head = head
        if not 2 <= len(dims) <= MAX_DEPTH + 1:
            raise ValueError("bnn_amd: %s takes 1 to %d layers (len(dims) 2 to %d), got dims=%s"
                             % (type(self).__name__, MAX_DEPTH, MAX_DEPTH + 1, dims))
        self.dims = dims
        self._lnames = tuple("l%d" % (i + 1) for i in range(len(dims) - 1))
        for i, name in enumerate(self._lnames):
            setattr(self, name, BayesianLinear(dims[i], dims[i + 1], 1,      # the reference passes layer id 1 to all of them
                                               weight_mu_init=weight_mu_init, lambdal_init=lambdal_init))
        for i, l in enumerate(self._layers()):
            l._layer_id = 32 + i              # per-network Philox stream ids (not the process-wide counter)

    def _layers(self):
        m = self._modules
        return [m[k] for k in self._lnames]

    def _gates(self, gates, named):
        """The n gate tensors of one ``forward`` call, and what follows them positionally (``sample``, ``medimean``)."""
        n = len(self._lnames)
        if len(gates) > n + 2:
            raise TypeError("bnn_amd: forward of a %d-layer network takes %d gates and at most sample, medimean after them; got "
                            "%d positional arguments after x" % (n, n, len(gates)))
        gs = dict(("g%d" % (i + 1), g) for i, g in enumerate(gates[:n]))
        for k, v in named.items():
            if not (k[:1] == "g" and k[1:].isdigit() and str(int(k[1:])) == k[1:] and 1 <= int(k[1:]) <= n):
                raise TypeError("bnn_amd: forward got an unexpected keyword argument %r (a %d-layer network takes g1 .. g%d)"
                                % (k, n, n))
            if k in gs:
                raise TypeError("bnn_amd: forward got the gate %s twice" % k)
            gs[k] = v
        missing = [k for k in ("g%d" % (i + 1) for i in range(n)) if k not in gs]
        if missing:
            raise TypeError("bnn_amd: forward of a %d-layer network needs one gate (or None) per layer; missing %s"
                            % (n, ", ".join(missing)))
        return [gs["g%d" % (i + 1)] for i in range(n)], gates[n:]

    def forward(self, x, *gates, sample=_NOT_GIVEN, medimean=_NOT_GIVEN, **named):
        """``net(x, g1, ..., gN, sample=False, medimean=False)``: one gate tensor (or None) per layer, positionally or as
        ``g1=..., gN=...`` (or mixed); positional arguments after the N-th gate are ``sample`` and ``medimean``.  A wrong number
        of gates, a gate given twice, or ``sample`` / ``medimean`` given both positionally and by name: TypeError."""
        gs, rest = self._gates(gates, named)
        for k, name in enumerate(("sample", "medimean")[:len(rest)]):
            if (sample, medimean)[k] is not _NOT_GIVEN:
                raise TypeError("bnn_amd: forward got multiple values for argument %r" % name)
        sample = rest[0] if len(rest) > 0 else (False if sample is _NOT_GIVEN else sample)
        medimean = rest[1] if len(rest) > 1 else (False if medimean is _NOT_GIVEN else medimean)
        layers = self._layers()
        x = x.view(-1, self.dims[0])
        for l, g in zip(layers[:-1], gs[:-1]):
            x = F.relu(l.forward(x, g, sample, medimean))
        x = layers[-1].forward(x, gs[-1], sample, medimean)
        if self.head == "sigmoid":
            # the logits as the last GEMM left them, then one lbbnn_binary_head launch (LBBNN-GP-MFsim_study.py:261)
            from .layers import _SigmoidHeadFn
            if self._logp2_now:
                return ops.binary_head(x.detach(), log_probs=True, want_probs=False)
            return _SigmoidHeadFn.apply(x) if x.requires_grad else ops.binary_head(x)
        return F.log_softmax(x, dim=1)

    def inclusion_probabilities(self):
        """Per layer the posterior inclusion probabilities alpha = sigmoid(lambdal) as detached (O, I) tensors on the
        parameters' device: the simulation study's result."""
        return [torch.sigmoid(l.lambdal.detach()) for l in self._layers()]

    def log_prior(self):
        layers = self._layers()
        t = layers[0].log_prior
        for l in layers[1:]:
            t = t + l.log_prior
        return t

    @torch.no_grad()
    def sample_predict(self, x, *, gates="sample", rng=None, log_probs=False):
        """One stochastic evaluation forward (test_ensemble's ``net.forward(data, sample=True, g1=gamma.rsample(), ...)``,
        LBBNN-GP-MF.py:388-389, without log-probabilities): (B, classes) log-probabilities, no autograd.  Every draw comes from
        the Philox state inside the HIP kernels -- lbbnn_gate_members (gates, weight and bias noise of all layers) and one
        mean-only GEMM per layer with ReLU or the head's log_softmax in its epilogue -- so this is member 0 of a one-member ensemble
        (``evaluate.ensemble_forward``).  ``gates``: "sample" (the training draw: the hard gate u < alpha when ``gamma.exact``
        is set, else the relaxed gate at ``distributions.TEMPER_PRIOR``; both read at call time) or "mpm" (the median
        probability model, gates alpha > 0.5 and sampled weights: outofsample(medimod=True), :469-473).  ``rng``: a
        {seed, offset} snapshot (2 int64 on the device) to draw from; default: the device's ``ops.RngState``, which this call
        then advances by one.  The draws match the reference in distribution, not in numbers.  A sigmoid head: (B, units)
        probabilities, or with ``log_probs`` (one unit) the (B, 2) log-probabilities of the two classes."""
        if not x.is_cuda:
            raise RuntimeError("bnn_amd: sample_predict needs a HIP device tensor (input is on %s); there is no CPU path"
                               % x.device)
        st = None
        if rng is None:
            st = ops.RngState.get(x.device)
            rng = st.t
        out = self._predict_members(x, rng, 1, gates, log_probs=log_probs)[0][0]
        if st is not None:
            st.advance(1)
        return out

    def _predict_members(self, input, rng, S, gates="sample", out=None, rows=False, keep_gates=False, log_probs=False):
        """S evaluation forwards of one batch; member m draws from {rng[0], rng[1] + m}, bitwise what ``sample_forward`` of the
        layers at that offset computes.  ceil(n / 4) + n launches: lbbnn_gate_members per group of _lib.MAX_LAYERS consecutive
        layers (every group reads the same ``rng``, member count and advance), then lbbnn_gemm_members_mean per layer.
        ``out``: optional (S, >= B*classes) buffer for the head.  Returns ((S, B, classes) log-probabilities, per-layer (S, O)
        gate row sums or None, per-layer (S, O, I) gates or None).  Does not advance the live state.  A sigmoid head: the last
        GEMM leaves the logits, then ONE lbbnn_binary_head launch over the members' buffer: (S, B, units) probabilities (in
        ``out`` when given), or with ``log_probs`` (one unit) the (S, B, 2) log-probabilities, a tensor of its own."""
        from . import evaluate
        evaluate._check_log_probs(self, log_probs)
        if not input.is_cuda:
            raise RuntimeError("bnn_amd: sample_predict needs a HIP device tensor (input is on %s); there is no CPU path"
                               % input.device)
        if gates not in ("sample", "mpm"):
            raise ValueError("bnn_amd: gates must be 'sample' or 'mpm', got %r" % (gates,))
        layers = self._layers()
        n = len(layers)
        for l in layers:
            if l.noise:
                raise ValueError("bnn_amd: evaluation draws its own noise in-kernel; injected draws (layer.noise) belong to the "
                                 "torch-draw forward -- clear layer.noise first")
        if any(ops.operand_ld(l.in_features) > ops.GATE_MEMBERS_MAX_LD for l in layers):
            return self._predict_members_loop(input, rng, S, gates, out, rows, keep_gates, log_probs)
        from . import distributions
        x = input.view(-1, self.dims[0]).float()
        if x.stride(1) != 1 or x.stride(0) < self.dims[0]:
            x = x.contiguous()
        B, dev = x.shape[0], x.device
        f = dict(dtype=torch.float32, device=dev)
        # operand format per layer: the rule of _forward_hip_draws (16-bit precisions take the bf16 hi|lo operands where the
        # split kernel accepts the shape and the input rows are 16-B aligned; a hidden layer's input rows are the previous
        # layer's output rows, aligned exactly when its width is a multiple of 4)
        splits = []
        for k, l in enumerate(layers):
            in_ok = (x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0) if k == 0 else layers[k - 1].out_features % 4 == 0
            splits.append(bool(ops.split_precision() and ops.split_eligible(l.in_features, l.out_features) and in_ok))
        descs = (_lib.GateMemberDesc * n)()
        bufs = [l._fill_member_desc(descs[k], S, splits[k], rows, keep_gates) for k, l in enumerate(layers)]
        stream = ops._stream()
        mode, T = (ops.GATES_MPM if gates == "mpm" else ops.GATES_SAMPLE), float(distributions.TEMPER_PRIOR)
        for k, cnt in _lib.layer_groups(n):                    # every group reads the same offset; the caller advances once
            _lib.check(_lib.lib().lbbnn_gate_members(_lib.group_slice(descs, k, cnt), cnt, S, mode, T, rng.data_ptr(), 1, stream),
                       "lbbnn_gate_members")
        C = self.dims[-1]
        if out is None:
            out = torch.empty((S, ops.pad4(B * C)), **f)
        elif out.dim() != 2 or out.shape[0] != S or out.shape[1] < B * C or out.stride(0) % 4 or not out.is_contiguous():
            raise RuntimeError("bnn_amd: out must be a contiguous (S, >= B*classes) buffer with 16-B aligned rows")
        ops.member_gemm_chain(x, S, [(b["w"], b["bias"], s) for b, s in zip(bufs, splits)], head=self.head, out=out,
                              stream=stream)
        res = evaluate._members_result(out, S, B, C, self.head, log_probs)
        for l in layers:
            l.log_prior, l.log_variational_posterior = 0, 0          # an evaluation forward keeps no log-probabilities (:253)
        return (res, [b["rows"] for b in bufs] if rows else None, [b["gates"] for b in bufs] if keep_gates else None)

    def _predict_members_loop(self, input, rng, S, gates, out, rows, keep_gates, log_probs=False):
        """``_predict_members`` for a network with a layer wider than lbbnn_gate_members takes (operand_ld(in_features) >
        ops.GATE_MEMBERS_MAX_LD): member m is the chain of the layers' ``sample_forward`` at {rng[0], rng[1] + m} -- by
        definition what the batched form computes -- and its gates / gate row sums are the ones that chain drew.  n layer
        calls per member; the layers keep the last member's draws, as after ``sample_forward``.  The median probability model
        has no training-kernel chain: gates="mpm" raises.  A sigmoid head: the chains leave their logits in one (S, member stride)
        buffer (``out`` when given), then the one lbbnn_binary_head launch of the batched form."""
        if gates != "sample":
            raise ValueError("bnn_amd: gates='mpm' needs every layer within lbbnn_gate_members' width (operand_ld(in_features) "
                             "<= %d)" % ops.GATE_MEMBERS_MAX_LD)
        layers = self._layers()
        n = len(layers)
        C = self.dims[-1]
        sigmoid = self.head == "sigmoid"
        head = "log_softmax" if C <= 16 and not sigmoid else None
        x = input.view(-1, self.dims[0]).float()
        if x.stride(1) != 1 or x.stride(0) < self.dims[0]:
            x = x.contiguous()
        B = x.shape[0]
        if sigmoid:
            # (the chains write their logits into ``out`` itself and the head goes over it as one block: looked at first)
            if out is not None and (out.dim() != 2 or out.shape[0] != S or out.shape[1] < B * C or not out.is_contiguous()):
                raise RuntimeError("bnn_amd: out must be a contiguous (S, >= B*classes) buffer")
            logits = out if out is not None else torch.empty((S, ops.pad4(B * C)), dtype=torch.float32, device=x.device)
        else:
            res = torch.empty((S, B, C), dtype=torch.float32, device=x.device)
        g_rows = [torch.empty((S, l.out_features), dtype=torch.float32, device=x.device) for l in layers] if rows else None
        g_all = [torch.empty((S, l.out_features, l.in_features), dtype=torch.float32, device=x.device)
                 for l in layers] if keep_gates else None
        for m in range(S):
            r = rng[:2].clone()
            r[1] += m
            h = x
            for k, l in enumerate(layers):
                h, _, _ = l.sample_forward(h, activation="relu" if k < n - 1 else head, rng=r)
                if rows:
                    g_rows[k][m] = l.gammas.sum(1)
                if keep_gates:
                    g_all[k][m] = l.gammas
            if sigmoid:
                logits[m, :B * C].copy_(h.reshape(-1))
            else:
                res[m] = h if head else F.log_softmax(h, dim=1)
        if sigmoid:
            from . import evaluate
            res = evaluate._binary_members(logits, S, B, C, log_probs)
        elif out is not None:
            if out.dim() != 2 or out.shape[0] != S or out.shape[1] < B * C:
                raise RuntimeError("bnn_amd: out must be a (S, >= B*classes) buffer")
            out[:, :B * C].copy_(res.view(S, B * C))
        for l in layers:
            l.log_prior, l.log_variational_posterior = 0, 0          # an evaluation forward keeps no log-probabilities (:253)
        return res, g_rows, g_all

    def log_variational_posterior(self):
        layers = self._layers()
        t = layers[0].log_variational_posterior
        for l in layers[1:]:
            t = t + l.log_variational_posterior
        return t

    def sample_elbo(self, input, target, samples=SAMPLES, *, num_batches=None, draws="torch", stats=None, monitor=None):
        """:285-319, same positional arguments.  NUM_BATCHES / SAMPLES are module globals there (:34-67) and here
        (``bnn_amd.base.NUM_BATCHES = 600``, ``SAMPLES = 1``); ``num_batches=`` overrides the former per call.
        ``draws``: "torch" (default) draws the gates and the Gamma precisions with torch.distributions, as the reference;
        "hip" draws every stochastic input of the step inside the HIP kernels from the Philox state (``ops.RngState``,
        reseeded by ``torch.manual_seed``), reads nothing back to the host, and can be captured
        (``graphs.make_graphed_train_step``).  The two agree in distribution, not bit for bit.
        A sigmoid head (LBBNN-GP-MFsim_study.py:275-302): ``target`` is float32 (B,) or (B, units) (an integer 0 / 1 target is
        converted with ``.float()``), the likelihood term is ``losses.elbo_bce_loss`` (nn.BCELoss(reduction='sum'), fused), and the
        return has the script's five values (loss, log_prior, log_q, nll, out) with ``out`` the mean of the samples'
        probabilities (for one sample the tensor itself).  ``stats``: the int32[4] device tensor ``elbo_bce_loss`` adds its counts
        to (training accuracy with one read per epoch); sigmoid head only.
        ``monitor``: a ``losses.TrainMonitor`` (``dims[-1]`` classes / units) that records the step and holds the guard word
        for ``optimizer.set_guard``; both heads, both ``draws`` modes, ``samples == 1`` only (one monitored step is one loss
        launch) and HIP tensors only.  The step's loss is then ONE fused launch, ``losses.elbo_loss(out, target, log_q -
        log_prior, num_batches, monitor=monitor)`` (``elbo_bce_loss`` for a sigmoid head), in place of the nll launch and the
        torch expression ``nll + (log_q - log_prior) / num_batches``; the returned ``nll`` is ``(loss - (log_q - log_prior) /
        num_batches).detach()`` (the reference only prints it).  The fused loss rounds ONCE, from fp64, so it equals the
        unfused one to fp32 rounding, not bit for bit; likewise the gradients of ``log_prior`` and ``log_q``: g * (1 / N)
        against g / N.  ``log_prior`` and ``log_q`` themselves are the same bits.  Without a monitor nothing changes.  The guard
        catches a loss that is not finite -- e.g. an invalid ``a``, ``b``, ``pa``, ``pb`` whose draw or density comes out NaN or
        inf -- not an invalid parameter whose loss stays finite (VALIDATE_ARGS)."""
        if draws not in ("torch", "hip"):
            raise ValueError("bnn_amd: sample_elbo(draws=...) must be 'torch' or 'hip', got %r" % (draws,))
        if num_batches is None:
            num_batches = NUM_BATCHES
        sigmoid = self.head == "sigmoid"
        if stats is not None and not sigmoid:
            raise ValueError("bnn_amd: sample_elbo(stats=...) belongs to the BCE loss of a head=\"sigmoid\" network")
        if sigmoid:
            from .losses import elbo_bce_loss
            target = target if target.dtype == torch.float32 else target.float()
        if monitor is not None:
            from .losses import TrainMonitor
            who = "bnn_amd: sample_elbo(monitor=...): "
            if not isinstance(monitor, TrainMonitor):
                raise ValueError(who + "monitor must be a bnn_amd.TrainMonitor, got %s" % type(monitor).__name__)
            if samples != 1:
                raise ValueError(who + "one monitored step is one loss launch: samples must be 1, got %d" % samples)
            if draws == "torch" and not input.is_cuda:
                raise ValueError(who + "the monitor lives in the fused HIP loss; input is on %s" % input.device)
        if draws == "hip":
            return self._sample_elbo_hip(input, target, samples, num_batches, stats, monitor)
        dev = input.device
        lps, lqs, nlls, outs = [], [], [], []
        for _ in range(samples):
            gs = []
            for l in self._layers():
                l.alpha = 1 / (1 + torch.exp(-l.lambdal))             # :292-297
                l.gamma.alpha = l.alpha
                gs.append(l.gamma.rsample().to(dev))                  # :300-302
            out = self.forward(input, *gs, sample=True, medimean=False)
            lps.append(self.log_prior())
            lqs.append(self.log_variational_posterior())
            if monitor is not None:
                return self._monitored_elbo(out, target, lps[0], lqs[0], num_batches, stats, monitor)
            if sigmoid:
                nlls.append(elbo_bce_loss(out, target, stats=stats))  # sim study :292-296
                outs.append(out)
            else:
                nlls.append(F.nll_loss(out, target, reduction="sum"))
        log_prior = torch.stack(lps).mean()
        log_q = torch.stack(lqs).mean()
        nll = torch.stack(nlls).mean()
        loss = nll + (log_q - log_prior) / num_batches                # :318
        if sigmoid:
            return loss, log_prior, log_q, nll, (outs[0] if samples == 1 else torch.stack(outs).mean(0))
        return loss, log_prior, log_q, nll

    def _monitored_elbo(self, out, target, log_prior, log_q, num_batches, stats, monitor):
        """The tail of a monitored step (samples == 1): the whole ELBO in the one fused loss launch that records it."""
        from .losses import elbo_bce_loss, elbo_loss
        kl = log_q - log_prior
        if self.head == "sigmoid":
            loss = elbo_bce_loss(out, target, kl, num_batches, stats=stats, monitor=monitor)
            return loss, log_prior, log_q, loss.detach() - kl.detach() / num_batches, out
        loss = elbo_loss(out, target, kl, num_batches, monitor=monitor)
        return loss, log_prior, log_q, loss.detach() - kl.detach() / num_batches

    def _sample_elbo_hip(self, input, target, samples, num_batches, stats=None, monitor=None):
        """sample_elbo(draws="hip"): per sample one Philox snapshot (the offset advances once), one _BaseDrawFn node per
        layer with ReLU / log_softmax in the GEMM epilogues, the NLL as one launch (losses.elbo_loss).  log_prior and log_q:
        up to three layers the chain of torch adds; deeper, one lbbnn_fold_rows launch over the slots the layers' kernels
        wrote (_FoldTotalsFn) -- the same fp32 left fold.  A sigmoid head: the last node runs without an activation, then the
        head node (layers._SigmoidHeadFn) and the BCE loss (losses.elbo_bce_loss), whose backward hands the head the logits
        gradient."""
        from .layers import _SigmoidHeadFn
        from .losses import elbo_bce_loss, elbo_loss
        if not input.is_cuda:
            raise RuntimeError("bnn_amd: sample_elbo(draws='hip') needs a HIP device tensor (input is on %s); there is no "
                               "CPU path" % input.device)
        x = input.view(-1, self.dims[0]).float()
        st = ops.RngState.get(input.device)
        layers = self._layers()
        n = len(layers)
        sigmoid = self.head == "sigmoid"
        head = "log_softmax" if self.dims[-1] <= 16 and not sigmoid else None
        fold = bool(self._fold_totals and n > 3)
        lps, lqs, nlls, outs = [], [], [], []
        for _ in range(samples):
            rng = st.t[:2].clone()
            st.advance(1)
            h, lp, lq = x, None, None
            buf = torch.empty((2, n), dtype=torch.float32, device=x.device) if fold else None
            vals = ([], [])
            for k, l in enumerate(layers):
                slot = (buf[0, k], buf[1, k]) if fold else None       # where this layer's kernel writes (log_prior, log_q)
                h, lp_l, lq_l = _BaseDrawFn.apply(l, h, rng, "relu" if k < n - 1 else head, slot,
                                                  *[getattr(l, n_) for n_ in l._names])
                l._publish_draws(lp_l, lq_l)
                if fold:
                    vals[0].append(lp_l)
                    vals[1].append(lq_l)
                else:
                    lp = lp_l if lp is None else lp + lp_l
                    lq = lq_l if lq is None else lq + lq_l
            if fold:
                lp, lq = _FoldTotalsFn.apply(buf, *vals[0], *vals[1])
            if sigmoid:
                h = _SigmoidHeadFn.apply(h)
                outs.append(h)
            elif head is None:
                h = F.log_softmax(h, dim=1)
            lps.append(lp)
            lqs.append(lq)
            if monitor is not None:
                return self._monitored_elbo(h, target, lp, lq, num_batches, stats, monitor)
            nlls.append(elbo_bce_loss(h, target, stats=stats) if sigmoid else elbo_loss(h, target))
        if samples == 1:
            log_prior, log_q, nll = lps[0], lqs[0], nlls[0]
        else:
            log_prior, log_q, nll = torch.stack(lps).mean(), torch.stack(lqs).mean(), torch.stack(nlls).mean()
        loss = nll + (log_q - log_prior) / num_batches                # :318
        if sigmoid:
            return loss, log_prior, log_q, nll, (outs[0] if samples == 1 else torch.stack(outs).mean(0))
        return loss, log_prior, log_q, nll
