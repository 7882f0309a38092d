"""Tensor-level wrappers over the C ABI (include/lbbnn.h).

Every function takes torch tensors that must already live on a HIP device (contiguous fp32),
enqueues on torch's current stream and returns without synchronising.  Nothing here computes
on the host; a CPU tensor or a missing library raises.
"""
import ctypes
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import Priors

F_RELU = 0x1
F_MEAN_ONLY = 0x2
F_SPLIT16 = 0x4
F_LOG_SOFTMAX = 0x8
F_SINGLE16 = 0x10
F_HALF16 = 0x20
F_F16S = 0x40
F_VAR1 = 0x80
F_XPLANES = 0x100

STREAM_EPS_OUT = 0
STREAM_EPS_Z = 1
STREAM_EPS_Z2 = 2
STREAM_EPS_ACT = 3
STREAM_EPS_W = 4
STREAM_EPS_B = 5
STREAM_MASK = 6
STREAM_ROW_MASK = 7
STREAM_GATE = 8          # the baseline layer's in-kernel draws (sample_elbo(draws="hip")): gate uniforms, tau_w, tau_b
STREAM_GAMMA_W = 9
STREAM_GAMMA_B = 10
GATES_SAMPLE = 0         # lbbnn_gate_members: gates drawn as in training; the median probability model (alpha > 0.5)
GATES_MPM = 1
GATE_MEMBERS_MAX_LD = 4096  # widest operand row lbbnn_gate_members takes (kGmMaxLd); wider layers: BayesianNetwork's member loop


# GEMM arithmetic.  A name selects the operand FORMAT of the forward's dual-moment GEMM:
#   "fp32"     exact fp32 MFMA (v_mfma_f32_16x16x4_f32): the reference's own precision
#   "fp16x3"   row-scaled fp16 hi + lo operands, 3 + 3 products (LBBNN_F_F16S): 2-3e-8 of max|out| against fp64 -- tighter than an
#              fp32-accumulate torch.mm; the contract-grade 16-bit mode
#   "fp16x3f"  the same operands, ONE product for the variance GEMM (LBBNN_F_VAR1, 3 + 1): 1.4-1.8e-5 (contract 1e-4), 4 MFMAs
#              per tile step instead of 6; x^2 from the fp16 planes by packed fp16 math
#   "bf16x3"   bf16 hi + lo operands, 3 + 3 products (round 1-2 headline): 2.7e-6
#   "bf16" / "fp16"   ONE product per moment: reduced-precision modes OUTSIDE the contract (2e-3 / 3e-4), own tolerances
# The backward products and every mean-only product stay on the bf16x3 kernels whatever 16-bit mode is chosen.
# The process-wide default below applies to every module that has no ``precision`` attribute of its own:
# ``net.set_precision(name)`` (layers._NetworkBase) / ``layer.precision = name`` select per network / per layer.
PRECISIONS = ("fp32", "bf16x3", "bf16", "fp16", "fp16x3", "fp16x3f")
_PRECISION = "fp32"


def set_precision(name: str):
    """Process-wide DEFAULT precision (modules with their own ``precision`` attribute ignore it)."""
    global _PRECISION
    if name not in PRECISIONS:
        raise ValueError("precision must be one of %s" % (PRECISIONS,))
    _PRECISION = name


def get_precision(module=None) -> str:
    """The precision in force for ``module`` (its own ``precision`` attribute if set, else the process default)."""
    own = getattr(module, "precision", None) if module is not None else None
    if own is not None:
        if own not in PRECISIONS:
            raise ValueError("precision must be one of %s" % (PRECISIONS,))
        return own
    return _PRECISION


def split_precision(module=None) -> bool:
    """Do the GEMMs of ``module`` take 16-bit operand planes (every mode but "fp32")?"""
    return get_precision(module) != "fp32"


def f16s_precision(module=None) -> bool:
    return get_precision(module) in ("fp16x3", "fp16x3f")


def split_eligible(I: int, O: int) -> bool:
    """Shapes the split-precision kernels accept (see lbbnn_lrt_gemm, LBBNN_F_SPLIT16); operands and x must also stay
    under 2 GiB each (32-bit buffer offsets), which the callers' batch sizes do by orders of magnitude."""
    return O > 16 and I % 8 == 0 and (I % 32 == 0 or operand_ld(I) - I >= 8) and O * operand_ld(I) * 4 < 0x7FFFFFF0


F16_VAR1_MIN_I = 256          # "fp16x3f": rows shorter than this keep three variance products (layers._split)


def f16s_eligible(I: int, O: int) -> bool:
    """Shapes the row-scaled fp16 format takes: what the split kernels take, and rows of at most 1280 weights (the weight
    pass scales a row by its maximum, which it holds in registers: weight_pass.hip)."""
    return split_eligible(I, O) and operand_ld(I) <= 1280


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor], name: str = "tensor") -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("bnn_amd: %s is on %s; the HIP path needs a GPU tensor (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float32 and t.dtype != torch.int64:
        raise RuntimeError("bnn_amd: %s has dtype %s, expected float32" % (name, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError("bnn_amd: %s must be contiguous" % name)
    return t.data_ptr()


def _ptr_rows(t: torch.Tensor, name: str) -> int:
    """Pointer of a 2-D fp32 GPU tensor whose rows are dense (stride(1) == 1); row stride is free."""
    if not t.is_cuda:
        raise RuntimeError("bnn_amd: %s is on %s; the HIP path needs a GPU tensor (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError("bnn_amd: %s must be a 2-D float32 tensor with dense rows" % name)
    return t.data_ptr()


def operand_ld(I: int) -> int:
    return ((I + 31) // 32) * 32


# ----------------------------------------------------------------------------------------- RNG state
class RngState:
    """Per-device {seed, offset} pair in device memory, read by the kernels (graph-replay safe).

    The seed follows ``torch.initial_seed()`` (so ``torch.manual_seed(i)`` in a training script
    reseeds the in-kernel noise too); the offset is advanced on the device after every layer call.
    """
    _states = {}
    _requested = None          # (seed, offset) of the last manual_seed(): applies to states created afterwards too

    def __init__(self, device: torch.device):
        self.device = device
        self.seed = None
        # words 0-1: the live {seed, offset}; words 2-3: the copy a fused forward's later kernels read
        # (lbbnn_layers_operands_snap)
        self.t = torch.zeros(4, dtype=torch.int64, device=device)
        req = RngState._requested
        self.reseed(torch.initial_seed(), req[1] if (req is not None and req[0] == torch.initial_seed()) else 0)

    def reseed(self, seed: int, offset: int = 0):
        self.seed = int(seed)
        s = self.seed & 0xFFFFFFFFFFFFFFFF
        if s >= 1 << 63:
            s -= 1 << 64
        self.t[:2].copy_(torch.tensor([s, int(offset)], dtype=torch.int64))

    @classmethod
    def get(cls, device: torch.device) -> "RngState":
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        st = cls._states.get(key)
        if st is None:
            st = cls(device)
            cls._states[key] = st
        elif st.seed != torch.initial_seed() and not torch.cuda.is_current_stream_capturing():
            st.reseed(torch.initial_seed())
        return st

    def advance(self, delta: int = 1):
        _lib.check(_lib.lib().lbbnn_rng_advance(self.t.data_ptr(), delta, _stream()), "lbbnn_rng_advance")


def manual_seed(seed: int, offset: int = 0):
    """Reseed the in-kernel noise of every device that has a state (also done implicitly when
    ``torch.manual_seed`` changes ``torch.initial_seed()``)."""
    torch.manual_seed(seed)
    RngState._requested = (int(seed), int(offset))
    for st in RngState._states.values():
        st.reseed(seed, offset)


def philox_normal(rng: torch.Tensor, stream_id: int, rows: int, cols: int, row_base: int = 0) -> torch.Tensor:
    """The exact N(0,1) values the kernels draw (2-D if rows > 0, else 1-D of length cols)."""
    out = torch.empty((rows, cols) if rows > 0 else (cols,), dtype=torch.float32, device=rng.device)
    _lib.check(_lib.lib().lbbnn_philox_normal(rng.data_ptr(), stream_id, row_base, rows, cols, out.data_ptr(),
                                              _stream()), "lbbnn_philox_normal")
    return out


def philox_uniform(rng: torch.Tensor, stream_id: int, rows: int, cols: int, row_base: int = 0) -> torch.Tensor:
    """The exact uniforms of the baseline layer's in-kernel gate draw: (rows, cols), element (r, c) = counter (row_base + r,
    c // 4), word c % 4, as ((bits >> 8) + 0.5) 2^-24."""
    out = torch.empty((rows, cols), dtype=torch.float32, device=rng.device)
    _lib.check(_lib.lib().lbbnn_philox_uniform(rng.data_ptr(), stream_id, row_base, rows, cols, out.data_ptr(), _stream()),
               "lbbnn_philox_uniform")
    return out


def philox_std_gamma(rng: torch.Tensor, stream_id: int, a: torch.Tensor, rate: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The in-kernel Gamma draws: element i is Gamma(a[i]) from counter (i, attempt), divided by rate[i] (default 1) and
    clamped below at FLT_MIN (what the baseline layer's tau_w / tau_b are, element 0 / element o of their streams)."""
    a = a.detach().float().contiguous()
    rate = None if rate is None else rate.detach().float().contiguous()
    out = torch.empty_like(a)
    _lib.check(_lib.lib().lbbnn_philox_std_gamma(rng.data_ptr(), stream_id, a.data_ptr(), _ptr(rate, "rate"), a.numel(),
                                                 out.data_ptr(), _stream()), "lbbnn_philox_std_gamma")
    return out


def gamma_grad(x: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """The device's g(x, a) = -(dF(x; a)/da) / f(x; a) of the standard Gamma (the reparameterised dx/da)."""
    x = x.detach().float().contiguous()
    a = a.detach().float().contiguous()
    if x.shape != a.shape:
        raise ValueError("bnn_amd.ops.gamma_grad: x and a must have the same shape")
    out = torch.empty_like(x)
    _lib.check(_lib.lib().lbbnn_gamma_grad(x.data_ptr(), a.data_ptr(), x.numel(), out.data_ptr(), _stream()), "lbbnn_gamma_grad")
    return out


# ----------------------------------------------------------------------------------------- K1
def weight_pass(mu, rho, lambdal, *, z_fwd=None, z_kl=None, r0_c=None, bias_rho=None,
                priors: Priors, e_w=None, var_w=None, kl_rows=None, act_mu=None, act_var=None,
                bias_var=None, split=False, e_scale=None, v_scale=None):
    """lbbnn_weight_pass.  Output tensors are caller-allocated (see LayerWorkspace).  split: False / 0 fp32 operands,
    True / 1 bf16 hi | lo, 2 row-scaled fp16 hi | lo (lbbnn_weight_pass_f16: e_scale / v_scale (O) receive the row scales), 3 the same
    with var_w as plain fp16 rows (hi part only: the operands of the 3 + 1 product form)."""
    O, I = mu.shape
    ld = operand_ld(I)
    if int(split) >= 2:
        rc = _lib.lib().lbbnn_weight_pass_f16(
            _ptr(mu, "weight_mu"), _ptr(rho, "weight_rho"), _ptr(lambdal, "lambdal"),
            _ptr(z_fwd), _ptr(z_kl), _ptr(r0_c), _ptr(bias_rho), ctypes.byref(priors),
            _ptr(e_w), _ptr(var_w), ld, _ptr(e_scale, "e_scale"), _ptr(v_scale, "v_scale"),
            _ptr(kl_rows), _ptr(act_mu), _ptr(act_var), _ptr(bias_var), O, I, F_VAR1 if int(split) == 3 else 0, _stream())
        _lib.check(rc, "lbbnn_weight_pass_f16")
        return
    rc = _lib.lib().lbbnn_weight_pass(
        _ptr(mu, "weight_mu"), _ptr(rho, "weight_rho"), _ptr(lambdal, "lambdal"),
        _ptr(z_fwd), _ptr(z_kl), _ptr(r0_c), _ptr(bias_rho), ctypes.byref(priors),
        _ptr(e_w), _ptr(var_w), ld, _ptr(kl_rows), _ptr(act_mu), _ptr(act_var), _ptr(bias_var),
        O, I, F_SPLIT16 if split else 0, _stream())
    _lib.check(rc, "lbbnn_weight_pass")


def output_grad(g_out, *, out=None, std=None, eps=None, rng=None, rng_stream: int = 0, row_offset: int = 0,
                relu: bool = False, gv_scale=None, want_g: bool = True, defer_sums=None):
    """lbbnn_output_grad.  Returns (gm, gv, gmT, gvT, g_sum, gv_sum); the gv* are None for a posterior-mean forward.
    gv_scale (O,): per-column factor on G_v (the variational-dropout alpha).
    defer_sums: a list -- the column-sum partials stay in the workspace and a job for reduce_partials_flush is appended to
    it; g_sum / gv_sum are returned as (still unwritten) tensors that the flush fills."""
    B, O = g_out.shape
    f = dict(dtype=torch.float32, device=g_out.device)
    if g_out.stride(1) != 1:
        g_out = g_out.contiguous()
    stoch = std is not None
    # want_g=False: the caller needs no input gradient (a first layer): G_m / G_v themselves are not written, only G^T and sums
    gm, gmT, g_sum = (torch.empty((B, O), **f) if want_g else None), torch.empty((O, B), **f), torch.empty(O, **f)
    gv = gvT = gv_sum = None
    if stoch:
        gv, gvT, gv_sum = (torch.empty((B, O), **f) if want_g else None), torch.empty((O, B), **f), torch.empty(O, **f)
    if B == 0:
        g_sum.zero_()
        if stoch:
            gv_sum.zero_()
        return gm, gv, gmT, gvT, g_sum, gv_sum
    a = _lib.OutGradArgs()
    a.g_out = _ptr_rows(g_out, "g_out")
    a.out = _ptr_rows(out, "out") if (relu and out is not None) else None
    a.std = _ptr_rows(std, "std") if stoch else None
    ldo = out.stride(0) if (relu and out is not None) else (std.stride(0) if stoch else O)
    if relu and stoch and out.stride(0) != std.stride(0):
        raise ValueError("bnn_amd: out and std must share a row stride")
    a.eps = _ptr(eps, "eps") if (stoch and eps is not None) else None
    a.rng = rng.data_ptr() if rng is not None else None
    work = torch.empty(_lib.lib().lbbnn_output_grad_workspace(B, O), **f)
    a.gm, a.gmT, a.work = (gm.data_ptr() if gm is not None else None), gmT.data_ptr(), work.data_ptr()
    a.g_sum = g_sum.data_ptr() if defer_sums is None else None
    if stoch:
        a.gv, a.gvT = (gv.data_ptr() if gv is not None else None), gvT.data_ptr()
        a.gv_sum = gv_sum.data_ptr() if defer_sums is None else None
    if defer_sums is not None:
        nbt = (B + 63) // 64
        defer_sums.append(dict(work=work, outs=(g_sum, gv_sum, None), block_stride=O, q_stride=nbt * O, nblk=nbt, ncols=O,
                               nq=2 if stoch else 1))
    a.row_offset, a.rng_stream = row_offset, rng_stream
    a.gv_scale = _ptr(gv_scale, "gv_scale") if (stoch and gv_scale is not None) else None
    a.B, a.O, a.ldg, a.ldo, a.relu = B, O, g_out.stride(0), ldo, 1 if relu else 0
    _lib.check(_lib.lib().lbbnn_output_grad(ctypes.byref(a), _stream()), "lbbnn_output_grad")
    return gm, gv, gmT, gvT, g_sum, gv_sum


def head_dx(gm, gv, wmT, wvT, x, *, C: int, I: int):
    """lbbnn_head_dx: dX (B, I) of a <= 16-class head from G_m / G_v (B, C) and the transposed fp32 operands [I][ld]."""
    B = gm.shape[0]
    gm_ptr, gv_ptr = _ptr_rows(gm, "gm"), (_ptr_rows(gv, "gv") if gv is not None else None)
    if gv is not None and gv.stride(0) != gm.stride(0):
        raise ValueError("bnn_amd: gm and gv must share a row stride (got %d and %d)" % (gm.stride(0), gv.stride(0)))
    out = torch.empty((B, I), dtype=torch.float32, device=gm.device)
    rc = _lib.lib().lbbnn_head_dx(gm_ptr, gv_ptr, gm.stride(0),
                                  _ptr(wmT), _ptr(wvT), wmT.stride(0), _ptr_rows(x, "x") if gv is not None else None,
                                  x.stride(0) if gv is not None else 0, out.data_ptr(), I, B, C, I, _stream())
    _lib.check(rc, "lbbnn_head_dx")
    return out



def head_dw(gm, gv, x, *, nslabs: int = 16):
    """lbbnn_head_dw: (S, C, I) split-K slabs of dW_m = G_m^T x and dW_v = G_v^T x^2 of a <= 16-class head, from the row-major
    gradients (B, C) and the row-major layer input (B, I); gv None: (dWm, None)."""
    B, C = gm.shape
    I = x.shape[1]
    S = max(1, min(int(nslabs), B))
    dWm = torch.empty((S, C, I), dtype=torch.float32, device=gm.device)
    dWv = torch.empty((S, C, I), dtype=torch.float32, device=gm.device) if gv is not None else None
    rc = _lib.lib().lbbnn_head_dw(_ptr_rows(gm, "gm"), _ptr_rows(gv, "gv") if gv is not None else None, gm.stride(0),
                                  _ptr_rows(x, "x"), x.stride(0), dWm.data_ptr(), dWv.data_ptr() if dWv is not None else None,
                                  B, C, I, S, _stream())
    _lib.check(rc, "lbbnn_head_dw")
    return dWm, dWv


def matmul_splitk(a, w_op, *, K: int, N: int, kchunk: int):
    """lbbnn_matmul_splitk: slabs out[z] = a[:, Kz] @ w[Kz, :] (w given as its bf16x3 operand [N][ld(K)]);
    returns (S, M, N) with S = ceil(K / kchunk)."""
    M = a.shape[0]
    S = (K + kchunk - 1) // kchunk
    out = torch.empty((S, M, N), dtype=torch.float32, device=a.device)
    rc = _lib.lib().lbbnn_matmul_splitk(_ptr_rows(a, "a"), a.stride(0), _ptr(w_op), operand_ld(K), out.data_ptr(), N,
                                        M, K, N, kchunk, _stream())
    _lib.check(rc, "lbbnn_matmul_splitk")
    return out


def dx_combine(gx, gxv, x):
    """lbbnn_dx_combine: gx += 2 * x * gxv in place (gx, gxv dense (B,I); x may have a row stride)."""
    B, I = gx.shape
    rc = _lib.lib().lbbnn_dx_combine(_ptr(gx, "gx"), _ptr(gxv, "gxv"), _ptr_rows(x, "x"), x.stride(0), B, I, _stream())
    _lib.check(rc, "lbbnn_dx_combine")
    return gx


def weight_pass_backward(mu, rho, lambdal, dWm, dWv=None, *, z_fwd=None, z_kl=None, r0_c=None, da_mu=None,
                         da_var=None, g_kl=None, priors: Priors, work: Optional[torch.Tensor] = None, defer_sums=None):
    """lbbnn_weight_pass_backward (K1b).  Returns (dmu, drho, dlambdal, dz_fwd, dz_kl, dr0_c); the three
    vector gradients are None when the corresponding input vector was not given.
    defer_sums: a list -- as in output_grad: the three column sums are finished by reduce_partials_flush."""
    O, I = mu.shape
    a = _lib.WpbArgs()
    a.mu, a.rho, a.lambdal = _ptr(mu, "weight_mu"), _ptr(rho, "weight_rho"), _ptr(lambdal, "lambdal")
    nsplit = dWm.shape[0] if dWm.dim() == 3 else 1           # (S,O,I): split-K slabs, added inside the kernel
    for t, name in ((dWm, "dWm"), (dWv, "dWv")):
        if t is not None and (tuple(t.shape[-2:]) != tuple(mu.shape) or not t.is_contiguous()
                              or (t.shape[0] if t.dim() == 3 else 1) != nsplit):
            raise ValueError("bnn_amd: %s must be a contiguous (O,I) or (S,O,I) tensor" % name)
    a.dWm, a.dWv = _ptr(dWm, "dWm"), _ptr(dWv)
    a.z_fwd, a.z_kl, a.r0_c = _ptr(z_fwd), _ptr(z_kl), _ptr(r0_c)
    a.da_mu, a.da_var, a.g_kl = _ptr(da_mu), _ptr(da_var), _ptr(g_kl)
    a.priors = priors
    f = dict(dtype=torch.float32, device=mu.device)
    dmu, drho, dlam = torch.empty_like(mu), torch.empty_like(mu), torch.empty_like(mu)
    dz_fwd = torch.empty(I, **f) if z_fwd is not None else None
    dz_kl = torch.empty(I, **f) if (z_kl is not None and (g_kl is not None or da_mu is not None)) else None
    dr0_c = torch.empty(I, **f) if (r0_c is not None and da_mu is not None) else None
    need = _lib.lib().lbbnn_weight_pass_backward_workspace(O, I)
    if work is None or work.numel() < need:
        work = torch.empty(need, **f)
    a.dmu, a.drho, a.dlambdal = dmu.data_ptr(), drho.data_ptr(), dlam.data_ptr()
    deferred = defer_sums is not None and (dz_fwd is not None or dz_kl is not None or dr0_c is not None)
    a.work = work.data_ptr()
    a.dz_fwd, a.dz_kl, a.dr0_c = (None, None, None) if deferred else (_ptr(dz_fwd), _ptr(dz_kl), _ptr(dr0_c))
    a.O, a.I = O, I
    a.nsplit, a.split_stride = nsplit, O * I
    _lib.check(_lib.lib().lbbnn_weight_pass_backward(ctypes.byref(a), _stream()), "lbbnn_weight_pass_backward")
    if deferred:
        ld = (I + 3) & ~3
        # dr0_c is RETURNED as a parameter gradient: autograd adopts it as .grad only while nobody else holds a reference
        # (layers.join_vector_backward checks the adoption), so the job keeps its address, not the tensor
        defer_sums.append(dict(work=work, outs=(dz_fwd, dz_kl, None), ptrs=(_ptr(dz_fwd), _ptr(dz_kl), _ptr(dr0_c)),
                               block_stride=3 * ld, q_stride=ld, nblk=(O + 7) // 8, ncols=I, nq=3))
    return dmu, drho, dlam, dz_fwd, dz_kl, dr0_c


def reduce_partials_flush(pending):
    """lbbnn_reduce_partials_batch: finish the column sums that output_grad / weight_pass_backward left as partials
    (``defer_sums``), up to 8 jobs per launch, in filing order; clears the list."""
    i = 0
    while i < len(pending):
        grp = pending[i:i + 8]
        arr = (_lib.ReduceJob * len(grp))()
        for k, j in enumerate(grp):
            arr[k].work = j["work"].data_ptr()
            for q in range(3):
                arr[k].out[q] = j["ptrs"][q] if "ptrs" in j else (j["outs"][q].data_ptr() if j["outs"][q] is not None else None)
            arr[k].block_stride, arr[k].q_stride = j["block_stride"], j["q_stride"]
            arr[k].nblk, arr[k].ncols, arr[k].nq = j["nblk"], j["ncols"], j["nq"]
        _lib.check(_lib.lib().lbbnn_reduce_partials_batch(arr, len(grp), _stream()), "lbbnn_reduce_partials_batch")
        i += 8
    pending.clear()


# ----------------------------------------------------------------------------------------- K2
# When set to a GemmEventLog, every lrt_gemm launch is bracketed by HIP events recorded on the launch stream and
# (B, I, O, start, end) is logged -- bench.py's per-kernel roofline pass (run OUTSIDE its timed region).
# torch.cuda.Event creates the HIP event lazily at its first record(): the constructor therefore records every pooled
# event once and synchronises, so no event is created (or first touched by the runtime) between two bracketed launches.
class GemmEventLog(list):
    """``every``: bracket only every n-th launch group of ``group`` launches (the event records themselves cost host
    time: 6 per step made an otherwise GPU-bound eager loop host-bound)."""

    def __init__(self, launches: int, group: int = 1, every: int = 1):
        super().__init__()
        self._pool = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for s, e in self._pool:
            s.record()
            e.record()
        torch.cuda.synchronize()
        self._group, self._every, self._n = group, every, 0

    def take(self):
        k = self._n
        self._n += 1
        if (k // self._group) % self._every:
            return None
        return self._pool.pop() if self._pool else None


GEMM_EVENTS = None


class Finalize(NamedTuple):
    """What a forward's GEMM launch carries beside the product (lbbnn_gemm_desc_t::layers .. advance): the KL finalize of
    ``n`` layers (0: none) by one extra workgroup and, with ``advance``, ``rng_live[1] += advance``."""
    layers: object                      # _lib.LayerDesc array (or _lib.group_slice of one); None with n == 0
    n: int
    fin_rng: Optional[int]              # pointer of the Philox state K5 draws from
    kl_total: Optional[int]             # pointer of the network total, or None
    rng_live: Optional[int] = None      # pointer of the live Philox state
    advance: int = 0


def _gemm_input(x, cols: int, what: str, O: int, eps, finalize):
    """What both GEMM wrappers ask of x (B, cols) and eps (B, O).  Returns x with dense rows, or None for an empty batch
    without a finalize: (0, O) activations as torch.mm gives, no call (the KL side is unaffected by B)."""
    if x.dim() != 2 or x.shape[1] != cols:
        raise RuntimeError("bnn_amd: %s must be (B,%d), got %s" % (what, cols, tuple(x.shape)))
    B = x.shape[0]
    if eps is not None and tuple(eps.shape) != (B, O):
        raise RuntimeError("bnn_amd: eps must be (%d,%d), got %s" % (B, O, tuple(eps.shape)))
    if B == 0 and finalize is None:
        return None
    if x.stride(1) != 1 or x.stride(0) < cols:
        x = x.contiguous()
    return x


def _gemm_desc(x, e_w, var_w, *, I, O, bias_mean, bias_var, var_scale, eps, rng, rng_stream, row_offset, out, std_out, flags,
               finalize):
    """lbbnn_gemm_desc_t of the fields every operand format has; a format's own fields (scales, planes, head) stay zero."""
    d = _lib.GemmDesc()
    d.x, d.ldx = _ptr_rows(x, "input"), x.stride(0)
    d.e_w, d.var_w, d.ld = _ptr(e_w), _ptr(var_w), operand_ld(I)
    d.bias_mean, d.bias_var, d.var_scale, d.eps = _ptr(bias_mean), _ptr(bias_var), _ptr(var_scale), _ptr(eps, "eps")
    d.rng = rng.data_ptr() if rng is not None else None
    d.rng_stream, d.row_offset = rng_stream, row_offset
    d.out, d.ldo = (out.data_ptr(), out.stride(0)) if out is not None else (None, 0)
    d.std_out = _ptr(std_out, "std_out")
    d.B, d.I, d.O, d.flags = x.shape[0], I, O, flags
    if finalize is not None:            # a Finalize, or its fields in order (the last two may be left out)
        d.layers, d.n_layers, d.fin_rng, d.kl_total, d.rng_live, d.advance = finalize if len(finalize) == 6 else Finalize(*finalize)
    return d


def _gemm_call(name: str, args, B: int, I: int, O: int):
    """One single-GEMM library call on the current stream, checked; between a pair of GEMM_EVENTS' events when a log is set."""
    ev = GEMM_EVENTS.take() if GEMM_EVENTS is not None else None
    if ev is not None:
        ev[0].record()
    _lib.check(getattr(_lib.lib(), name)(*args, _stream()), name)
    if ev is not None:
        ev[1].record()
        GEMM_EVENTS.append((B, I, O, ev[0], ev[1]))


def lrt_gemm(x, e_w, var_w, *, I: int, O: int, bias_mean=None, bias_var=None, var_scale=None,
             eps=None, rng: Optional[torch.Tensor] = None, rng_stream: int = 0, row_offset: int = 0,
             relu: bool = False, mean_only: bool = False, log_softmax: bool = False,
             split: bool = False, out: Optional[torch.Tensor] = None, std_out: Optional[torch.Tensor] = None,
             finalize=None, half: bool = False, single: Optional[bool] = None):
    """lbbnn_lrt_gemm: out = x.e_w^T + b [+ sqrt(x^2.var_w^T + bv) * eps] [ReLU].
    single: ONE 16-bit product per moment (the reduced "bf16" / "fp16" modes; default: what the process-wide precision says).
    With ``std_out`` or ``finalize`` (a Finalize: the KL finalize of the whole network, n may be 0, and the forward's RNG advance
    ride in this launch) the call is lbbnn_lrt_gemm_ex: the descriptor carries what a forward adds to the product."""
    dev = x.device
    x = _gemm_input(x, I, "input", O, eps, finalize)
    B = 0 if x is None else x.shape[0]
    if out is None:
        out = torch.empty((B, O), dtype=torch.float32, device=dev)
    if x is None:
        return out
    flags = ((F_RELU if relu else 0) | (F_MEAN_ONLY if mean_only else 0) | (F_LOG_SOFTMAX if log_softmax else 0)
             | (F_SPLIT16 if split else 0)
             | (F_SINGLE16 if (split and not mean_only and (single if single is not None else _PRECISION in ("bf16", "fp16"))) else 0)
             | (F_HALF16 if (half and split and not mean_only) else 0))
    if std_out is None and finalize is None:
        _gemm_call("lbbnn_lrt_gemm", (
            _ptr_rows(x, "input"), x.stride(0), _ptr(e_w), _ptr(var_w), operand_ld(I),
            _ptr(bias_mean), _ptr(bias_var), _ptr(var_scale), _ptr(eps, "eps"),
            rng.data_ptr() if rng is not None else None, rng_stream, row_offset,
            out.data_ptr(), out.stride(0), B, I, O, flags), B, I, O)
    else:
        d = _gemm_desc(x, e_w, var_w, I=I, O=O, bias_mean=bias_mean, bias_var=bias_var, var_scale=var_scale, eps=eps, rng=rng,
                       rng_stream=rng_stream, row_offset=row_offset, out=out, std_out=std_out, flags=flags, finalize=finalize)
        _gemm_call("lbbnn_lrt_gemm_ex", (ctypes.byref(d),), B, I, O)
    return out


class GemmPlan(NamedTuple):
    """lbbnn_gemm_plan_t: the kernel instantiation a dual-moment GEMM call takes."""
    family: str              # "skinny" | "staged" | "dma" | "split" ("none": B == 0, nothing is launched)
    large_tile: bool
    xvec: bool
    mean_only: bool
    products: int
    half: bool
    fan: bool
    kernel_id: int


def lrt_gemm_plan_code(B: int, I: int, O: int, *, ldx: Optional[int] = None, x_aligned: bool = True, flags: int = 0,
                       members: int = 1, fan: int = 0, kchunk: int = 0):
    """lbbnn_lrt_gemm_plan as (return code, GemmPlan or None): a rejected input gives the launch's LBBNN_E_* code."""
    p = _lib.GemmPlan()
    rc = _lib.lib().lbbnn_lrt_gemm_plan(B, I, O, I if ldx is None else ldx, 1 if x_aligned else 0, flags, members, fan, kchunk,
                                        ctypes.byref(p))
    if rc != 0:
        return rc, None
    return 0, GemmPlan(_lib.GEMM_FAMILIES[p.family], bool(p.large_tile), bool(p.xvec), bool(p.mean_only), p.products,
                       bool(p.half), bool(p.fan), p.kernel_id)


def lrt_gemm_plan(B: int, I: int, O: int, **kw) -> GemmPlan:
    """The kernel ``lrt_gemm`` / ``vd_gemm_members`` / ``lrt_gemm_combine`` / ``matmul_splitk`` launch for these sizes, x layout
    (row stride ``ldx``, default I; ``x_aligned``: base on a 16-B boundary) and ``flags`` (the F_* bits), ``members`` > 1 for
    the member forms, ``fan`` > 0 for the fan-out, ``kchunk`` for split-K.  A host-side query: no tensor, no GPU.  Rejected
    inputs raise as the launch would."""
    rc, plan = lrt_gemm_plan_code(B, I, O, **kw)
    _lib.check(rc, "lbbnn_lrt_gemm_plan")
    return plan


def vd_gemm_members(x, e_w, var_w, var_scale, rng: torch.Tensor, *, I: int, O: int, members: int, fanout: bool = False,
                    rng_stream: int = 0, row_offset: int = 0, member_advance: int = 1, relu: bool = False,
                    split: bool = False, single: bool = False, half: bool = False, out: Optional[torch.Tensor] = None):
    """lbbnn_vd_gemm_members: variational dropout's dual-moment GEMM (var_scale = alpha, no bias) for ``members`` members,
    member m drawing its noise at Philox offset rng[1] + m * member_advance.  ``fanout``: x is the (B, I) input every member
    shares, whose two products are computed once; else x is (members, B, I) with a member stride that is a multiple of 4.
    ``out``: (members, B, O) with dense rows and a member stride that is a multiple of 4 (default: rows padded to 16 B per
    member).  single / half: one bf16 / fp16 product per moment (with ``split``)."""
    if fanout:
        if x.dim() != 2 or x.shape[1] != I:
            raise RuntimeError("bnn_amd: fan-out input must be (B,%d), got %s" % (I, tuple(x.shape)))
        ldx, x_ms, B = x.stride(0), 0, x.shape[0]
        xp = _ptr_rows(x, "input")
    else:
        if x.dim() != 3 or x.shape[0] != members or x.shape[2] != I:
            raise RuntimeError("bnn_amd: input must be (%d,B,%d), got %s" % (members, I, tuple(x.shape)))
        ldx, x_ms, B = x.stride(1), x.stride(0), x.shape[1]
        xp = _ptr_rows(x[0], "input")
    if out is None:
        out = torch.empty((members, pad4(B * O)), dtype=torch.float32, device=x.device)[:, :B * O].view(members, B, O)
    if tuple(out.shape) != (members, B, O) or out.stride(2) != 1:
        raise RuntimeError("bnn_amd: out must be (%d,%d,%d) with dense rows" % (members, B, O))
    flags = ((F_RELU if relu else 0) | (F_SPLIT16 if split else 0) | (F_SINGLE16 if (split and single) else 0)
             | (F_HALF16 if (split and half) else 0))
    rc = _lib.lib().lbbnn_vd_gemm_members(
        xp, ldx, x_ms, _ptr(e_w), _ptr(var_w), operand_ld(I), _ptr(var_scale, "var_scale"), _ptr(rng, "rng"), rng_stream,
        row_offset, member_advance, _ptr_rows(out[0], "out"), out.stride(1), out.stride(0), B, I, O, flags, members,
        1 if fanout else 0, _stream())
    _lib.check(rc, "lbbnn_vd_gemm_members")
    return out


def pad4(n: int) -> int:
    """n floats rounded up to a multiple of 4: rows and member blocks on 16-B boundaries."""
    return -(-n // 4) * 4


def member_gemm_chain(x, members: int, layers, *, head: str, out, empty=torch.empty, rng=None, stream=None):
    """A network's layers for ``members`` members, one member-GEMM launch per layer, wired by five rules: the member stride
    of a layer's output is pad4(B * O); every layer but the last gets ReLU; the last layer's epilogue applies log_softmax
    exactly when O <= 16 and ``head`` is "log_softmax"; the first layer reads the (B, I0) rows ``x`` for every member (member
    stride 0); each later layer reads what the previous one wrote, rows of ldx = its O.  ``layers``: per layer (operand, bias,
    split) -- one (O, ld) operand for all members or (members, O, ld), one (O,) bias or (members, O), whether the layer takes
    the bf16 hi | lo kernels: the mean-only form (lbbnn_gemm_members_mean) -- or (operand, bias, split, var_w, bias_var,
    rng_stream, row_offset): the dual-moment form (lbbnn_lrt_gemm_members; bias, var_w and bias_var shared; member m draws at
    Philox offset rng[1] + m of the state ``rng``).  The last layer writes ``out`` (members, >= pad4(B * O)), whose row
    stride is its member stride; the buffers between the layers come from ``empty``."""
    (B, I), last, dev = x.shape, len(layers) - 1, x.device
    stream = _stream() if stream is None else stream
    h, ldx, h_ms = x, x.stride(0), 0
    for i, (w, bias, split, *dual) in enumerate(layers):
        O, ld = w.size(-2), operand_ld(I)
        if i < last:
            o_ms, flags = pad4(B * O), F_RELU
            o = empty((members, o_ms), dtype=torch.float32, device=dev)
        else:
            o, o_ms, flags = out, out.stride(0), (F_LOG_SOFTMAX if O <= 16 and head == "log_softmax" else 0)
        if split:
            flags |= F_SPLIT16
        w_ms = O * ld if w.dim() == 3 else 0
        if dual:
            var_w, bias_var, rng_stream, row_offset = dual
            rc = _lib.lib().lbbnn_lrt_gemm_members(
                h.data_ptr(), ldx, h_ms, w.data_ptr(), w_ms, var_w.data_ptr(), ld, bias.data_ptr(), bias_var.data_ptr(),
                rng.data_ptr(), rng_stream, row_offset, 1, o.data_ptr(), O, o_ms, B, I, O, flags, members, stream)
            _lib.check(rc, "lbbnn_lrt_gemm_members")
        else:
            rc = _lib.lib().lbbnn_gemm_members_mean(
                h.data_ptr(), ldx, h_ms, w.data_ptr(), w_ms, ld, bias.data_ptr(), O if bias.dim() == 2 else 0,
                o.data_ptr(), O, o_ms, B, I, O, flags, members, stream)
            _lib.check(rc, "lbbnn_gemm_members_mean")
        h, ldx, h_ms, I = o, O, o_ms, O               # (h keeps the buffer alive until the launch that reads it is queued)
    return out


def sparse_row_ptr(kept_rows: torch.Tensor) -> torch.Tensor:
    """(O + 1,) int32 row pointers of a CSR layer: the exclusive scan of its (O,) kept_rows, the total last."""
    rp = torch.zeros(kept_rows.numel() + 1, dtype=torch.int32, device=kept_rows.device)
    torch.cumsum(kept_rows, 0, dtype=torch.int32, out=rp[1:])
    return rp


def sparse_row_pad(B: int) -> int:
    """Floats per unit of a transposed activation buffer [unit][sparse_row_pad(B)]: B rounded up to a wave's 64 rows."""
    return -(-B // 64) * 64


def sparse_member_chain(x, members: int, layers, *, head: str, out, empty=torch.empty, rng=None, stochastic: bool = True,
                        stream=None, levels: int = 0):
    """A sparse model's layers for ``members`` members: ONE lbbnn_transpose_operand launch lays the (B, I0) rows ``x`` out as
    x^T [I0][sparse_row_pad(B)], then one lbbnn_sparse_layer_members launch per layer.  The rules are member_gemm_chain's,
    with the activations between the layers transposed ([member][unit][sparse_row_pad(B)]): every layer but the last gets
    ReLU; the last writes ``out`` (members, >= pad4(B * O)) row-major and applies log_softmax exactly when O <= 16 and
    ``head`` is "log_softmax".  ``layers``: per layer (row_ptr, col, mean, var, bias_mu, bias_var, z, rng_stream, row_offset)
    with z None (LRT) or a (members, >= I) view of the members' z whose row stride is its member stride.  ``stochastic``
    False: the posterior-mean branch (no eps_out is drawn).
    ``levels`` = K >= 1: a threshold sweep's layers (row_ptr (K * O + 1), the K CSRs level after level) -- the same launches
    through lbbnn_sparse_layer_levels for K * ``members`` members, member j * members + s being level j under draw s; ``out``
    has K * members rows and z still ``members``."""
    (B, I), last, dev = x.shape, len(layers) - 1, x.device
    total = max(levels, 1) * members
    stream = _stream() if stream is None else stream
    ldb = sparse_row_pad(B)
    h = empty((I, ldb), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().lbbnn_transpose_operand(_ptr_rows(x, "x"), B, I, x.stride(0), h.data_ptr(), ldb, 0, 0, stream),
               "lbbnn_transpose_operand")
    h_ms = 0
    for i, (row_ptr, col, mean, var, bias_mu, bias_var, z, rng_stream, row_offset) in enumerate(layers):
        O = bias_mu.numel()
        flags = 0 if stochastic else F_MEAN_ONLY
        if i < last:
            o, ldo, o_ms, rows, flags = empty((total, O * ldb), dtype=torch.float32, device=dev), ldb, O * ldb, 0, flags | F_RELU
        else:
            o, ldo, o_ms, rows = out, O, out.stride(0), 1
            if O <= 16 and head == "log_softmax":
                flags |= F_LOG_SOFTMAX
        args = (row_ptr.data_ptr(), col.data_ptr(), mean.data_ptr(), var.data_ptr(), col.numel(), bias_mu.data_ptr(),
                bias_var.data_ptr(), h.data_ptr(), ldb, h_ms, None if z is None else z.data_ptr(), 0 if z is None else z.stride(0),
                None if rng is None else rng.data_ptr(), rng_stream, row_offset, 1, o.data_ptr(), ldo, o_ms, rows, B, I, O, flags)
        if levels:
            _lib.check(_lib.lib().lbbnn_sparse_layer_levels(*args, levels, members, stream), "lbbnn_sparse_layer_levels")
        else:
            _lib.check(_lib.lib().lbbnn_sparse_layer_members(*args, members, stream), "lbbnn_sparse_layer_members")
        h, h_ms, I = o, o_ms, O                       # (h keeps the buffer alive until the launch that reads it is queued)
    return out


def sparse_transposed_pattern(row_ptr: torch.Tensor, col: torch.Tensor, I: int):
    """(col_ptr (I + 1) int32, trow (nnz) int32, tslot (nnz) int32) of a CSR layer: the same entries column by column, rows
    ascending within a column; tslot[k] is the CSR slot of transposed entry k.  Torch ops on the tensors' own device, no host
    read: CSR slots are row-major, so a STABLE sort of the slots by column keeps the rows of a column in ascending order; the
    row of a slot is repeat_interleave of the row lengths (its output size is known: nnz); the column lengths are an integer
    scatter-add of ones (bincount would read its largest value back to size its result)."""
    nnz, O, dev = col.numel(), row_ptr.numel() - 1, col.device
    c = col.long()
    tslot = torch.argsort(c, stable=True)
    rows = torch.repeat_interleave(torch.arange(O, device=dev), (row_ptr[1:] - row_ptr[:-1]).long(), output_size=nnz)
    counts = torch.zeros(I, dtype=torch.int64, device=dev).index_add_(0, c, torch.ones(nnz, dtype=torch.int64, device=dev))
    col_ptr = torch.zeros(I + 1, dtype=torch.int32, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int32, out=col_ptr[1:])
    return col_ptr, rows[tslot].to(torch.int32), tslot.to(torch.int32)


def sparse_draw_members(layers, members: int, rng, *, weight_noise: bool = True, empty=torch.empty, stream=None):
    """The explicit weights of ``members`` sampled-weight members of a sparse model (lbbnn_sparse_draw_members, one launch per
    group of up to LBBNN_MAX_LAYERS layers).  ``layers``: per layer (col, mean, var, bias_mu, bias_var, z, layer_id, I, tpos)
    with z None (LRT) or a (members, >= I) view whose row stride is its member stride, and tpos None or the (nnz,) int32 place
    of every slot in the column-by-column order.  Member m draws at Philox offset rng[1] + m; ``weight_noise`` False: eps = 0,
    nothing is drawn.  Returns per layer (w (members, pad4(nnz)), b (members, pad4(O)), wt): wt the values once more at
    wt[m][tpos[k]] (None without tpos)."""
    stream = _stream() if stream is None else stream
    n = len(layers)
    descs = (_lib.SparseDrawDesc * n)()
    out = []
    for i, (col, mean, var, bias_mu, bias_var, z, layer_id, I, tpos) in enumerate(layers):
        nnz, O, dev = col.numel(), bias_mu.numel(), bias_mu.device
        ldw, ldb = pad4(nnz), pad4(O)
        w = empty((members, ldw), dtype=torch.float32, device=dev)
        b = empty((members, ldb), dtype=torch.float32, device=dev)
        wt = None if tpos is None else empty((members, ldw), dtype=torch.float32, device=dev)
        # (one constructor call in the struct's field order)
        descs[i] = _lib.SparseDrawDesc(col.data_ptr(), mean.data_ptr(), var.data_ptr(), bias_mu.data_ptr(), bias_var.data_ptr(),
                                       None if z is None else z.data_ptr(), 0 if z is None else z.stride(0),
                                       None if tpos is None else tpos.data_ptr(), None if wt is None else wt.data_ptr(),
                                       w.data_ptr(), ldw, b.data_ptr(), ldb, O, I, nnz, layer_id)
        out.append((w, b, wt))
    for k, cnt in _lib.layer_groups(n):
        rc = _lib.lib().lbbnn_sparse_draw_members(_lib.group_slice(descs, k, cnt), cnt, members,
                                                  rng.data_ptr() if weight_noise else None, 0 if weight_noise else F_MEAN_ONLY,
                                                  stream)
        _lib.check(rc, "lbbnn_sparse_draw_members")
    return out


def sparse_gather_members(mode: int, ptr, idx, slot, w, a, out, *, B: int, K: int, N: int, lda: int, a_mstride: int, ldo: int,
                          o_mstride: int, blocks: int, per_member: int = 1, bias=None, h=None, ldh: int = 0, h_mstride: int = 0,
                          relu: bool = False, out_rows: bool = False, a_shared: bool = False, dot_bias=None, dot_acc=None, stream=None):
    """One lbbnn_sparse_gather_members launch: the member layer on stored values ``w`` (members, >= nnz), pattern ptr / idx
    (values through ``slot`` when given), input lines ``a``, post-op ``mode`` (_lib.GATHER_*).  ``dot_bias`` (members, >= K) with
    ``dot_acc``: the same launch adds <a[block][.][b], dot_bias[m]> to dot_acc[(m * B + b) * per_member + c]."""
    # (one constructor call in the struct's field order: this runs six times per explanation)
    g = _lib.SparseGatherArgs(ptr.data_ptr(), idx.data_ptr(), None if slot is None else slot.data_ptr(), w.data_ptr(), w.stride(0),
                              None if bias is None else bias.data_ptr(), 0 if bias is None else bias.stride(0), a.data_ptr(),
                              a_mstride, None if h is None else h.data_ptr(), h_mstride, out.data_ptr(), o_mstride, lda, ldh, ldo,
                              B, K, N, idx.numel(), mode, int(relu), int(out_rows), int(a_shared), blocks, per_member,
                              None if dot_bias is None else dot_bias.data_ptr(), 0 if dot_bias is None else dot_bias.stride(0),
                              None if dot_acc is None else dot_acc.data_ptr())
    import ctypes
    _lib.check(_lib.lib().lbbnn_sparse_gather_members(ctypes.byref(g), _stream() if stream is None else stream),
               "lbbnn_sparse_gather_members")
    return out


def plane_ld(n: int) -> int:
    return operand_ld(n)


def head_slab_floats(B: int, O: int) -> int:
    return int(_lib.lib().lbbnn_head_slab_floats(B, O))


def format_x(x, planes=None):
    """lbbnn_format_x: fp32 rows (B, I) -> fp16 hi | lo planes, a (B, plane_ld(I)) fp32-sized buffer (tail zero)."""
    B, I = x.shape
    if x.stride(1) != 1:
        x = x.contiguous()
    if planes is None:
        planes = torch.empty((B, plane_ld(I)), dtype=torch.float32, device=x.device)
    rc = _lib.lib().lbbnn_format_x(_ptr_rows(x, "input"), x.stride(0), planes.data_ptr(), planes.stride(0), B, I, _stream())
    _lib.check(rc, "lbbnn_format_x")
    return planes


def lrt_gemm16(x, e_w, var_w, e_scale, v_scale, *, I: int, O: int, bias_mean=None, bias_var=None, var_scale=None,
               eps=None, rng: Optional[torch.Tensor] = None, rng_stream: int = 0, row_offset: int = 0, relu: bool = False,
               var1: bool = False, x_planes: bool = False, out: Optional[torch.Tensor] = None, want_out: bool = True,
               out_planes: Optional[torch.Tensor] = None, std_out: Optional[torch.Tensor] = None, finalize=None,
               head=None):
    """lbbnn_lrt_gemm_ex on LBBNN_F_F16S operands: the dual-moment GEMM + sampling epilogue of lrt_gemm in the row-scaled fp16
    format.  x: fp32 rows (B, I), or with ``x_planes`` the (B, plane_ld(I)) plane buffer a previous call / format_x wrote.
    Outputs: fp32 ``out`` (allocated unless ``want_out`` is False) and / or ``out_planes`` (B, plane_ld(O)) for the next layer.
    ``finalize`` as in lrt_gemm.  ``head``: dict(e_w, var_w (C, operand_ld(O)) fp32 operands of the <= 16-class layer that follows,
    bias_mean, bias_var, eps (or None), rng_stream, out (B, C), slab (head_slab_floats(B, O)), log_softmax) -- the head's GEMM
    is folded into this launch's epilogue + a small finalize launch.  Returns (out or None, out_planes or None)."""
    if x_planes and x.dim() == 2 and x.stride(1) != 1:
        raise RuntimeError("bnn_amd: x planes must have dense rows, got strides %s" % (tuple(x.stride()),))
    dev = x.device
    x = _gemm_input(x, plane_ld(I) if x_planes else I, "x planes" if x_planes else "input", O, eps, finalize)
    B = 0 if x is None else x.shape[0]
    if out is None and want_out:
        out = torch.empty((B, O), dtype=torch.float32, device=dev)
    if x is None:
        return out, out_planes
    d = _gemm_desc(x, e_w, var_w, I=I, O=O, bias_mean=bias_mean, bias_var=bias_var, var_scale=var_scale, eps=eps, rng=rng,
                   rng_stream=rng_stream, row_offset=row_offset, out=out, std_out=std_out, finalize=finalize,
                   flags=F_F16S | (F_RELU if relu else 0) | (F_VAR1 if var1 else 0) | (F_XPLANES if x_planes else 0))
    d.mean_scale, d.wvar_scale = _ptr(e_scale, "e_scale"), _ptr(v_scale, "v_scale")
    d.out_planes, d.ldp = (out_planes.data_ptr(), out_planes.stride(0)) if out_planes is not None else (None, 0)
    if head is not None:
        C = head["out"].shape[1]
        d.head_e, d.head_v, d.head_ld, d.head_classes = _ptr(head["e_w"]), _ptr(head["var_w"]), head["e_w"].stride(0), C
        d.head_bias_mean, d.head_bias_var, d.head_eps = _ptr(head.get("bias_mean")), _ptr(head.get("bias_var")), _ptr(head.get("eps"), "eps")
        d.head_rng_stream = head.get("rng_stream", 0)
        d.head_out, d.head_ldo, d.head_slab = head["out"].data_ptr(), head["out"].stride(0), _ptr(head["slab"])
        d.head_flags = F_LOG_SOFTMAX if head.get("log_softmax") else 0
    _gemm_call("lbbnn_lrt_gemm_ex", (ctypes.byref(d),), B, I, O)
    return out, out_planes


def lrt_gemm_combine(a, op, *, K: int, N: int, comb_x, comb_add, split: bool = False):
    """lbbnn_lrt_gemm_combine: comb_add + 2 * comb_x (.) (a (M,K) @ op^T), op = [N][operand_ld(K)]; writes into comb_add's
    storage (returned)."""
    M = a.shape[0]
    if a.stride(1) != 1:
        a = a.contiguous()
    rc = _lib.lib().lbbnn_lrt_gemm_combine(
        _ptr_rows(a, "a"), a.stride(0), _ptr(op), operand_ld(K), _ptr_rows(comb_x, "comb_x"), comb_x.stride(0),
        _ptr_rows(comb_add, "comb_add"), comb_add.stride(0), comb_add.data_ptr(), comb_add.stride(0), M, K, N,
        F_SPLIT16 if split else 0, _stream())
    _lib.check(rc, "lbbnn_lrt_gemm_combine")
    return comb_add


# ----------------------------------------------------------------------------------------- K3
def _ptr_array(ts: Sequence[torch.Tensor]):
    arr = (ctypes.c_void_p * max(len(ts), 1))()
    for i, t in enumerate(ts):
        arr[i] = _ptr(t, "flow parameter")
    return arr


def mnf_flow_planar(q0_mean, q0_log_var, z_params, r_params, *, eps_fwd=None, eps_kl=None,
                    rng: Optional[torch.Tensor] = None, layer_id: int = 0, z_fwd, z_kl=None, scal=None,
                    want_kl: bool = True):
    """lbbnn_mnf_flow_planar.  z_params / r_params: lists of (u, w, bias) per transform."""
    I = q0_mean.shape[0]
    zu, zw, zb = (_ptr_array([p[k] for p in z_params]) for k in range(3))
    ru, rw, rb = (_ptr_array([p[k] for p in r_params]) for k in range(3))
    rc = _lib.lib().lbbnn_mnf_flow_planar(
        _ptr(q0_mean, "q0_mean"), _ptr(q0_log_var, "q0_log_var"),
        zu, zw, zb, len(z_params), ru, rw, rb, len(r_params),
        _ptr(eps_fwd), _ptr(eps_kl), rng.data_ptr() if rng is not None else None, layer_id,
        _ptr(z_fwd), _ptr(z_kl), _ptr(scal), I, 1 if want_kl else 0, _stream())
    _lib.check(rc, "lbbnn_mnf_flow_planar")


K3_GENERIC, K3_LDS, K3_FAST, K3_VEC = 0, 1, 2, 3        # LBBNN_K3_*: the form of a K3 launch
K5_GENERIC, K5_LDS = 0, 1                               # LBBNN_K5_*: the per-layer K5 launch
K5_UNSTAGED, K5_STAGED = 0, 1                           # ... and the all-layers launch


def _c_ints(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def flow_planar_form(layers, members: int = 1) -> int:
    """lbbnn_flow_planar_form: the kernel form ONE K3 launch over ``layers`` = [(I, Tz, Tr, want_kl, aligned16)] takes
    (K3_*), or the LBBNN_E_* code the launch would return.  Host only: no tensor, no GPU."""
    cols = list(zip(*layers)) if layers else [()] * 5
    return int(_lib.lib().lbbnn_flow_planar_form(len(layers), *[_c_ints(c) for c in cols], members))


def kl_finalize_form(layers, all_layers: bool = False) -> int:
    """lbbnn_kl_finalize_form for ``layers`` = [(O, I, mnf, active)]: K5_GENERIC / K5_LDS of the per-layer launch, or, with
    ``all_layers``, K5_UNSTAGED / K5_STAGED of lbbnn_layers_finalize's; a negative LBBNN_E_* code for inputs the launch
    refuses.  Host only."""
    cols = list(zip(*layers)) if layers else [()] * 4
    return int(_lib.lib().lbbnn_kl_finalize_form(len(layers), *[_c_ints(c) for c in cols], 1 if all_layers else 0))


FLOW_PLANAR, FLOW_RADIAL, FLOW_HOUSEHOLDER, FLOW_SYLVESTER = 0, 1, 2, 3


def flow_chain(steps, *, I: int, z_in=None, q0_mean=None, q0_log_var=None, eps=None, rng=None, rng_stream: int = 0,
               z_out: Optional[torch.Tensor] = None, logdet=None, log_q0=None, z_last=None):
    """lbbnn_flow_chain.  steps: list of (type, M, p0, p1, p2) (tensors or None).  Returns (z_out, logdet)."""
    if len(steps) > _lib.MAX_FLOW_T:
        raise ValueError("bnn_amd: at most %d transforms per flow" % _lib.MAX_FLOW_T)
    ch = _lib.FlowChain()
    ch.n = len(steps)
    for k, (ty, M, p0, p1, p2) in enumerate(steps):
        st = ch.step[k]
        st.type, st.M = ty, M
        st.p0, st.p1, st.p2 = _ptr(p0, "flow parameter"), _ptr(p1, "flow parameter"), _ptr(p2, "flow parameter")
    ref = z_in if z_in is not None else q0_mean
    if z_out is None:
        z_out = torch.empty(I, dtype=torch.float32, device=ref.device)
    if logdet is None:
        logdet = torch.empty(1, dtype=torch.float32, device=ref.device)
    rc = _lib.lib().lbbnn_flow_chain(ctypes.byref(ch), _ptr(z_in, "z"), _ptr(q0_mean), _ptr(q0_log_var), _ptr(eps),
                                     rng.data_ptr() if rng is not None else None, rng_stream, I,
                                     z_out.data_ptr(), logdet.data_ptr(),
                                     log_q0.data_ptr() if log_q0 is not None else None,
                                     z_last.data_ptr() if z_last is not None else None, _stream())
    _lib.check(rc, "lbbnn_flow_chain")
    return z_out, logdet


def flow_chain_rows(steps, z: torch.Tensor):
    """lbbnn_flow_chain_rows: the 1-D chain applied to every row of z (R,I).  Returns (z_out (R,I), logdet (R,))."""
    if len(steps) > _lib.MAX_FLOW_T:
        raise ValueError("bnn_amd: at most %d transforms per flow" % _lib.MAX_FLOW_T)
    ch = _lib.FlowChain()
    ch.n = len(steps)
    for k, (ty, M, p0, p1, p2) in enumerate(steps):
        st = ch.step[k]
        st.type, st.M = ty, M
        st.p0, st.p1, st.p2 = _ptr(p0, "flow parameter"), _ptr(p1, "flow parameter"), _ptr(p2, "flow parameter")
    z = z.float()
    if z.stride(1) != 1:
        z = z.contiguous()
    R, I = z.shape
    z_out = torch.empty((R, I), dtype=torch.float32, device=z.device)
    logdet = torch.zeros(R, dtype=torch.float32, device=z.device)
    rc = _lib.lib().lbbnn_flow_chain_rows(ctypes.byref(ch), _ptr_rows(z, "z"), z.stride(0), R, I, z_out.data_ptr(), I,
                                          logdet.data_ptr(), _stream())
    _lib.check(rc, "lbbnn_flow_chain_rows")
    return z_out, logdet


def mnf_aux_backward(act_mu, act_var, eps_act, r0_b1, r0_b2, zb_last, g_kl, rng=None, layer_id: int = 0):
    """lbbnn_mnf_aux_backward -> (da_mu, da_var, aux); zb_last: 1-element view of the forward's scal[3]."""
    O, I = act_mu.shape[0], r0_b1.shape[0]
    da_mu, da_var = torch.empty_like(act_mu), torch.empty_like(act_mu)
    aux = torch.empty(4, dtype=torch.float32, device=act_mu.device)
    rc = _lib.lib().lbbnn_mnf_aux_backward(_ptr(act_mu, "act_mu"), _ptr(act_var, "act_var"), _ptr(eps_act, "eps_act"),
                                           _ptr(r0_b1, "r0_b1"), _ptr(r0_b2, "r0_b2"), zb_last.data_ptr(), _ptr(g_kl, "g_kl"),
                                           O, I, da_mu.data_ptr(), da_var.data_ptr(), aux.data_ptr(),
                                           rng.data_ptr() if rng is not None else None, layer_id, _stream())
    _lib.check(rc, "lbbnn_mnf_aux_backward")
    return da_mu, da_var, aux


def bias_backward(bias_mu, bias_rho, g_sum, gv_sum, g_kl, priors: Priors):
    """lbbnn_bias_backward -> (d_bias_mu, d_bias_rho) of a layer without flows (gv_sum / g_kl may be None)."""
    d_mu, d_rho = torch.empty_like(bias_mu), torch.empty_like(bias_rho)
    rc = _lib.lib().lbbnn_bias_backward(_ptr(bias_mu, "bias_mu"), _ptr(bias_rho, "bias_rho"), _ptr(g_sum, "g_sum"),
                                        _ptr(gv_sum), _ptr(g_kl), ctypes.byref(priors), d_mu.data_ptr(), d_rho.data_ptr(),
                                        bias_mu.shape[0], _stream())
    _lib.check(rc, "lbbnn_bias_backward")
    return d_mu, d_rho


def bias_backward_partials(job, B, bias_mu, bias_rho, g_kl, priors: Priors):
    """lbbnn_bias_backward_partials: `job` is what output_grad(defer_sums=[...]) filed (its partials wait in job["work"])."""
    d_mu, d_rho = torch.empty_like(bias_mu), torch.empty_like(bias_rho)
    rc = _lib.lib().lbbnn_bias_backward_partials(job["work"].data_ptr(), B, bias_mu.shape[0], 1 if job["nq"] == 2 else 0,
                                                 _ptr(bias_mu, "bias_mu"), _ptr(bias_rho, "bias_rho"), _ptr(g_kl),
                                                 ctypes.byref(priors), d_mu.data_ptr(), d_rho.data_ptr(), _stream())
    _lib.check(rc, "lbbnn_bias_backward_partials")
    return d_mu, d_rho


def mnf_aux_backward_batch(items, g_kl):
    """lbbnn_mnf_aux_backward_batch: V1 of several layers in one launch.  items: dicts with act_mu, act_var, eps_act (or
    None), r0_b1, r0_b2, zb_last, rng (or None), layer_id.  Returns [(da_mu, da_var, aux)] in the same order."""
    outs = []
    i = 0
    while i < len(items):
        grp = items[i:i + 4]
        arr = (_lib.AuxBwdArgs * len(grp))()
        for k, it in enumerate(grp):
            da_mu, da_var = torch.empty_like(it["act_mu"]), torch.empty_like(it["act_mu"])
            aux = torch.empty(4, dtype=torch.float32, device=da_mu.device)
            a = arr[k]
            a.act_mu, a.act_var, a.eps_act = _ptr(it["act_mu"], "act_mu"), _ptr(it["act_var"], "act_var"), _ptr(it.get("eps_act"))
            a.r0_b1, a.r0_b2, a.zb_last, a.g_kl = _ptr(it["r0_b1"]), _ptr(it["r0_b2"]), it["zb_last"].data_ptr(), _ptr(g_kl, "g_kl")
            a.da_mu, a.da_var, a.aux = da_mu.data_ptr(), da_var.data_ptr(), aux.data_ptr()
            a.rng = it["rng"].data_ptr() if it.get("rng") is not None else None
            a.O, a.I, a.layer_id = da_mu.shape[0], it["r0_b1"].shape[0], it["layer_id"]
            outs.append((da_mu, da_var, aux))
        _lib.check(_lib.lib().lbbnn_mnf_aux_backward_batch(arr, len(grp), _stream()), "lbbnn_mnf_aux_backward_batch")
        i += 4
    return outs


def mnf_flow_planar_backward(q0_mean, q0_log_var, z_params, r_params, *, eps_fwd=None, eps_kl=None, r0_b1=None, r0_b2=None,
                             aux=None, dz_fwd=None, dz_kl=None, g_kl=None, bias_mu, bias_rho, g_sum, gv_sum=None,
                             priors: Priors, rng=None, layer_id: int = 0, defer=None):
    """lbbnn_mnf_flow_planar_backward.  Returns a dict: q0_mean, q0_log_var, r0_b1, r0_b2, bias_mu, bias_rho and
    z_flow / r_flow = lists of (du, dw, dbias) per transform.  ``defer``: a list -- the launch is NOT issued; the filled
    argument struct (with everything it points to kept alive) is appended for mnf_flow_planar_backward_flush."""
    I, O = q0_mean.shape[0], bias_mu.shape[0]
    a = _lib.FlowBwdArgs()
    for name, t in (("q0_mean", q0_mean), ("q0_log_var", q0_log_var), ("eps_fwd", eps_fwd), ("eps_kl", eps_kl),
                    ("r0_b1", r0_b1), ("r0_b2", r0_b2), ("aux", aux), ("dz_fwd", dz_fwd), ("dz_kl", dz_kl),
                    ("g_kl", g_kl), ("bias_mu", bias_mu), ("bias_rho", bias_rho), ("g_sum", g_sum), ("gv_sum", gv_sum)):
        setattr(a, name, _ptr(t, name))
    a.priors = priors
    f = dict(dtype=torch.float32, device=q0_mean.device)
    out = {n: torch.empty(I, **f) for n in ("q0_mean", "q0_log_var", "r0_b1", "r0_b2")}
    out["bias_mu"], out["bias_rho"] = torch.empty(O, **f), torch.empty(O, **f)
    for n in ("q0_mean", "q0_log_var", "r0_b1", "r0_b2", "bias_mu", "bias_rho"):
        setattr(a, "d_" + n, out[n].data_ptr())
    for key, params, fl, gr in (("z_flow", z_params, a.z_flow, a.d_z_flow), ("r_flow", r_params, a.r_flow, a.d_r_flow)):
        fl.T = len(params)
        grads = []
        for t, (u, w, b) in enumerate(params):
            fl.u[t], fl.w[t], fl.b[t] = _ptr(u, "flow u"), _ptr(w, "flow w"), _ptr(b, "flow bias")
            g3 = (torch.empty_like(u), torch.empty_like(w), torch.empty_like(b))
            gr.u[t], gr.w[t], gr.b[t] = g3[0].data_ptr(), g3[1].data_ptr(), g3[2].data_ptr()
            grads.append(g3)
        out[key] = grads
    work = torch.empty(_lib.lib().lbbnn_mnf_flow_backward_workspace(I, len(z_params), len(r_params)), **f)
    a.work, a.O, a.I = work.data_ptr(), O, I
    a.rng, a.layer_id = (rng.data_ptr() if rng is not None else None), layer_id
    if defer is not None:
        keep = (q0_mean, q0_log_var, eps_fwd, eps_kl, r0_b1, r0_b2, aux, dz_fwd, dz_kl, g_kl, bias_mu, bias_rho, g_sum, gv_sum,
                z_params, r_params, work, rng)
        # (NOT the output tensors: autograd must hold the only reference so that AccumulateGrad adopts them instead of
        # copying them -- a copy made before the deferred launch would copy unwritten memory)
        defer.append((a, keep))
        return out
    _lib.check(_lib.lib().lbbnn_mnf_flow_planar_backward(ctypes.byref(a), _stream()), "lbbnn_mnf_flow_planar_backward")
    return out


def mnf_flow_planar_backward_flush(pending):
    """Issue the deferred V2 chains: ONE launch per group of up to 4 layers (lbbnn_mnf_flow_planar_backward_batch), or one
    launch each where a flow has more than 4 transforms."""
    i = 0
    while i < len(pending):
        grp = pending[i:i + 4]
        arr = (_lib.FlowBwdArgs * len(grp))()
        for k, (a, _) in enumerate(grp):
            ctypes.memmove(ctypes.byref(arr[k]), ctypes.byref(a), ctypes.sizeof(_lib.FlowBwdArgs))
        rc = _lib.lib().lbbnn_mnf_flow_planar_backward_batch(arr, len(grp), _stream())
        if rc == -2:                                  # LBBNN_E_SHAPE: a flow with more than 4 transforms
            for a, _ in grp:
                _lib.check(_lib.lib().lbbnn_mnf_flow_planar_backward(ctypes.byref(a), _stream()), "lbbnn_mnf_flow_planar_backward")
        else:
            _lib.check(rc, "lbbnn_mnf_flow_planar_backward_batch")
        i += 4
    pending.clear()


_DENSE_GRAD_FIELDS = {0: ("w_in", "b_in", ("w_mid", 0), ("b_mid", 0), ("w_mid", 1), ("b_mid", 1), ("w_mid", 2), ("b_mid", 2),
                          "w_a", "b_a", "w_b", "b_b"),
                      1: ("w_in", "b_in", "w_a", "b_a", "w_b", "b_b")}


def _dense_grad_array(kind_id, params, T):
    """lbbnn_dense_grad_t array + fresh gradient tensors for T transforms whose parameters come in module order
    (RNVP: network.0/2/4/6 weight, bias, t, s; MNF type: f, g, k -- the order dense_descs reads them in)."""
    fields = _DENSE_GRAD_FIELDS[kind_id]
    n = len(fields)
    arr = (_lib.DenseGrad * max(T, 1))()
    grads = [torch.empty_like(p) for p in params[:T * n]]
    for t in range(T):
        for f, g in zip(fields, grads[t * n:(t + 1) * n]):
            if isinstance(f, tuple):
                getattr(arr[t], f[0])[f[1]] = g.data_ptr()
            else:
                setattr(arr[t], f, g.data_ptr())
    return arr, grads


def mnf_flow_dense_backward(q0_mean, q0_log_var, z_descs, Tz, z_kind, z_params, r_descs, Tr, r_kind, r_params, *, save,
                            eps_fwd=None, eps_kl=None, r0_b1=None, r0_b2=None, aux=None, dz_fwd=None, dz_kl=None, g_kl=None,
                            bias_mu, bias_rho, g_sum, gv_sum=None, priors: Priors, rng=None, layer_id: int = 0, defer=None,
                            keep=()):
    """lbbnn_mnf_flow_dense_backward (``defer``: a list -- nothing is launched, the filled argument struct and what it
    points to are appended for mnf_flow_dense_backward_flush).  z_descs / r_descs: the forward's lbbnn_dense_transform_t arrays (same masks);
    z_params / r_params: the flows' parameter tensors in module order (shapes of the gradients).  Returns a dict:
    q0_mean, q0_log_var, r0_b1, r0_b2, bias_mu, bias_rho and z_flow / r_flow = flat gradient lists in parameter order."""
    I, O = q0_mean.shape[0], bias_mu.shape[0]
    a = _lib.DenseBwdArgs()
    for name, t in (("q0_mean", q0_mean), ("q0_log_var", q0_log_var), ("eps_fwd", eps_fwd), ("eps_kl", eps_kl),
                    ("r0_b1", r0_b1), ("r0_b2", r0_b2), ("aux", aux), ("dz_fwd", dz_fwd), ("dz_kl", dz_kl),
                    ("g_kl", g_kl), ("bias_mu", bias_mu), ("bias_rho", bias_rho), ("g_sum", g_sum), ("gv_sum", gv_sum),
                    ("save", save)):
        setattr(a, name, _ptr(t, name))
    a.priors = priors
    f = dict(dtype=torch.float32, device=q0_mean.device)
    out = {n: torch.empty(I, **f) for n in ("q0_mean", "q0_log_var", "r0_b1", "r0_b2")}
    out["bias_mu"], out["bias_rho"] = torch.empty(O, **f), torch.empty(O, **f)
    for n in ("q0_mean", "q0_log_var", "r0_b1", "r0_b2", "bias_mu", "bias_rho"):
        setattr(a, "d_" + n, out[n].data_ptr())
    gz, out["z_flow"] = _dense_grad_array(z_kind, z_params, Tz)
    gr, out["r_flow"] = _dense_grad_array(r_kind, r_params, Tr)
    a.zt = ctypes.cast(z_descs, ctypes.POINTER(_lib.DenseTransform))
    a.rt = ctypes.cast(r_descs, ctypes.POINTER(_lib.DenseTransform)) if r_descs is not None else None
    a.d_zt = ctypes.cast(gz, ctypes.POINTER(_lib.DenseGrad))
    a.d_rt = ctypes.cast(gr, ctypes.POINTER(_lib.DenseGrad))
    work = torch.empty(_lib.lib().lbbnn_mnf_flow_dense_backward_workspace(I), **f)
    a.work, a.Tz, a.Tr, a.O, a.I = work.data_ptr(), Tz, Tr, O, I
    a.rng, a.layer_id = (rng.data_ptr() if rng is not None else None), layer_id
    if defer is not None:
        # (the output tensors are NOT kept here: autograd must hold their only reference, see mnf_flow_planar_backward)
        alive = (q0_mean, q0_log_var, eps_fwd, eps_kl, r0_b1, r0_b2, aux, dz_fwd, dz_kl, g_kl, bias_mu, bias_rho, g_sum, gv_sum,
                 save, z_descs, r_descs, z_params, r_params, gz, gr, work, rng, keep)
        defer.append((a, alive, (Tz, Tr, g_kl is not None)))
        return out
    _lib.check(_lib.lib().lbbnn_mnf_flow_dense_backward(ctypes.byref(a), _stream()), "lbbnn_mnf_flow_dense_backward")
    return out


def mnf_flow_dense_backward_flush(pending):
    """Issue the deferred dense-flow chains: layers that agree on (Tz, Tr, KL branch) share their launches
    (lbbnn_mnf_flow_dense_backward_batch, up to 4 layers per call)."""
    groups = {}
    for item in pending:
        groups.setdefault(item[2], []).append(item)
    for items in groups.values():
        for i in range(0, len(items), 4):
            grp = items[i:i + 4]
            arr = (_lib.DenseBwdArgs * len(grp))()
            for k, (a, _, _) in enumerate(grp):
                ctypes.memmove(ctypes.byref(arr[k]), ctypes.byref(a), ctypes.sizeof(_lib.DenseBwdArgs))
            _lib.check(_lib.lib().lbbnn_mnf_flow_dense_backward_batch(arr, len(grp), _stream()), "lbbnn_mnf_flow_dense_backward_batch")
    pending.clear()


def q0_rows(q0_mean, q0_log_var, R: int, *, eps=None, rng=None, rng_stream: int = 0):
    """lbbnn_q0_rows: z0 (R,I) = q0_mean + exp(q0_log_var)^.5 * eps, eps (R,I) explicit or Philox."""
    I = q0_mean.shape[0]
    if eps is not None:
        eps = eps.reshape(R, I).float().contiguous()
    elif rng is None:
        raise RuntimeError("bnn_amd: q0_rows needs explicit eps or an rng state")
    z0 = torch.empty((R, I), dtype=torch.float32, device=q0_mean.device)
    _lib.check(_lib.lib().lbbnn_q0_rows(_ptr(q0_mean, "q0_mean"), _ptr(q0_log_var, "q0_log_var"), _ptr(eps, "eps"),
                                        rng.data_ptr() if rng is not None else None, rng_stream, R, I, z0.data_ptr(),
                                        _stream()), "lbbnn_q0_rows")
    return z0


def flow_dense_rows(descs, T: int, z: torch.Tensor, *, masks: Optional[torch.Tensor] = None, rng: Optional[torch.Tensor] = None,
                    rng_stream: int = STREAM_ROW_MASK * 64, row_base: int = 0, want_masks: bool = False, keep=()):
    """lbbnn_flow_dense_rows: a chain of T dense coupling transforms (``descs`` = PropagateFlow.dense_descs(None, None)[0])
    on the R rows of z (R,I), each row with its own masks.  masks: (T,R,I) in {0,1} or None (drawn in-kernel from ``rng``).
    Returns (z_out (R,I), logdet_rows (R,), masks used (T,R,I) or None)."""
    if z.dim() != 2:
        raise RuntimeError("bnn_amd: flow_dense_rows wants z as (R,I), got %s" % (tuple(z.shape),))
    R, I = z.shape
    if I > _lib.lib().lbbnn_flow_dense_rows_max_dim():
        raise RuntimeError("bnn_amd: row-batched dense flows hold 16 rows of z in LDS: dim %d exceeds the limit %d"
                           % (I, _lib.lib().lbbnn_flow_dense_rows_max_dim()))
    z = z.float()
    if z.stride(1) != 1:
        z = z.contiguous()
    f = dict(dtype=torch.float32, device=z.device)
    if masks is not None:
        if tuple(masks.shape) != (T, R, I):
            raise RuntimeError("bnn_amd: masks must be (%d,%d,%d), got %s" % (T, R, I, tuple(masks.shape)))
        masks = masks.float().contiguous()
    elif rng is None:
        raise RuntimeError("bnn_amd: flow_dense_rows needs explicit masks or an rng state")
    z_out = torch.empty((R, I), **f)
    logdet = torch.zeros(R, **f)
    mask_out = torch.empty((T, R, I), **f) if (want_masks and masks is None) else None
    _lib.check(_lib.lib().lbbnn_flow_dense_rows(
        descs, T, _ptr(masks, "masks"), _ptr(mask_out), rng.data_ptr() if rng is not None else None, rng_stream,
        int(row_base), _ptr_rows(z, "z"), z.stride(0), R, I, z_out.data_ptr(), I, logdet.data_ptr(), _stream()),
        "lbbnn_flow_dense_rows")
    del keep
    return z_out, logdet, (masks if masks is not None else mask_out)


def flow_dense_save_size(I: int, Tz: int, Tr: int) -> int:
    return int(_lib.lib().lbbnn_flow_dense_save_size(I, Tz, Tr))


# ----------------------------------------------------------------------------------------- K4
def mnf_flow_dense(q0_mean, q0_log_var, z_descs, Tz, r_descs, Tr, *, eps_fwd=None, eps_kl=None,
                   rng: Optional[torch.Tensor] = None, layer_id: int = 0, z_fwd, z_kl=None, scal=None, work=None,
                   want_kl: bool = True):
    """lbbnn_mnf_flow_dense.  z_descs / r_descs: ctypes arrays of _lib.DenseTransform (see flows.dense_descs)."""
    I = q0_mean.shape[0]
    rc = _lib.lib().lbbnn_mnf_flow_dense(
        _ptr(q0_mean, "q0_mean"), _ptr(q0_log_var, "q0_log_var"),
        z_descs, Tz, r_descs, Tr,
        _ptr(eps_fwd), _ptr(eps_kl), rng.data_ptr() if rng is not None else None, layer_id,
        _ptr(z_fwd), _ptr(z_kl), _ptr(scal), _ptr(work), I, 1 if want_kl else 0, _stream())
    _lib.check(rc, "lbbnn_mnf_flow_dense")


def flow_dense_workspace(I: int) -> int:
    return int(_lib.lib().lbbnn_flow_dense_workspace(I))


# ----------------------------------------------------------------------------------------- K5
def kl_total(kls: torch.Tensor, n: int) -> torch.Tensor:
    """lbbnn_kl_total: kls[n] = ((0 + kls[0]) + kls[1]) + ... + kls[n - 1] in fp32, one launch; ``kls`` holds n + 1 contiguous
    floats (the per-layer values the finalize launches of a deep network wrote, then the total).  Returns kls[n]."""
    if kls.dtype != torch.float32 or not kls.is_contiguous() or kls.numel() < n + 1:
        raise RuntimeError("bnn_amd: kl_total needs a contiguous fp32 buffer of n + 1 values")
    _lib.check(_lib.lib().lbbnn_kl_total(kls.data_ptr(), n, kls.data_ptr() + 4 * n, _stream()), "lbbnn_kl_total")
    return kls[n]


def fold_rows(v: torch.Tensor, rows: int, n: int) -> torch.Tensor:
    """lbbnn_fold_rows: out[r] = ((0 + v[r][0]) + v[r][1]) + ... + v[r][n - 1] in fp32 for r < rows, one launch; ``v`` is a
    (>= rows, >= n) fp32 device tensor with dense rows.  Returns a new (rows,) tensor."""
    if not v.is_cuda:
        raise RuntimeError("bnn_amd: fold_rows needs a HIP device tensor (v is on %s); there is no CPU path" % v.device)
    if v.dtype != torch.float32 or v.dim() != 2 or v.shape[0] < rows or v.shape[1] < n or (v.shape[1] > 1 and v.stride(1) != 1):
        raise RuntimeError("bnn_amd: fold_rows needs a 2-D fp32 buffer of at least (rows, n) values with dense rows")
    out = torch.empty(rows, dtype=torch.float32, device=v.device)
    _lib.check(_lib.lib().lbbnn_fold_rows(v.data_ptr(), rows, n, v.stride(0), out.data_ptr(), _stream()), "lbbnn_fold_rows")
    return out


def kl_finalize(kl_rows, bias_mu, bias_rho, *, priors: Priors, act_mu=None, act_var=None, eps_act=None,
                r0_b1=None, r0_b2=None, scal=None, rng: Optional[torch.Tensor] = None, layer_id: int = 0,
                kl_out=None, kl_layer=None, accumulate: bool = False):
    O = bias_mu.shape[0]
    I = r0_b1.shape[0] if r0_b1 is not None else 0
    rc = _lib.lib().lbbnn_kl_finalize(
        _ptr(kl_rows), _ptr(bias_mu, "bias_mu"), _ptr(bias_rho, "bias_rho"), O,
        _ptr(act_mu), _ptr(act_var), _ptr(eps_act), _ptr(r0_b1), _ptr(r0_b2), I,
        _ptr(scal), ctypes.byref(priors), rng.data_ptr() if rng is not None else None, layer_id,
        _ptr(kl_out), _ptr(kl_layer), 1 if accumulate else 0, _stream())
    _lib.check(rc, "lbbnn_kl_finalize")


def transpose_operand(src: torch.Tensor, *, square: bool = False, split: bool = False,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lbbnn_transpose_operand: (R,C) fp32 -> GEMM operand [C][operand_ld(R)] holding src^T (squared if asked)."""
    R, C = src.shape
    ld = operand_ld(R)
    if out is None:
        out = torch.empty((C, ld), dtype=torch.float32, device=src.device)
    rc = _lib.lib().lbbnn_transpose_operand(_ptr_rows(src, "src"), R, C, src.stride(0), out.data_ptr(), ld,
                                            1 if square else 0, F_SPLIT16 if split else 0, _stream())
    _lib.check(rc, "lbbnn_transpose_operand")
    return out


def format_operand(src: torch.Tensor, *, square: bool = False, split: bool = False) -> torch.Tensor:
    """lbbnn_format_operand: (R,C) fp32 -> GEMM operand [R][operand_ld(C)] holding src (squared if asked), no transpose."""
    R, C = src.shape
    ld = operand_ld(C)
    out = torch.empty((R, ld), dtype=torch.float32, device=src.device)
    rc = _lib.lib().lbbnn_format_operand(_ptr_rows(src, "src"), R, C, src.stride(0), out.data_ptr(), ld,
                                         1 if square else 0, F_SPLIT16 if split else 0, _stream())
    _lib.check(rc, "lbbnn_format_operand")
    return out


def log_softmax_backward(g: torch.Tensor, logp: torch.Tensor) -> torch.Tensor:
    """lbbnn_log_softmax_backward: g - exp(logp) * rowsum(g) for (B, C <= 64) tensors."""
    B, C = g.shape
    if g.stride(1) != 1:
        g = g.contiguous()
    out = torch.empty((B, C), dtype=torch.float32, device=g.device)
    rc = _lib.lib().lbbnn_log_softmax_backward(_ptr_rows(g, "g"), g.stride(0), _ptr_rows(logp, "logp"), logp.stride(0),
                                               out.data_ptr(), C, B, C, _stream())
    _lib.check(rc, "lbbnn_log_softmax_backward")
    return out


def log_softmax_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B, O = x.shape
    if out is None:
        out = torch.empty_like(x)
    rc = _lib.lib().lbbnn_log_softmax_rows(_ptr(x, "input"), x.stride(0), out.data_ptr(), out.stride(0), B, O, _stream())
    _lib.check(rc, "lbbnn_log_softmax_rows")
    return out


def binary_head(logits: torch.Tensor, *, probs: Optional[torch.Tensor] = None, log_probs: bool = False,
                want_probs: bool = True):
    """lbbnn_binary_head on a (B, O <= 16) block of logits with dense rows: the probabilities 1 / (1 + exp(-x)) (a new (B, O)
    tensor, or ``probs`` -- which may be ``logits`` itself) and / or, with ``log_probs`` (O == 1), the (B, 2) log-probabilities
    [logsigmoid(-x), logsigmoid(x)] of the two classes, from the logits in the same launch.  Returns probs, logp2 or the pair."""
    B, O = logits.shape
    if not (want_probs or log_probs):
        raise ValueError("bnn_amd: binary_head has nothing to compute")
    if log_probs and O != 1:
        raise ValueError("bnn_amd: the 2-class log-probabilities of the binary head need one output unit, got %d" % O)
    if want_probs and probs is None:
        probs = torch.empty((B, O), dtype=torch.float32, device=logits.device)
    logp2 = torch.empty((B, 2), dtype=torch.float32, device=logits.device) if log_probs else None
    rc = _lib.lib().lbbnn_binary_head(_ptr_rows(logits, "logits"), logits.stride(0) if B > 1 else O, B, O,
                                      _ptr_rows(probs, "probs") if want_probs else None,
                                      (probs.stride(0) if B > 1 else O) if want_probs else 0,
                                      logp2.data_ptr() if log_probs else None, 2, _stream())
    _lib.check(rc, "lbbnn_binary_head")
    if want_probs and log_probs:
        return probs, logp2
    return probs if want_probs else logp2


def sigmoid_backward(g: torch.Tensor, probs: torch.Tensor) -> torch.Tensor:
    """lbbnn_sigmoid_backward: g * ((1 - p) * p) for (B, O <= 16) tensors."""
    B, O = g.shape
    if g.stride(1) != 1:
        g = g.contiguous()
    out = torch.empty((B, O), dtype=torch.float32, device=g.device)
    rc = _lib.lib().lbbnn_sigmoid_backward(_ptr_rows(g, "g"), g.stride(0) if B > 1 else O, _ptr_rows(probs, "probs"),
                                           probs.stride(0) if B > 1 else O, out.data_ptr(), O, B, O, _stream())
    _lib.check(rc, "lbbnn_sigmoid_backward")
    return out


def structure_descs(lambdals: Sequence[torch.Tensor], layer_ids: Sequence[int]):
    """The lbbnn_structure_desc_t array of a chain of (O, I) fp32 lambdal tensors with dense rows (first layer first), and the
    width lbbnn_gate_structure_width gives it (0: the call would refuse these layers)."""
    n = len(lambdals)
    descs = (_lib.StructureDesc * max(n, 1))()
    for d, lam, lid in zip(descs, lambdals, layer_ids):
        d.lambdal = _ptr_rows(lam, "lambdal")
        d.O, d.I, d.ld, d.layer_id = lam.shape[0], lam.shape[1], (lam.stride(0) if lam.shape[0] > 1 else lam.shape[1]), int(lid)
    return descs, int(_lib.lib().lbbnn_gate_structure_width(descs, n))


def gate_structure(descs, n: int, samples: int, rng: torch.Tensor, *, kept, needed, active, feature_count, unit_count=None,
                   need_out=None):
    """lbbnn_gate_structure on caller-allocated int32 outputs: kept / active (samples, n), needed (samples, n + 1) are written;
    feature_count (I0,) and unit_count (hidden widths, concatenated; nullable) are ADDED TO; need_out: nullable uint8
    (samples, width).  Sample s draws at Philox offset rng[1] + s; the caller advances the state."""
    for name, t, dt in (("kept", kept, torch.int32), ("needed", needed, torch.int32), ("active", active, torch.int32),
                        ("feature_count", feature_count, torch.int32), ("unit_count", unit_count, torch.int32),
                        ("need_out", need_out, torch.uint8)):
        if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
            raise RuntimeError("bnn_amd: %s must be a contiguous %s tensor on a HIP device (no CPU path)" % (name, dt))
    if kept.numel() < samples * n or active.numel() < samples * n or needed.numel() < samples * (n + 1):
        raise ValueError("bnn_amd: gate_structure outputs are smaller than (samples, layers)")
    widths = [descs[0].I] + [descs[l].O for l in range(n)]
    if (feature_count.numel() < widths[0] or (unit_count is not None and unit_count.numel() < sum(widths[1:-1]))
            or (need_out is not None and need_out.numel() < samples * sum(widths))):
        raise ValueError("bnn_amd: gate_structure totals / need_out are smaller than the network's boundaries %s" % (widths,))
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().lbbnn_gate_structure(descs, n, samples, rng.data_ptr(), p(kept), p(needed), p(active),
                                               p(feature_count), p(unit_count), p(need_out), _stream()), "lbbnn_gate_structure")


def _study_fit(entry, args_type, P, lr_cols, *, params, exp_avg, exp_avg_sq, step, rng, skipped, x, y, priors, hyper, lr, restarts,
               history, I, O, batch, first_epoch, n_epochs, **counts):
    """What lrt_study_fit and mnf_study_fit share: the checks of the caller's device tensors, the members the two argument
    structs have in common, the call.  ``P``: the width of a packed row; ``lr_cols``: () for one rate per epoch, (3,) for the
    three rate groups; ``counts``: the struct's further integer members."""
    R, epochs = params.shape[0], history.shape[1]
    checks = [("params", params, torch.float32, (R, P)), ("exp_avg", exp_avg, torch.float32, (R, P)),
              ("exp_avg_sq", exp_avg_sq, torch.float32, (R, P)), ("step", step, torch.float32, (R,)),
              ("rng", rng, torch.int64, (R, 2)), ("skipped", skipped, torch.int64, (R,)),
              ("hyper", hyper, torch.float32, (R, 6)), ("history", history, torch.float64, (R, epochs, _lib.STUDY_HISTORY_COLS)),
              ("x", x, torch.float32, None), ("y", y, torch.float32, None), ("priors", priors, torch.float32, None),
              ("lr", lr, torch.float32, None), ("restarts", restarts, torch.int32, None)]
    for name, t, dt, shape in checks:
        if t is None and name == "restarts":
            continue
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise RuntimeError("bnn_amd: %s must be a contiguous %s tensor%s on a HIP device (no CPU path)"
                               % (name, dt, "" if shape is None else " of shape %s" % (shape,)))
    N = x.shape[-2]
    if x.shape not in ((N, I), (R, N, I)) or y.shape not in ((N, O), (R, N, O)):
        raise ValueError("bnn_amd: x must be (N, I) or (R, N, I) and y (N, O) or (R, N, O), got %s and %s"
                         % (tuple(x.shape), tuple(y.shape)))
    lr_shapes = ((epochs,) + lr_cols, (R, epochs) + lr_cols)
    if priors.shape not in ((1, 5), (R, 5)) or tuple(lr.shape) not in lr_shapes:
        raise ValueError("bnn_amd: priors must be (1 | R, 5) and lr %s or %s" % lr_shapes)
    a = args_type()
    a.params, a.exp_avg, a.exp_avg_sq = params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    a.step, a.rng, a.skipped = step.data_ptr(), rng.data_ptr(), skipped.data_ptr()
    a.x, a.x_rstride = x.data_ptr(), (N * I if x.dim() == 3 else 0)
    a.y, a.y_rstride = y.data_ptr(), (N * O if y.dim() == 3 else 0)
    a.priors, a.priors_rstride = priors.data_ptr(), (1 if priors.shape[0] == R and R > 1 else 0)
    a.hyper, a.lr, a.lr_rstride = hyper.data_ptr(), lr.data_ptr(), (epochs if lr.dim() == 2 + len(lr_cols) else 0)
    n_restarts = 0 if restarts is None else restarts.numel()
    a.restarts, a.n_restarts = (restarts.data_ptr() if n_restarts else None), n_restarts
    a.history = history.data_ptr()
    a.R, a.I, a.O, a.N, a.batch = R, I, O, N, batch
    a.epochs, a.first_epoch, a.n_epochs = epochs, first_epoch, n_epochs
    for k, v in counts.items():
        setattr(a, k, v)
    _lib.check(getattr(_lib.lib(), entry)(ctypes.byref(a), _stream()), entry)


def lrt_study_fit(*, I: int, O: int, **kw):
    """lbbnn_lrt_study_fit on caller-allocated device tensors (bnn_amd.study lays them out), keywords: ``params`` / ``exp_avg`` /
    ``exp_avg_sq`` (R, 3 O I + 2 O) and ``step`` (R) float32, ``rng`` (R, 2) and ``skipped`` (R) int64, ``x`` (N, I) or (R, N, I),
    ``y`` (N, O) or (R, N, O), ``priors`` (1 or R, 5) and ``hyper`` (R, 6) float32 rows of lbbnn_priors_t / lbbnn_adam_hyper_t,
    ``lr`` (epochs) or (R, epochs), ``restarts`` int32 or None, ``history`` (R, epochs, 6) float64, ``batch``, ``first_epoch``,
    ``n_epochs``.  One launch; everything in the first row is updated in place."""
    _study_fit("lbbnn_lrt_study_fit", _lib.StudyArgs, 3 * O * I + 2 * O, (), I=I, O=O, **kw)


def mnf_study_fit(*, I: int, O: int, Tz: int, Tr: int, **kw):
    """lbbnn_mnf_study_fit on caller-allocated device tensors, as ``lrt_study_fit`` with these differences: ``params`` /
    ``exp_avg`` / ``exp_avg_sq`` are (R, P), P = 3 O I + 2 O + 5 I + (Tz + Tr)(2 I + 1), rows in the order of
    ``MNFBayesianLinear._param_list()``; ``lr`` is (epochs, 3) or (R, epochs, 3): the rates of the named tensors, of z_flow and
    of r_flow."""
    _study_fit("lbbnn_mnf_study_fit", _lib.MnfStudyArgs, 3 * O * I + 2 * O + 5 * I + (Tz + Tr) * (2 * I + 1), (3,),
               I=I, O=O, Tz=Tz, Tr=Tr, **kw)


# ----------------------------------------------------------------------------------------- workspaces
class LayerWorkspace:
    """Caller-owned device buffers of one layer, allocated once and reused every forward
    (the C ABI never allocates; fixed addresses also make the launch sequence graph-capturable)."""

    def __init__(self, O: int, I: int, device: torch.device, mnf: bool):
        ld = operand_ld(I)
        f = dict(dtype=torch.float32, device=device)
        self.device = device
        self.e_w = torch.empty((O, ld), **f)
        self.var_w = torch.empty((O, ld), **f)
        self.kl_rows = torch.empty(O, **f)
        self.bias_var = torch.empty(O, **f)
        self.e_scale = torch.ones(O, **f)          # LBBNN_F_F16S row scales (written by the weight pass)
        self.v_scale = torch.ones(O, **f)
        self.kl = torch.zeros((), **f)
        self._bw = None
        if mnf:
            self.act_mu = torch.empty(O, **f)
            self.act_var = torch.empty(O, **f)
            self.z_fwd = torch.empty(I, **f)
            self.z_kl = torch.empty(I, **f)
            self.scal = torch.empty(8, **f)

    def backward_operands(self):
        """fp32 operand pair the backward rebuilds for dX (allocated on first use)."""
        if self._bw is None:
            self._bw = (torch.empty_like(self.e_w), torch.empty_like(self.var_w))
        return self._bw
