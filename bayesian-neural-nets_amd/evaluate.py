"""Ensemble evaluation of a Bayesian network -- what ``test_ensemble`` computes per test batch
(LBBNN-GP-MF-LRT.py:229-272, LBBNN-GP-MF-MNF.py:277-334), minus the script's file output:

* ``outputs[s] = net(data, sample=True)`` for s < samples (each a fused no-grad HIP forward with its own draws),
* ensemble prediction = argmax of the mean log-probability over the samples (``outputs[0:10].mean(0)``),
* posterior-mean prediction = argmax of ``net(data, sample=False)``,
* density[s] = mean of one Bernoulli draw of every layer's inclusion probabilities (``layer.gamma.rsample()``).

The reference's own ``test_ensemble`` also runs unchanged on these modules; this is the batched convenience form.

Baseline LBBNN networks (``base.BayesianNetwork``, LBBNN-GP-MF.py:345-502) take their own batched form, ``base_ensemble``:
one lbbnn_gate_members launch draws every member's gates, weights and biases (the training kernels' streams and counters,
member m at Philox offset live + m), then one mean-only GEMM launch per layer runs all members.  ``gates="mpm"`` selects the
median probability model of ``outofsample(medimod=True)``.  ``predictive_entropy`` is the ``outofsample`` entropy of every
family.

Variational-dropout networks (``vd.BNN``, variational_dropout.py:154-160) take ``vd_ensemble``: theta is shared by every
member, so each layer's operands are formed once, the first layer's two products (same input, same weights for every member)
are computed once and fanned out to all members in its epilogue, and every later layer runs all members in one launch
(lbbnn_vd_gemm_members).  Member m is bitwise the m-th of ``samples`` consecutive ``net(data)`` calls.

LRT and MNF networks also have a *frozen evaluation model*, ``freeze(net, gates="alpha" | "mpm")`` -> ``FrozenNetwork``: a
snapshot of the GEMM operands taken once (lbbnn_frozen_operands), with the gates as trained or thresholded -- the median
probability model of ``outofsample(net, loader, medimod=True)`` (LBBNN-GP-MF-LRT.py:295-314, LBBNN-GP-MF-MNF.py:342-366) --
which the member GEMMs then evaluate without reading the parameters again, and which reports its own density.
``freeze(net, gates, dense=True)`` also takes an MNF network with RNVP / MNF-type z flows (the reference's default): every
member's z through the coupling flows is then ONE lbbnn_flow_dense_members launch for all layers and members.

Baseline networks have a frozen model of their own, ``freeze_base(net, gates="sample" | "mpm", compact=...)`` ->
``FrozenBaseNetwork``: sigma, alpha and the gated means taken once (lbbnn_base_frozen_operands), every member then drawn from
that snapshot (lbbnn_base_frozen_members) at the streams, offsets and counters of ``base_ensemble`` -- a full model's members are
``base_ensemble``'s bit for bit, a compact model's weights the full model's at the rows and columns that stay.
``freeze_base(net, "mpm", sparse=True)`` -> ``SparseFrozenBaseNetwork``: the kept weights alone in CSR, every member's (nnz,)
values drawn at the full network's counters (lbbnn_base_sparse_draw_members: the dense model's member weights bit for bit at
the kept positions) and run by the member layer on stored values (lbbnn_sparse_gather_members); the baseline member has explicit
weights, so ``explain_ensemble`` explains exactly the members this model's ``ensemble`` evaluates.

An LRT / MNF network with ``head="identity"`` (regression) returns raw outputs from every ensemble form above and from its frozen
models; ``ensemble_regression`` / ``RegressionAccumulator`` (lbbnn_eval_regression) are its metrics -- predictive mean, epistemic
and aleatoric variance, mixture log density, PIT -- and the classification tools refuse such a model.  ``ensemble_scores`` /
``RegressionScoreAccumulator`` / ``predict_regression`` (lbbnn_eval_regression_scores) are the same for a noise level per element
or per member -- e.g. a network whose outputs carry their own log-variances -- plus the CRPS and prediction intervals.

``structure_posterior`` (lbbnn_gate_structure) samples the posterior over the sparse architectures of an LRT, MNF or baseline
network: per sample the hard gates of every layer and ``live_structure``'s sweep in one launch -- kept and active-path weights,
needed units, and how often each input feature and hidden unit lies on an active path to some output.

``explain`` (lbbnn_explain_step between mean-only GEMMs) answers the local question for a frozen LRT / MNF model: its
posterior-mean forward is a ReLU chain on fixed operands, so per row the pre-head output is exactly linear in the input, and the
call returns every input's contribution ``J[b, c, i] * x[b, i]``, the bias path and a residual that ties them to the logits;
``ExplanationAccumulator`` / ``explain_batches`` (lbbnn_explain_totals) average them over a pass on the device.
``explain_ensemble`` (lbbnn_sparse_draw_members / _gather_members, lbbnn_explain_seed / _member_stats) explains sampled-weight
members of the sparse median probability model and returns the mean, spread and sign probability of every contribution over them.

``threshold_sweep(net, thresholds)`` -> ``ThresholdSweep`` answers where to prune: the sparse models of up to 16 ascending
thresholds from one count and one pack launch (lbbnn_sparse_count_levels / _pack_levels), evaluated K x S members a layer launch
(lbbnn_sparse_layer_levels) under draws common to the levels; ``sweep_batches`` is the evaluation pass over all of them, and
``sw.model(j)`` hands the chosen level on as a ``SparseFrozenNetwork``.
"""
import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import ops


def _head_of(net) -> str:
    return getattr(net, "head", "log_softmax")


def _check_log_probs(net, log_probs: bool):
    """``log_probs=True`` is the 2-class form of a sigmoid head with ONE output unit."""
    if not log_probs:
        return
    if _head_of(net) == "identity":
        raise ValueError("bnn_amd: log_probs=True applies to a head=\"sigmoid\" network; an identity head returns raw outputs "
                         "(regression) and has no log-probabilities")
    if _head_of(net) != "sigmoid":
        raise ValueError("bnn_amd: log_probs=True applies to a head=\"sigmoid\" network (a log_softmax head returns "
                         "log-probabilities already)")
    if net.dims[-1] != 1:
        raise ValueError("bnn_amd: log_probs=True needs one output unit (the two classes of a binary outcome), this head has %d"
                         % net.dims[-1])


def _binary_members(buf: torch.Tensor, S: int, B: int, O: int, log_probs: bool) -> torch.Tensor:
    """The binary head over the (S, member stride) logits buffer of a member GEMM, member m's (B, O) block at buf[m, :B * O]: ONE
    lbbnn_binary_head launch over the whole buffer as a column of single elements (the function is elementwise; the padding
    between members is computed and never shown).  Probabilities in place -> (S, B, O); ``log_probs`` (O == 1) -> the (S, B, 2)
    log-probabilities, a view with the buffer's member stride."""
    ms = buf.shape[1]
    flat = buf.view(S * ms, 1)
    if log_probs:
        return ops.binary_head(flat, log_probs=True, want_probs=False).view(S, ms, 2)[:, :B]
    ops.binary_head(flat, probs=flat)
    return buf[:, :B * O].view(S, B, O)


def _members_result(buf: torch.Tensor, S: int, B: int, C: int, head: str, log_probs: bool) -> torch.Tensor:
    """The (S, >= pad4(B * C)) buffer the last member GEMM wrote as the (S, B, C) result: the sigmoid head's one launch, a view
    where the GEMM applied log_softmax itself (C <= 16), torch's log_softmax otherwise."""
    if head == "sigmoid":
        return _binary_members(buf, S, B, C, log_probs)
    outputs = buf[:, :B * C].view(S, B, C)
    if head == "identity":
        return outputs                                      # the raw outputs: the sigmoid head minus its launch
    return outputs if C <= 16 else torch.log_softmax(outputs, dim=-1)


def _member_counts(samples, max_members):
    """(S, chunk) of an ensemble call: the members, and how many of them one launch takes (default: all)."""
    S = int(samples)
    if S < 1:
        raise ValueError("bnn_amd: samples must be >= 1")
    chunk = S if max_members is None else int(max_members)
    if chunk < 1:
        raise ValueError("bnn_amd: max_members must be >= 1")
    return S, chunk


def _forward_head(net, data, sample: bool, log_probs: bool):
    """net(data, sample) of an LRT / MNF network; with ``log_probs`` the sigmoid head's 2-class log-probabilities."""
    if not log_probs:
        return net(data, sample=sample)
    net._logp2_now = True
    try:
        return net(data, sample=sample)
    finally:
        net._logp2_now = False


def _batched_ok(net, data) -> bool:
    """The one-launch-per-kernel ensemble applies to LRT networks and to MNF networks whose flows are planar with <= 4
    transforms, on a HIP device, without injected noise; anything else takes the loop of single forwards."""
    from . import layers as L
    if not isinstance(net, L._NetworkBase) or not data.is_cuda:
        return False
    for l in net._layers():
        if l.noise or getattr(l, "as_written", False):
            return False
        if l._mnf and (l._check_flows() != "planar" or len(l.z_flow.transforms) > 4):
            return False
        if l.in_features % 4 or ops.operand_ld(l.in_features) > 2048:
            return False
    return True


@torch.no_grad()
def ensemble_forward_batched(net, data: torch.Tensor, samples: int = 10, *, log_probs: bool = False) -> torch.Tensor:
    """``samples`` stochastic evaluation forwards of one batch (LBBNN-GP-MF-MNF.py:286-294: TEST_SAMPLES x net(data,
    sample=True)) in 2 + 3 launches instead of 5 per member: one K3 and one K1 launch produce every member's z and
    operands (the variance operand, z-free, once for all), then each layer's GEMM runs all members as gridDim.z slices of
    ONE launch (lbbnn_lrt_gemm_members) -- member m draws at Philox offset (live offset + m), exactly where the m-th of
    ``samples`` consecutive ``net(data, sample=True)`` calls would, so the result is bit-identical to that loop
    (tests/test_parity_gpu.py::test_ensemble_batched_equals_loop_bitwise) under the fp32 and bf16x3 settings.  The member
    dimension exists in the bf16 hi | lo operand format only: under "fp16x3" / "fp16x3f" the batched form still multiplies in
    bf16x3 (2.7e-6 of max|out| against fp64, tighter than fp16x3f's 1.4e-5) while the loop's single forwards take the
    row-scaled fp16 kernels -- same draws, results equal to the formats' error (tools/ensemble_fuzz.py)."""
    import ctypes
    from . import _lib
    _check_log_probs(net, log_probs)
    net.eval()
    S = int(samples)
    layers = net._layers()
    n = len(layers)
    x = data.view(-1, net.dims[0])
    x = x.float() if x.dtype != torch.float32 else x
    if x.stride(1) != 1:
        x = x.contiguous()
    B, dev = x.shape[0], x.device
    st = ops.RngState.get(dev)
    rng = st.t
    f = dict(dtype=torch.float32, device=dev)
    descs = (_lib.LayerDesc * n)()
    keep, chain, z_all = [], [], []
    for i, l in enumerate(layers):
        cfg = (True, False, i < n - 1)
        # (the member dimension of the batched ensemble exists in the bf16 hi | lo format: any 16-bit precision selects it)
        l._split_now = int(bool(l._split(x if i == 0 else None)) and (i == 0 or layers[i - 1].out_features % 4 == 0))
        keep.append(l._fill_desc(descs[i], cfg, None))
        ld = ops.operand_ld(l.in_features)
        e, ws = torch.empty((S, l.out_features, ld), **f), l._workspace()
        chain.append((e, l.bias_mu, l._split_now, ws.var_w, ws.bias_var, ops.STREAM_EPS_OUT * 64 + l._layer_id, l.row_offset))
        descs[i].e_w = e.data_ptr()
        if l._mnf:
            z = torch.empty((S, ld), **f)
            z_all.append(z)
            descs[i].z_fwd = z.data_ptr()
        descs[i].eps_z = None
    stream = torch.cuda.current_stream(dev).cuda_stream
    for k, cnt in _lib.layer_groups(n):                        # (every group reads the same live offset; advanced once, below)
        _lib.check(_lib.lib().lbbnn_ensemble_operands(_lib.group_slice(descs, k, cnt), cnt, S, rng.data_ptr(), 1, stream),
                   "lbbnn_ensemble_operands")
    C = layers[-1].out_features
    obuf = ops.member_gemm_chain(x, S, chain, head=_head_of(net), out=torch.empty((S, ops.pad4(B * C)), **f), rng=rng,
                                 stream=stream)
    st.advance(S)                                              # as S single forwards would have
    for l in layers:
        l.kl = 0
    net._kl_total = None
    del keep
    return _members_result(obuf, S, B, C, _head_of(net), log_probs)


def _has_dense_flows(net) -> bool:
    from . import layers as L
    return isinstance(net, L._NetworkBase) and any(l._mnf and l._check_flows() == "dense" for l in net._layers())


def _is_vd(net) -> bool:
    from . import vd
    return isinstance(net, vd.BNN)


def _vd_check(net, data, samples, max_members):
    if not _is_vd(net):
        raise ValueError("bnn_amd: vd_ensemble takes a variational-dropout network (bnn_amd.vd.BNN)")
    return _member_counts(samples, max_members)


@torch.no_grad()
def vd_ensemble(net, data: torch.Tensor, samples: int = 10, *, max_members: Optional[int] = None) -> torch.Tensor:
    """(samples, B, classes) log-probabilities of ``samples`` forwards of a variational-dropout network
    (variational_dropout.py:154-160: ``all_predictions[x] = model(images)``), bitwise the loop of ``samples`` consecutive
    ``net(data)`` calls, in chunks of at most ``max_members`` members (default: all; chunked and unchunked results are the same
    bits).  Per chunk: one lbbnn_vd_operands per layer (theta is shared), the first layer ONCE with its epilogue writing every
    member (fan-out), each later layer one launch for all members, and the log_softmax of ``BNN.forward``.  A single forward
    advances the live Philox offset by 1 after each of its L layers, so member m's layer i draws at offset live + L*m + i here
    too (member_advance = L); the live offset ends at live + L*samples.  Per layer the kernel (split or not, SINGLE16,
    HALF16) is the one ``BayesianLayer._forward_hip`` picks for that member's input.  Injected noise (``layer.noise``) is
    not supported here (ValueError): the loop form of ``ensemble_forward(batched=False)`` takes it."""
    S, chunk = _vd_check(net, data, samples, max_members)
    layers = net._layers()
    if any(l.noise for l in layers):
        raise ValueError("bnn_amd: vd_ensemble draws in-kernel noise; a layer has injected noise (use batched=False)")
    if not data.is_cuda:
        raise RuntimeError("bnn_amd: ensemble evaluation needs a HIP device tensor (data is on %s); there is no CPU path"
                           % data.device)
    net.eval()
    L = len(layers)
    x = data.view(-1, net.dims[0]).float()                    # as BNN.forward / BayesianLayer.forward
    B, C, dev = x.shape[0], net.dims[-1], x.device
    st = ops.RngState.get(dev)
    f = dict(dtype=torch.float32, device=dev)
    head = torch.empty((S, ops.pad4(B * C)), **f)              # member strides padded to 16 B
    outputs = head[:, :B * C].view(S, B, C)
    if B == 0:
        st.advance(L * S)
        return torch.log_softmax(outputs, dim=-1)
    single = ops.get_precision() in ("bf16", "fp16")          # as ops.lrt_gemm reads it
    for m0 in range(0, S, chunk):
        c = min(chunk, S - m0)
        h = x
        for i, l in enumerate(layers):
            # the kernel choice of the loop: _forward_hip decides on member 0's input rows, and every member's rows have the
            # same stride and 16-B alignment (the padded member stride)
            split, half = l._arith(h if i == 0 else h[0])
            if i == 0 and (x.stride(1) != 1 or x.stride(0) < l.n):
                h = x.contiguous()                            # (what ops.lrt_gemm does with such rows, after the choice)
            e_w, var_w = l._operands(split, half)
            last = i == L - 1
            out = outputs[m0:m0 + c] if last else torch.empty((c, ops.pad4(B * l.m)), **f)[:, :B * l.m].view(c, B, l.m)
            ops.vd_gemm_members(h, e_w, var_w, l.alpha, st.t, I=l.n, O=l.m, members=c, fanout=i == 0,
                                rng_stream=ops.STREAM_EPS_OUT * 64 + l._layer_id, row_offset=l.row_offset,
                                member_advance=L, relu=not last, split=split, single=split and single, half=half, out=out)
            st.advance(1)                                     # layer i + 1 draws at the next offset, as in the loop
            h = out
        if c > 1:
            st.advance(L * (c - 1))                           # the other members' offsets
    return torch.log_softmax(outputs, dim=-1)


def _is_base(net) -> bool:
    from . import base
    return isinstance(net, base.BayesianNetwork)


@torch.no_grad()
def base_ensemble(net, data: torch.Tensor, samples: int = 10, *, gates: str = "sample", max_members: Optional[int] = None,
                  keep_gates: bool = False, log_probs: bool = False) -> Dict[str, object]:
    """``samples`` evaluation forwards of a baseline LBBNN network of n layers in ceil(n / 4) + n launches (1 + 3 for the
    reference's three layers) per chunk of at most ``max_members`` members (default: all in one).  Member m draws at
    Philox offset (live offset + m) and equals, bit for bit, what
    ``net.sample_predict`` / the layers' ``sample_forward`` compute at that offset; chunked and unchunked results are the same
    bits.  The live offset advances by ``samples``.  Returns ``outputs`` (samples, B, classes) log-probabilities,
    ``gate_rows`` (per layer (samples, O): the sum over each row of the gates the member used) and, with ``keep_gates``,
    ``gates`` (per layer (samples, O, I)).  A network with a layer wider than lbbnn_gate_members takes
    (``ops.operand_ld(in_features) > ops.GATE_MEMBERS_MAX_LD``) runs each member as its ``sample_forward`` chain instead
    (``BayesianNetwork._predict_members_loop``; ``gates="mpm"`` raises there).  A network with ``head="sigmoid"``: ``outputs``
    are the (samples, B, units) probabilities, or with ``log_probs`` (one unit) the (samples, B, 2) log-probabilities
    [logsigmoid(-logit), logsigmoid(logit)]; one lbbnn_binary_head launch more per chunk, same draws and offsets."""
    if not _is_base(net):
        raise ValueError("bnn_amd: base_ensemble takes a baseline LBBNN network (bnn_amd.base.BayesianNetwork)")
    _check_log_probs(net, log_probs)
    if not data.is_cuda:
        raise RuntimeError("bnn_amd: ensemble evaluation needs a HIP device tensor (data is on %s); there is no CPU path"
                           % data.device)
    S, chunk = _member_counts(samples, max_members)
    net.eval()
    B, C = data.reshape(-1, net.dims[0]).shape[0], net.dims[-1]
    st = ops.RngState.get(data.device)
    head = torch.empty((S, ops.pad4(B * C)), dtype=torch.float32, device=data.device)        # 16-B aligned member rows
    rows, kept, outs = [], [], []
    for m0 in range(0, S, chunk):
        c = min(chunk, S - m0)
        o, r, g = net._predict_members(data, st.t, c, gates, out=head[m0:m0 + c], rows=True, keep_gates=keep_gates,
                                       log_probs=log_probs)
        st.advance(c)
        outs.append(o)
        rows.append(r)
        kept.append(g)
    if C <= 16 and not log_probs:
        outputs = head[:, :B * C].view(S, B, C)             # the chunks wrote their log-probabilities into `head`
    else:
        outputs = outs[0] if len(outs) == 1 else torch.cat(outs)
    cat = lambda parts: [p[0] if len(parts) == 1 else torch.cat(p) for p in zip(*parts)]
    return {"outputs": outputs, "gate_rows": cat(rows), "gates": cat(kept) if keep_gates else None}


@torch.no_grad()
def ensemble_forward(net, data: torch.Tensor, samples: int = 10, batched=None, *, gates: str = "sample",
                     max_members: Optional[int] = None, log_probs: bool = False) -> torch.Tensor:
    """(samples, B, classes) log-probabilities of ``samples`` stochastic forwards (net left in eval mode).
    ``batched``: None = the one-launch-per-kernel form when the network qualifies (``_batched_ok``; a baseline network on a
    HIP device: ``base_ensemble``), else the loop of fused single forwards (``net.sample_predict`` for a baseline network);
    True / False force one of them (True on an MNF network with RNVP / MNF-type z flows: ``freeze(net, "alpha",
    dense=True).ensemble`` -- the loop's draws, results equal to rounding).  Either form advances the live Philox offset by
    ``samples``.
    ``gates`` ("sample" or "mpm") applies to baseline networks only, ``max_members`` (members per launch of the batched form)
    to baseline and variational-dropout networks and frozen models.  A ``FrozenNetwork`` (``freeze``): its ``ensemble``.
    A variational-dropout network (``vd.BNN``): None = ``vd_ensemble`` on a
    HIP device when no layer has injected noise, else the loop of ``net(data)``; True with injected noise raises ValueError.
    A network with ``head="sigmoid"`` (LRT / MNF, its frozen model, or a baseline network): (samples, B, units) PROBABILITIES, same draws and Philox
    offsets (the head consumes no randomness); ``log_probs=True`` (one unit) returns the (samples, B, 2) log-probabilities
    [logsigmoid(-logit), logsigmoid(logit)] instead, made from the logits by the same launch.
    A network with ``head="identity"`` (LRT / MNF or its frozen model): (samples, B, units) RAW outputs, the same draws and
    offsets, no head launch; ``log_probs=True`` is a ValueError."""
    net.eval()
    if log_probs and (_is_vd(net) or (_is_base(net) and _head_of(net) != "sigmoid")):
        raise ValueError("bnn_amd: log_probs=True applies to a network with head=\"sigmoid\" or its frozen model")
    if _is_frozen(net):
        if gates != "sample":
            raise ValueError("bnn_amd: gates=%r: the gates of a frozen model were fixed by evaluate.freeze(net, gates=...) "
                             "(this one has gates=%r); freeze again to change them" % (gates, net.gates))
        if batched is False:
            raise ValueError("bnn_amd: a frozen model has no loop-of-forwards form; leave batched at None")
        return net.ensemble(data, samples, max_members=max_members, log_probs=log_probs)
    if _is_vd(net):
        if gates != "sample":
            raise ValueError("bnn_amd: gates=%r (the median probability model) exists for baseline LBBNN networks only"
                             % (gates,))
        _vd_check(net, data, samples, max_members)
        noisy = any(l.noise for l in net._layers())
        if batched is None:
            batched = data.is_cuda and not noisy
        if batched:
            return vd_ensemble(net, data, samples, max_members=max_members)
        return torch.stack([net(data) for _ in range(int(samples))])
    if _is_base(net):
        if gates not in ("sample", "mpm"):
            raise ValueError("bnn_amd: gates must be 'sample' or 'mpm', got %r" % (gates,))
        if batched is None:
            batched = data.is_cuda
        if batched:
            return base_ensemble(net, data, samples, gates=gates, max_members=max_members, log_probs=log_probs)["outputs"]
        return torch.stack([net.sample_predict(data, gates=gates, log_probs=log_probs) for _ in range(samples)])
    if gates != "sample":
        raise ValueError("bnn_amd: gates=%r is not an option of ensemble_forward for an LRT / MNF network; the median "
                         "probability model of such a network is evaluate.freeze(net, gates=\"mpm\").ensemble(data, samples)"
                         % (gates,))
    if max_members is not None:
        raise ValueError("bnn_amd: max_members applies to baseline LBBNN networks only")
    _check_log_probs(net, log_probs)
    if batched is None:
        batched = _batched_ok(net, data)
    if batched and _has_dense_flows(net):
        # RNVP / MNF-type z flows: the batched form is the frozen alpha model (same draws as the loop, equal to rounding);
        # batched=None keeps the loop for such a network
        return freeze(net, "alpha", dense=True).ensemble(data, samples, log_probs=log_probs)
    if batched:
        return ensemble_forward_batched(net, data, samples, log_probs=log_probs)
    outs = [_forward_head(net, data, True, log_probs) for _ in range(samples)]
    return torch.stack(outs)


@torch.no_grad()
def ensemble_eval(net, data: torch.Tensor, target: Optional[torch.Tensor] = None, samples: int = 10) -> Dict[str, object]:
    """test_ensemble's numbers for one batch: ``outputs``, ``pred_ensemble``, ``pred_posterior_mean``, ``density`` (and
    ``correct_*`` with a target).  Frozen models (``freeze``): the same keys, ``pred_posterior_mean`` from
    ``frozen(data, sample=False)`` and ``density`` = ``samples`` copies of ``frozen.density`` (fixed gates are not resampled).
    Variational-dropout networks: ``outputs``, ``pred_ensemble``, and ``loss`` and
    ``correct_ensemble`` with a target (``_vd_ensemble_eval``).  Baseline networks: ``density[s]`` is the mean gate of member s over all weights -- the gates
    the member actually used (the reference draws a separate set, LBBNN-GP-MF.py:390-394) -- and the posterior mean is the
    mode-2 forward (weight = alpha * mu) with alpha = sigmoid(lambdal) set as the reference sets it (:369-374, :413)."""
    if _is_frozen(net):
        return _frozen_ensemble_eval(net, data, target, samples)
    if _is_base(net):
        return _base_ensemble_eval(net, data, target, samples)
    if _is_vd(net):
        return _vd_ensemble_eval(net, data, target, samples)
    binary = _binary_eval(net)
    if binary and target is not None:
        target = _binary_target(target)
    outputs = ensemble_forward(net, data, samples, log_probs=binary)
    density = []
    for _ in range(samples):
        g = [l.gamma.rsample().flatten() for l in net._layers()]
        density.append(torch.cat(g).mean())
    pred_ens = outputs.mean(0).argmax(1)
    pred_mean = _forward_head(net, data, False, binary).argmax(1)
    res = {"outputs": outputs, "pred_ensemble": pred_ens, "pred_posterior_mean": pred_mean,
           "density": torch.stack(density)}
    if target is not None:
        res["correct_ensemble"] = int(pred_ens.eq(target).sum())
        res["correct_posterior_mean"] = int(pred_mean.eq(target).sum())
    return res


_NOT_CLASSIFICATION = ("bnn_amd: this model has head=\"identity\" (regression): ensemble_eval, predictive_entropy, EvalAccumulator "
                       "and UncertaintyAccumulator are classification tools; use evaluate.RegressionAccumulator")


def _binary_eval(net) -> bool:
    """A sigmoid head is evaluated as two classes: its one unit's (.., 2) log-probabilities go to the metrics of a ``classes =
    2`` problem.  More than one unit (multi-label) has no class axis: ValueError."""
    if _head_of(net) == "identity":
        raise ValueError(_NOT_CLASSIFICATION)
    if _head_of(net) != "sigmoid":
        return False
    if net.dims[-1] != 1:
        raise ValueError("bnn_amd: the evaluation metrics take a sigmoid head with ONE output unit as a 2-class problem; this "
                         "head has %d units (multi-label): use the probabilities of ensemble_forward directly" % net.dims[-1])
    return True


def _binary_target(target: torch.Tensor) -> torch.Tensor:
    """0 / 1 targets of a binary head, given as float or integer, (B,) or (B, 1): the (B,) int64 class ids, on the device."""
    t = target.reshape(-1)
    return t if t.dtype == torch.int64 else t.long()


def _frozen_ensemble_eval(net, data, target, samples):
    binary = _binary_eval(net)
    if binary and target is not None:
        target = _binary_target(target)
    outputs = net.ensemble(data, samples, log_probs=binary)
    pred_ens = outputs.mean(0).argmax(1)
    pred_mean = net(data, sample=False, log_probs=binary).argmax(1)
    density = torch.full((int(samples),), net.density, dtype=torch.float32, device=outputs.device)
    res = {"outputs": outputs, "pred_ensemble": pred_ens, "pred_posterior_mean": pred_mean, "density": density}
    if target is not None:
        res["correct_ensemble"] = int(pred_ens.eq(target).sum())
        res["correct_posterior_mean"] = int(pred_mean.eq(target).sum())
    return res


def _vd_ensemble_eval(net, data, target, samples):
    """Variational dropout's validation numbers (variational_dropout.py:154-174): ``outputs``, ``pred_ensemble`` = argmax of
    ``outputs.mean(0)`` and, with a target, ``loss`` = ``vd.loss_fn(outputs.mean(0), target, net)`` and ``correct_ensemble``.
    No ``pred_posterior_mean`` or ``density``: the reference's VD script computes neither."""
    from . import vd
    outputs = ensemble_forward(net, data, samples)
    mean = outputs.mean(0)
    pred_ens = mean.argmax(1)
    res = {"outputs": outputs, "pred_ensemble": pred_ens}
    if target is not None:
        res["loss"] = vd.loss_fn(mean, target, net)
        net.eval()                                            # (loss_fn's `model.train()` call, :91)
        res["correct_ensemble"] = int(pred_ens.eq(target).sum())
    return res


def _base_mean_forward(net, data, binary: bool):
    """The posterior-mean forward of a baseline network (mode 2: weight = alpha * mu, LBBNN-GP-MF.py:413) with alpha =
    sigmoid(lambdal) set as the reference sets it (:369-374); ``binary``: the sigmoid head's 2-class log-probabilities."""
    layers = net._layers()
    for l in layers:
        l.alpha = 1 / (1 + torch.exp(-l.lambdal.detach()))
        l.gamma.alpha = l.alpha
    net._logp2_now = bool(binary)
    try:
        return net(data, *[None] * len(layers), sample=False)
    finally:
        net._logp2_now = False


def _base_ensemble_eval(net, data, target, samples):
    binary = _binary_eval(net)
    if binary and target is not None:
        target = _binary_target(target)
    r = base_ensemble(net, data, samples, log_probs=binary)
    outputs = r["outputs"]
    layers = net._layers()
    n_w = sum(l.out_features * l.in_features for l in layers)
    density = torch.stack([rw.double().sum(1) for rw in r["gate_rows"]]).sum(0) / n_w
    pred_mean = _base_mean_forward(net, data, binary).argmax(1)
    pred_ens = outputs.mean(0).argmax(1)
    res = {"outputs": outputs, "pred_ensemble": pred_ens, "pred_posterior_mean": pred_mean, "density": density.float()}
    if target is not None:
        res["correct_ensemble"] = int(pred_ens.eq(target).sum())
        res["correct_posterior_mean"] = int(pred_mean.eq(target).sum())
    return res


@torch.no_grad()
def predictive_entropy(outputs: torch.Tensor) -> torch.Tensor:
    """Per-row entropy of the ensemble's predictive distribution as ``outofsample`` computes it (LBBNN-GP-MF.py:476-496,
    LBBNN-GP-MF-LRT.py:318-334): per member sigmoid(log-probabilities) normalised over the classes of each row, the mean over
    the members, then -sum p log p per row.  ``outputs``: (samples, B, classes); returns (B,).  Any family."""
    if not torch.is_tensor(outputs) and _head_of(outputs) == "identity":
        raise ValueError(_NOT_CLASSIFICATION)
    if outputs.dim() != 3:
        raise ValueError("bnn_amd: outputs must be (samples, B, classes), got %s" % (tuple(outputs.shape),))
    p = torch.sigmoid(outputs.float())
    p = p / p.sum(-1, keepdim=True)
    m = p.mean(0)
    return -(m * torch.log(m)).sum(-1)


# ----------------------------------------------------------------------------------------- metrics on the device
def _dense_rows(t: torch.Tensor, rows: int, cols: int):
    """(tensor, row stride) of a (rows, cols) fp32 view the metrics kernel reads in place, or of its contiguous copy."""
    ld = t.stride(0) if rows > 1 else cols
    if (cols > 1 and t.stride(1) != 1) or ld < cols:
        t, ld = t.contiguous(), cols
    return t, ld


def _member_block(outputs: torch.Tensor, who: str):
    """(tensor, S, B, C, member stride, row stride) of the (samples, B, classes) fp32 block the metrics kernels read in place: any
    HIP tensor whose last dimension is dense and whose members do not overlap, else its contiguous copy."""
    if outputs.dim() != 3:
        raise ValueError("bnn_amd: outputs must be (samples, B, classes), got %s" % (tuple(outputs.shape),))
    if not outputs.is_cuda:
        raise RuntimeError("bnn_amd: %s needs a HIP device tensor (outputs is on %s); there is no CPU path"
                           % (who, outputs.device))
    S, B, C = outputs.shape
    if not 1 <= C <= 64:
        raise ValueError("bnn_amd: %s takes 1 to 64 classes, got %d" % (who, C))
    if not 1 <= S <= 65535:
        raise ValueError("bnn_amd: %s takes 1 to 65535 members, got %d" % (who, S))
    o = outputs if outputs.dtype == torch.float32 else outputs.float()
    ldp = o.stride(1) if B > 1 else C
    ms = o.stride(0) if S > 1 else 0
    if (C > 1 and o.stride(2) != 1) or ldp < C or (S > 1 and B > 0 and ms < (B - 1) * ldp + C):
        o, ldp, ms = o.contiguous(), C, B * C
    return o, S, B, C, ms, ldp


def _target_rows(target: torch.Tensor, B: int, dev) -> torch.Tensor:
    """``target`` as the dense (B,) int64 tensor the metrics kernels read."""
    if tuple(target.shape) != (B,) or target.device != dev:
        raise ValueError("bnn_amd: target must be (%d,) on %s, got %s on %s" % (B, dev, tuple(target.shape), target.device))
    t = target if target.dtype == torch.int64 else target.long()
    return t if (B < 2 or t.stride(0) == 1) else t.contiguous()


def _mean_rows(mean_outputs: torch.Tensor, B: int, C: int, dev):
    """(tensor, row stride) of the (B, C) posterior-mean outputs as the metrics kernels read them."""
    if tuple(mean_outputs.shape) != (B, C) or mean_outputs.device != dev:
        raise ValueError("bnn_amd: mean_outputs must be (%d, %d) on %s, got %s on %s"
                         % (B, C, dev, tuple(mean_outputs.shape), mean_outputs.device))
    return _dense_rows(mean_outputs if mean_outputs.dtype == torch.float32 else mean_outputs.float(), B, C)


def _launch(dev, name: str, *args):
    """``_lib.launch`` with ``dev`` the current device for the call."""
    from . import _lib
    with torch.cuda.device(dev):
        _lib.launch(dev, name, *args)


class _DeviceTotals:
    """What the accumulators share: ``_totals``, one int64 device buffer read in one copy (doubles as bit patterns); ``_work``,
    the kernels' partials, grown to the largest batch; ``updates``; and the refusals every update and result repeat."""
    _width = "classes"                       # the attribute that, with ``samples``, is fixed for the accumulator's life

    def _start(self, words: int, device):
        self.device = torch.device(device)
        self._totals = torch.zeros(words, dtype=torch.int64, device=self.device)
        self._work = None
        self.reset()

    def reset(self):
        self._totals.zero_()
        self.updates = 0

    def _note(self, with_mean: bool = False):
        self.updates += 1

    def _read(self):
        """The totals as a host int64 array (the one device-to-host copy)."""
        return self._totals.cpu().numpy()

    def _host(self):
        import numpy as np
        return np.ascontiguousarray(self._read(), dtype=np.int64)

    def _check_batch(self, S: int, W: int, dev):
        if (S, W) != (self.samples, getattr(self, self._width)):
            raise ValueError("bnn_amd: this %s was built for %d members and %d %s, the outputs have %d and %d"
                             % (type(self).__name__, self.samples, getattr(self, self._width), self._width, S, W))
        if dev != self._totals.device:
            raise ValueError("bnn_amd: the outputs are on %s, the accumulator on %s" % (dev, self._totals.device))

    def _work_ptr(self, need: int) -> int:
        """The address of at least ``need`` bytes of work memory."""
        if self._work is None or self._work.numel() * 8 < need:
            self._work = torch.empty(int(need) // 8, dtype=torch.float64, device=self._totals.device)
        return self._work.data_ptr()

    @staticmethod
    def _refuse_bad_targets(res, strict: bool, what: str):
        if strict and res["bad_targets"]:
            raise IndexError("bnn_amd: %d target(s) %s in this evaluation pass" % (res["bad_targets"], what))


class _MeanTotals(_DeviceTotals):
    """Totals whose updates may carry posterior-mean outputs: ``posterior_mean_updates`` counts those that did."""

    def reset(self):
        super().reset()
        self.posterior_mean_updates = 0

    def _note(self, with_mean: bool = False):
        self.updates += 1
        self.posterior_mean_updates += int(with_mean)


@torch.no_grad()
def ensemble_metrics(outputs: torch.Tensor, target: Optional[torch.Tensor] = None,
                     mean_outputs: Optional[torch.Tensor] = None, *, acc: Optional["EvalAccumulator"] = None) -> Dict[str, object]:
    """The per-row numbers of the reference's evaluation loops from one (samples, B, classes) block of log-probabilities, in
    ONE lbbnn_eval_metrics call (1 launch; 2 with ``acc``) and without a host synchronisation:

    * ``mean_log_probs`` (B, classes): the mean over the members (test_ensemble's ``outputs.mean(0)``,
      LBBNN-GP-MF-MNF.py:312-315), summed in member order in fp32 and divided by ``samples`` -- a fixed arithmetic
      (include/lbbnn.h), so the values and everything derived from them are reproducible bit for bit on the CPU;
    * ``pred_ensemble`` (B,) int64: its argmax by numpy.argmax's rule (NaN is the maximum, the lowest index wins a tie);
    * ``pred_posterior_mean`` (B,) int64 when ``mean_outputs`` (B, classes), the posterior-mean forward, is given;
    * ``entropy`` (B,): ``predictive_entropy(outputs)`` (outofsample, :370-392) computed in the same pass.

    ``outputs`` is any fp32 HIP tensor whose last dimension is dense -- the strided views ``FrozenNetwork.ensemble`` /
    ``base_ensemble`` / ``vd_ensemble`` return are read in place; classes <= 64.  ``target`` (B,) int64 matters with ``acc``
    only: an ``EvalAccumulator`` whose running totals this call adds to (``EvalAccumulator.update`` is this call)."""
    import ctypes
    from . import _lib
    o, S, B, C, ms, ldp = _member_block(outputs, "ensemble_metrics")
    dev = outputs.device
    a = _lib.EvalMetricsArgs()
    a.logp, a.m_stride, a.ldp, a.S, a.B, a.C = o.data_ptr(), ms, ldp, S, B, C
    keep = [o]
    if mean_outputs is not None:
        mo, a.ldm = _mean_rows(mean_outputs, B, C, dev)
        a.mean_logp = mo.data_ptr()
        keep.append(mo)
    if target is not None:
        t = _target_rows(target, B, dev)
        a.target = t.data_ptr()
        keep.append(t)
    # the per-row outputs as one allocation: [pred_ensemble | pred_posterior_mean] int64, then [mean_log_probs | entropy] fp32
    buf = torch.empty(2 * B + (B * C + B + 1) // 2, dtype=torch.int64, device=dev)
    fl = buf[2 * B:].view(torch.float32)
    res = {"mean_log_probs": fl[:B * C].view(B, C), "pred_ensemble": buf[:B], "entropy": fl[B * C:B * C + B]}
    a.ens_logp, a.pred_ensemble, a.entropy = fl.data_ptr(), buf.data_ptr(), fl.data_ptr() + 4 * B * C
    if mean_outputs is not None:
        res["pred_posterior_mean"] = buf[B:2 * B]
        a.pred_mean = buf.data_ptr() + 8 * B
    if acc is not None:
        acc._fill(a, S, B, C, dev)
    if B > 0:                                                # (an empty batch has no storage to point at, and nothing to add)
        _launch(dev, "lbbnn_eval_metrics", ctypes.byref(a))
    if acc is not None:
        acc._note(mean_outputs is not None)
    del keep
    return res


class EvalAccumulator(_MeanTotals):
    """Running totals of an evaluation pass, kept on the device: ``update`` adds a batch (no host read), ``result`` reads them
    -- the ONLY synchronisation of a pass.  What the reference's loops accumulate on the host with an ``.item()`` per batch:
    test_ensemble's two correct counts (LBBNN-GP-MF-MNF.py:316-323), outofsample's per-member ``corrects``, ensemble correct
    count and entropies (:370-392), VD's validation nll sum, correct count and confusion matrix
    (variational_dropout.py:160-176).  ``classes`` <= 64 and ``samples`` are fixed for the accumulator's life."""

    def __init__(self, classes: int, samples: int, device):
        from . import _lib
        C, S = int(classes), int(samples)
        if not 1 <= C <= 64:
            raise ValueError("bnn_amd: EvalAccumulator takes 1 to 64 classes, got %d" % C)
        if not 1 <= S <= 65535:
            raise ValueError("bnn_amd: EvalAccumulator takes 1 to 65535 members, got %d" % S)
        self.classes, self.samples = C, S
        # one buffer, one read: counts | correct_member | confusion | the two double sums (bit patterns)
        self._start(_lib.EVAL_COUNTS + S + C * C + 2, device)

    def _fill(self, a, S, B, C, dev):
        """Point the totals of an lbbnn_eval_metrics_args_t at this accumulator (work memory grows to the largest batch)."""
        from . import _lib
        self._check_batch(S, C, dev)
        a.work = self._work_ptr(_lib.lib().lbbnn_eval_metrics_work_bytes(S, B, C))
        n, base = _lib.EVAL_COUNTS, self._totals.data_ptr()
        a.counts, a.correct_member, a.confusion, a.sums = base, base + 8 * n, base + 8 * (n + S), base + 8 * (n + S + C * C)

    def update(self, outputs: torch.Tensor, target: Optional[torch.Tensor], mean_outputs: Optional[torch.Tensor] = None):
        """``ensemble_metrics(outputs, target, mean_outputs)`` of one batch, its numbers added to the totals."""
        return ensemble_metrics(outputs, target, mean_outputs, acc=self)

    def result(self, strict: bool = True) -> Dict[str, object]:
        """Python numbers: ``rows``, ``rows_with_target``, ``bad_targets``, ``correct_ensemble``, ``correct_posterior_mean``,
        ``entropy_nonfinite``, ``nll_sum`` (``F.nll_loss(outputs.mean(0), target, reduction="sum")`` over the pass),
        ``entropy_sum`` (over the rows with a finite entropy); ``correct_member`` (samples,) and ``confusion`` (classes,
        classes; rows = true labels) as numpy arrays; and derived ``accuracy_ensemble``, ``accuracy_posterior_mean`` (None when
        no update carried posterior-mean outputs), ``nll_mean`` (over the rows with a target) and ``entropy_mean`` (over the
        finite rows) -- NaN where the denominator is 0.  ``strict``: targets outside [0, classes) raise IndexError, as
        ``F.nll_loss`` would have; with ``strict=False`` they are reported in ``bad_targets`` and left out of the totals."""
        import numpy as np
        from . import _lib
        h = self._host()
        n, S, C = _lib.EVAL_COUNTS, self.samples, self.classes
        res = {k: int(h[i]) for i, k in enumerate(_lib.EVAL_COUNT_NAMES)}
        self._refuse_bad_targets(res, strict, "outside [0, %d)" % C)
        sums = h[n + S + C * C:].view(np.float64)
        res["correct_member"] = h[n:n + S].copy()
        res["confusion"] = h[n + S:n + S + C * C].reshape(C, C).copy()
        res["nll_sum"], res["entropy_sum"] = float(sums[0]), float(sums[1])
        nt, nf = res["rows_with_target"], res["rows"] - res["entropy_nonfinite"]
        div = lambda x, d: x / d if d else float("nan")
        res["accuracy_ensemble"] = div(res["correct_ensemble"], nt)
        res["accuracy_posterior_mean"] = div(res["correct_posterior_mean"], nt) if self.posterior_mean_updates else None
        res["nll_mean"] = div(res["nll_sum"], nt)
        res["entropy_mean"] = div(res["entropy_sum"], nf)
        return res


# ----------------------------------------------------------------------------------------- uncertainty on the device
UNCERTAINTY_ROW_KEYS = ("confidence", "total_entropy", "expected_entropy", "mutual_information", "brier", "log_score")
OOD_SCORES = ("total_entropy", "mutual_information", "max_prob")


def _ent_scale(classes: int, hist_bins: int):
    """The fp32 factor lbbnn_eval_uncertainty multiplies an entropy by to find its histogram bin: K / ln C (0 for one class)."""
    import numpy as np
    return np.float32(hist_bins / math.log(classes)) if classes > 1 else np.float32(0.0)


@torch.no_grad()
def ensemble_uncertainty(outputs: torch.Tensor, target: Optional[torch.Tensor] = None, *,
                         acc: Optional["UncertaintyAccumulator"] = None) -> Dict[str, object]:
    """How good the ensemble's uncertainty is, per row, from one (samples, B, classes) block of log-probabilities in ONE
    lbbnn_eval_uncertainty call (1 launch; 2 with ``acc``) and without a host synchronisation (arithmetic: include/lbbnn.h):

    * ``bma_probs`` (B, classes): the predictive distribution of the Bayesian model average, mean_s exp(outputs[s]);
      ``pred_bma`` (B,) int64 its argmax (numpy.argmax's rule) and ``confidence`` (B,) its maximum;
    * ``total_entropy`` = H[p], ``expected_entropy`` = mean_s H[p_s] (the aleatoric part) and ``mutual_information`` = their
      difference, clamped at 0 (the epistemic part, BALD: large when the members disagree, 0 when each is equally unsure);
    * with ``target`` (B,): ``brier`` = sum_c (p_c - [c == target])^2 and ``log_score`` = -log p_target, the log score of the
      model average (not ``nll_sum``'s mean log-probability), finite whenever one member gives the target a finite
      log-probability; NaN in both for rows without a target inside [0, classes).

    ``outputs``: as ``ensemble_metrics`` takes it (strided views are read in place; classes <= 64).  ``acc``: an
    ``UncertaintyAccumulator`` whose running totals this call adds to (``UncertaintyAccumulator.update`` is this call)."""
    import ctypes
    from . import _lib
    o, S, B, C, ms, ldp = _member_block(outputs, "ensemble_uncertainty")
    dev = outputs.device
    a = _lib.EvalUncertaintyArgs()
    a.logp, a.m_stride, a.ldp, a.S, a.B, a.C = o.data_ptr(), ms, ldp, S, B, C
    keep = [o]
    if target is not None:
        t = _target_rows(target, B, dev)
        a.target = t.data_ptr()
        keep.append(t)
    # the per-row outputs as one allocation: pred_bma int64, then [bma_probs | the six per-row floats] fp32
    n = len(UNCERTAINTY_ROW_KEYS)
    buf = torch.empty(B + (B * C + n * B + 1) // 2, dtype=torch.int64, device=dev)
    fl = buf[B:].view(torch.float32)
    res = {"bma_probs": fl[:B * C].view(B, C), "pred_bma": buf[:B]}
    a.bma_probs, a.pred_bma = fl.data_ptr(), buf.data_ptr()
    for i, k in enumerate(UNCERTAINTY_ROW_KEYS):
        res[k] = fl[B * C + i * B:B * C + (i + 1) * B]
        setattr(a, k, fl.data_ptr() + 4 * (B * C + i * B))
    if acc is not None:
        acc._fill(a, S, B, C, dev)
    if B > 0:                                                # (an empty batch has no storage to point at, and nothing to add)
        _launch(dev, "lbbnn_eval_uncertainty", ctypes.byref(a))
    if acc is not None:
        acc._note()
    del keep
    return res


class UncertaintyAccumulator(_DeviceTotals):
    """Running uncertainty and calibration totals of an evaluation pass, kept on the device: ``update`` adds a batch (no host
    read), ``result`` reads them -- one buffer, one copy.  Counts, the sums of the per-row numbers of ``ensemble_uncertainty``,
    a reliability table over ``conf_bins`` equal-width confidence bins and ``hist_bins``-bin histograms of the three
    out-of-distribution scores (total entropy and mutual information over [0, ln classes], 1 - confidence over [0, 1]).
    ``classes`` <= 64, ``samples``, ``conf_bins`` <= 100 and ``hist_bins`` <= 4096 are fixed for the accumulator's life."""

    def __init__(self, classes: int, samples: int, device, conf_bins: int = 20, hist_bins: int = 1024):
        from . import _lib
        C, S, M, K = int(classes), int(samples), int(conf_bins), int(hist_bins)
        if not 1 <= C <= 64:
            raise ValueError("bnn_amd: UncertaintyAccumulator takes 1 to 64 classes, got %d" % C)
        if not 1 <= S <= 65535:
            raise ValueError("bnn_amd: UncertaintyAccumulator takes 1 to 65535 members, got %d" % S)
        if not 1 <= M <= 100:
            raise ValueError("bnn_amd: UncertaintyAccumulator takes 1 to 100 confidence bins, got %d" % M)
        if not 1 <= K <= 4096:
            raise ValueError("bnn_amd: UncertaintyAccumulator takes 1 to 4096 histogram bins, got %d" % K)
        self.classes, self.samples, self.conf_bins, self.hist_bins = C, S, M, K
        self.ent_scale = _ent_scale(C, K)
        # one buffer, one read: counts | sums | bin_rows | bin_rows_with_target | bin_correct | bin_conf_sum | hist (the doubles
        # as bit patterns)
        self._start(self._offsets()["end"], device)

    def _offsets(self) -> Dict[str, int]:
        """Where each total starts in the buffer, in 8-byte words."""
        from . import _lib
        M, K = self.conf_bins, self.hist_bins
        off, at = {}, 0
        for name, n in (("counts", _lib.UNC_COUNTS), ("sums", _lib.UNC_SUMS), ("bin_rows", M), ("bin_rows_with_target", M),
                        ("bin_correct", M), ("bin_conf_sum", M), ("hist", 3 * K)):
            off[name] = at
            at += n
        off["end"] = at
        return off

    def _fill(self, a, S, B, C, dev):
        """Point the totals of an lbbnn_eval_uncertainty_args_t at this accumulator (work memory grows to the largest batch)."""
        from . import _lib
        self._check_batch(S, C, dev)
        a.work = self._work_ptr(_lib.lib().lbbnn_eval_uncertainty_work_bytes(S, B, C, self.conf_bins))
        base = self._totals.data_ptr()
        for name, at in self._offsets().items():
            if name != "end":
                setattr(a, name, base + 8 * at)
        a.conf_bins, a.hist_bins, a.ent_scale = self.conf_bins, self.hist_bins, float(self.ent_scale)

    def update(self, outputs: torch.Tensor, target: Optional[torch.Tensor] = None):
        """``ensemble_uncertainty(outputs, target)`` of one batch, its numbers added to the totals."""
        return ensemble_uncertainty(outputs, target, acc=self)

    def result(self, strict: bool = True) -> Dict[str, object]:
        """Python numbers and numpy arrays.  The raw totals: the counts ``rows``, ``rows_with_target``, ``bad_targets``,
        ``correct_bma``, ``nonfinite_rows`` (rows whose confidence, entropies or mutual information are not finite: they are in
        no sum, bin or histogram), ``log_score_nonfinite``; ``<name>_sum`` for total_entropy, expected_entropy,
        mutual_information, confidence (over the finite rows), brier and log_score (over the finite rows with a target);
        ``bin_rows``, ``bin_rows_with_target``, ``bin_correct``, ``bin_conf_sum`` (conf_bins,).  Derived: ``<name>_mean``,
        ``accuracy_bma``, ``ece`` = sum_m n_m / N |correct_m / n_m - conf_sum_m / n_m| and ``mce`` (the largest gap) over the
        rows with a target, empty bins skipped; ``reliability`` (per bin: ``edges``, ``rows``, ``rows_with_target``,
        ``accuracy``, ``confidence``); ``selective`` (per threshold k / conf_bins: ``coverage`` and ``accuracy`` of the rows with
        a target whose confidence is at least the threshold -- what abstaining below it would give); ``histograms``: for each of
        ``OOD_SCORES`` its ``counts`` and ``edges`` (``max_prob`` is the histogram of 1 - confidence, so that a higher score
        means less certain in all three).  NaN where a denominator is 0.  ``strict``: as ``EvalAccumulator.result``."""
        import numpy as np
        from . import _lib
        h = self._host()
        off, M, K, C = self._offsets(), self.conf_bins, self.hist_bins, self.classes
        res = {k: int(h[off["counts"] + i]) for i, k in enumerate(_lib.UNC_COUNT_NAMES)}
        self._refuse_bad_targets(res, strict, "outside [0, %d)" % C)
        res.update(classes=C, samples=self.samples, conf_bins=M, hist_bins=K)
        part = lambda name, n: h[off[name]:off[name] + n]
        sums = part("sums", _lib.UNC_SUMS).view(np.float64)
        n_rows, n_t, n_c = part("bin_rows", M).copy(), part("bin_rows_with_target", M).copy(), part("bin_correct", M).copy()
        conf_sum = part("bin_conf_sum", M).view(np.float64).copy()
        res.update(bin_rows=n_rows, bin_rows_with_target=n_t, bin_correct=n_c, bin_conf_sum=conf_sum)
        div = lambda x, d: x / d if d else float("nan")
        nf, N = res["rows"] - res["nonfinite_rows"], int(n_t.sum())
        for i, k in enumerate(_lib.UNC_SUM_NAMES):
            res[k + "_sum"] = float(sums[i])
            res[k + "_mean"] = div(float(sums[i]), nf if i < 4 else N if k == "brier" else N - res["log_score_nonfinite"])
        res["accuracy_bma"] = div(res["correct_bma"], res["rows_with_target"])
        full = n_t > 0
        with np.errstate(all="ignore"):
            acc_m, conf_m = n_c / n_t, conf_sum / n_t          # NaN in the empty bins
        gap = np.abs(acc_m[full] - conf_m[full])
        res["ece"] = float((n_t[full] / N * gap).sum()) if N else float("nan")
        res["mce"] = float(gap.max()) if N else float("nan")
        res["reliability"] = {"edges": np.arange(M + 1) / M, "rows": n_rows, "rows_with_target": n_t, "accuracy": acc_m,
                              "confidence": conf_m}
        kept_t, kept_c = n_t[::-1].cumsum()[::-1], n_c[::-1].cumsum()[::-1]      # bins k .. M-1: confidence >= k / M
        with np.errstate(all="ignore"):
            res["selective"] = {"threshold": np.arange(M) / M, "coverage": kept_t / N if N else np.full(M, np.nan),
                                "accuracy": kept_c / kept_t}
        hist = part("hist", 3 * K).reshape(3, K)
        ent_edges = np.arange(K + 1) * (math.log(C) / K if C > 1 else 0.0)
        res["histograms"] = {k: {"counts": hist[i].copy(), "edges": ent_edges if i < 2 else np.arange(K + 1) / K}
                             for i, k in enumerate(OOD_SCORES)}
        return res


def ood_auroc(in_result: Dict[str, object], out_result: Dict[str, object], score: str = "total_entropy"):
    """``(auroc, half_width)`` of telling an out-of-distribution pass from an in-distribution pass by ``score``
    ("total_entropy" | "mutual_information" | "max_prob": 1 - confidence; higher = out of distribution), from the histograms
    of two ``UncertaintyAccumulator.result()``s -- the reference's outofsample study (the entropy CDFs of FMNIST / KMNIST against
    MNIST) as one number.  Pairs that fall in the same bin count 1/2; ``half_width`` = 0.5 sum_k in_k out_k / (N_in N_out) is
    what they could change, so the AUROC of the per-row scores themselves lies in [auroc - half_width, auroc + half_width].
    Both passes must have the same number of classes and histogram bins (ValueError)."""
    import numpy as np
    if score not in OOD_SCORES:
        raise ValueError("bnn_amd: score must be one of %s, got %r" % (OOD_SCORES, score))
    for k in ("classes", "hist_bins"):
        if in_result[k] != out_result[k]:
            raise ValueError("bnn_amd: ood_auroc needs two passes with the same %s, got %d and %d" % (k, in_result[k], out_result[k]))
    hi = np.asarray(in_result["histograms"][score]["counts"], dtype=np.int64)
    ho = np.asarray(out_result["histograms"][score]["counts"], dtype=np.int64)
    n_in, n_out = int(hi.sum()), int(ho.sum())
    if not n_in or not n_out:
        return float("nan"), float("nan")
    below = np.concatenate([[0], hi.cumsum()[:-1]])            # in-distribution rows in lower bins
    ties = int((hi * ho).sum())
    pairs = n_in * n_out
    return (int((ho * below).sum()) + 0.5 * ties) / pairs, 0.5 * ties / pairs


# ----------------------------------------------------------------------------------------- regression on the device
def pit_coverage(pit_hist, level: float) -> float:
    """The share of the PIT values of a pass that fall inside the central interval [(1 - level) / 2, (1 + level) / 2] -- the
    empirical coverage of the central ``level`` predictive interval, ``level`` itself for a calibrated model -- from a PIT
    histogram of equal-width bins.  The two edges must be bin edges (with 20 bins: 0.5, 0.8, 0.9 ...): ValueError otherwise.
    NaN for an empty histogram."""
    import numpy as np
    h = np.asarray(pit_hist, dtype=np.int64)
    K, level = int(h.shape[0]), float(level)
    if not 0.0 < level <= 1.0:
        raise ValueError("bnn_amd: coverage level must lie in (0, 1], got %r" % (level,))
    lo, hi = (1.0 - level) / 2.0 * K, (1.0 + level) / 2.0 * K
    if abs(lo - round(lo)) > 1e-9 or abs(hi - round(hi)) > 1e-9:
        raise ValueError("bnn_amd: coverage(%r): the interval [%g, %g] does not end on bin edges of a %d-bin PIT histogram"
                         % (level, (1.0 - level) / 2.0, (1.0 + level) / 2.0, K))
    n = int(h.sum())
    return float(h[int(round(lo)):int(round(hi))].sum()) / n if n else float("nan")


def _regression_target(target: torch.Tensor, B: int, O: int, dev) -> torch.Tensor:
    """``target`` as the dense (B, O) float32 block the regression kernel reads."""
    if not torch.is_tensor(target) or target.device != dev or \
            (tuple(target.shape) != (B, O) and not (O == 1 and tuple(target.shape) == (B,))):
        raise ValueError("bnn_amd: target must be (%d, %d)%s on %s, got %s"
                         % (B, O, " or (%d,)" % B if O == 1 else "", dev,
                            "%s on %s" % (tuple(target.shape), target.device) if torch.is_tensor(target) else type(target).__name__))
    t = target if target.dtype == torch.float32 else target.float()
    return t.contiguous().view(B, O)


def _regression_log_var(log_var, O: int, dev) -> torch.Tensor:
    """``log_var`` as the (O,) float32 device tensor the kernel reads through its pointer: a live tensor as it is, a number as
    a tensor filled with it."""
    if torch.is_tensor(log_var):
        if log_var.dtype != torch.float32 or tuple(log_var.shape) != (O,) or log_var.device != dev or not log_var.is_contiguous():
            raise ValueError("bnn_amd: log_var must be a number or a contiguous float32 (%d,) tensor on %s, got %s %s on %s"
                             % (O, dev, log_var.dtype, tuple(log_var.shape), log_var.device))
        return log_var.detach()
    if isinstance(log_var, bool) or not isinstance(log_var, (int, float)):
        raise ValueError("bnn_amd: log_var must be a number or a float32 (%d,) tensor, got %s" % (O, type(log_var).__name__))
    return torch.full((O,), float(log_var), dtype=torch.float32, device=dev)


@torch.no_grad()
def ensemble_regression(outputs: torch.Tensor, target: Optional[torch.Tensor] = None, log_var=0.0,
                        mean_outputs: Optional[torch.Tensor] = None, *,
                        acc: Optional["RegressionAccumulator"] = None) -> Dict[str, object]:
    """The per-element numbers of a regression ensemble from one (samples, B, units) block of raw outputs (an identity-head
    network's ``ensemble_forward`` / ``FrozenNetwork.ensemble``) under a normal likelihood with log-variance ``log_var`` per
    output unit, in ONE lbbnn_eval_regression call (1 launch; 2 with ``acc``) and without a host synchronisation (arithmetic:
    include/lbbnn.h), each (B, units):

    * ``pred_mean``: the mean over the members, summed in member order in fp32 and divided by ``samples`` (reproducible bit
      for bit on the CPU), and ``epistemic_var``: the members' variance about it, in the same fixed arithmetic;
    * ``aleatoric_var`` = exp(log_var) and ``total_std`` = sqrt(epistemic_var + aleatoric_var);
    * with ``target`` (B, units) (or (B,) for one unit): ``sq_err`` = (y - pred_mean)^2, ``log_density`` = the log of the
      members' mixture density at y (a streaming logsumexp: finite whenever one member's density is) and ``pit`` = the mixture's
      CDF at y; NaN in all three for elements whose target is NaN or infinite, or without a target.

    ``outputs``: as ``ensemble_metrics`` takes it (strided views are read in place); units <= 16.  ``log_var``: a number, or a
    live float32 (units,) device tensor (the parameter the training loss learned).  ``acc``: a ``RegressionAccumulator`` whose
    running totals this call adds to (``RegressionAccumulator.update`` is this call with the accumulator's ``log_var``)."""
    import ctypes
    from . import _lib
    o, S, B, O, ms, ldp = _member_block(outputs, "ensemble_regression")
    if O > 16:
        raise ValueError("bnn_amd: ensemble_regression takes 1 to 16 output units, got %d" % O)
    dev = outputs.device
    lv = acc._log_var if acc is not None else _regression_log_var(log_var, O, dev)
    a = _lib.EvalRegressionArgs()
    a.out, a.m_stride, a.ldp, a.S, a.B, a.O, a.log_var = o.data_ptr(), ms, ldp, S, B, O, lv.data_ptr()
    keep = [o, lv]
    if mean_outputs is not None:
        mo, a.ldm = _mean_rows(mean_outputs, B, O, dev)
        a.mean_out = mo.data_ptr()
        keep.append(mo)
    if target is not None:
        t = _regression_target(target, B, O, dev)
        a.target, a.ldt = t.data_ptr(), O
        keep.append(t)
    keys = _lib.REG_ROW_KEYS
    buf = torch.empty((len(keys), B, O), dtype=torch.float32, device=dev)      # the per-element outputs as one allocation
    res = {}
    for i, k in enumerate(keys):
        res[k] = buf[i]
        setattr(a, k, buf.data_ptr() + 4 * i * B * O)
    if acc is not None:
        acc._fill(a, S, B, O, dev)
    if B > 0:                                                # (an empty batch has no storage to point at, and nothing to add)
        _launch(dev, "lbbnn_eval_regression", ctypes.byref(a))
    if acc is not None:
        acc._note(mean_outputs is not None)
    del keep
    return res


class RegressionAccumulator(_MeanTotals):
    """Running regression totals of an evaluation pass, kept on the device: ``update`` adds a batch (no host read), ``result``
    reads them -- one buffer, one copy, the ONLY synchronisation of a pass.  The counterpart of ``EvalAccumulator`` /
    ``UncertaintyAccumulator`` for a network with ``head="identity"``: error sums, the log density of the members' mixture,
    the epistemic and total predictive variance, and a histogram of the probability integral transform (calibration).

    ``units`` (1 to 16), ``samples`` and ``pit_bins`` (1 to 1024) are fixed for the accumulator's life.  ``log_var``: the
    log-variance of the normal likelihood per output unit -- a number, or a live float32 (units,) device tensor (e.g. the
    ``nn.Parameter`` that ``elbo_gaussian_loss`` trained), which the kernel reads through its pointer at every update."""

    _width = "units"
    _layout = ("REG_COUNTS", "REG_SUMS")       # the _lib names of the sizes of counts | sums; pit_hist follows them

    def __init__(self, units: int, samples: int, device, log_var, pit_bins: int = 20):
        from . import _lib
        O, S, K = int(units), int(samples), int(pit_bins)
        if not 1 <= O <= 16:
            raise ValueError("bnn_amd: RegressionAccumulator takes 1 to 16 output units, got %d" % O)
        if not 1 <= S <= 65535:
            raise ValueError("bnn_amd: RegressionAccumulator takes 1 to 65535 members, got %d" % S)
        if not 1 <= K <= 1024:
            raise ValueError("bnn_amd: RegressionAccumulator takes 1 to 1024 PIT bins, got %d" % K)
        self.units, self.samples, self.pit_bins = O, S, K
        # one buffer, one read: counts | sums (bit patterns) | pit_hist
        self._start(getattr(_lib, self._layout[0]) + getattr(_lib, self._layout[1]) + K, device)
        self._log_var = _regression_log_var(log_var, O, self._totals.device)

    def _work_bytes(self, S, B, O):
        from . import _lib
        return _lib.lib().lbbnn_eval_regression_work_bytes(S, B, O)

    def _fill(self, a, S, B, O, dev):
        """Point the totals of the call's arguments at this accumulator (work memory grows to the largest batch)."""
        from . import _lib
        self._check_batch(S, O, dev)
        a.work, a.pit_bins = self._work_ptr(self._work_bytes(S, B, O)), self.pit_bins
        nc, ns, base = getattr(_lib, self._layout[0]), getattr(_lib, self._layout[1]), self._totals.data_ptr()
        a.counts, a.sums, a.pit_hist = base, base + 8 * nc, base + 8 * (nc + ns)

    def update(self, outputs: torch.Tensor, target: Optional[torch.Tensor] = None, mean_outputs: Optional[torch.Tensor] = None):
        """``ensemble_regression(outputs, target, self's log_var, mean_outputs)`` of one batch, its numbers added to the totals."""
        return ensemble_regression(outputs, target, None, mean_outputs, acc=self)

    def result(self, strict: bool = True) -> Dict[str, object]:
        """Python numbers.  Counts: ``elements``, ``elements_with_target``, ``bad_targets`` (NaN or infinite targets),
        ``nonfinite_elements`` (a member's output or the log-variance is not finite: in no sum and no bin),
        ``scored_elements`` (finite, with a valid target: what the error sums are over).  ``<name>_sum`` for sq_err, abs_err,
        log_density, y, y2, posterior_mean_sq_err (over the scored elements), epistemic_var and total_var (over the finite
        ones).  Derived: ``rmse``, ``mae``, ``mean_log_density``, ``r2`` = 1 - sq_err_sum / (y2_sum - y_sum^2 / n),
        ``mean_epistemic_var``, ``mean_total_var``, ``rmse_posterior_mean`` (None when no update carried posterior-mean
        outputs) -- NaN where a denominator is 0; ``pit_hist`` (pit_bins,) as a numpy array and ``coverage``: a function
        ``coverage(level)`` = ``pit_coverage(pit_hist, level)``, the share of PIT values in the central ``level`` interval
        (ValueError when its edges are not bin edges).  ``strict``: as ``EvalAccumulator.result`` -- bad targets raise
        IndexError; with ``strict=False`` they are reported in ``bad_targets`` and left out of the totals."""
        return self._result_of(self._host(), strict)

    def _result_of(self, h, strict: bool) -> Dict[str, object]:
        """``result`` from the host copy ``h`` of totals laid out counts | sums | pit_hist."""
        import functools
        import numpy as np
        from . import _lib
        nc, ns = _lib.REG_COUNTS, _lib.REG_SUMS
        res = {k: int(h[i]) for i, k in enumerate(_lib.REG_COUNT_NAMES)}
        self._refuse_bad_targets(res, strict, "that are NaN or infinite")
        res.update(units=self.units, samples=self.samples, pit_bins=self.pit_bins)
        sums = h[nc:nc + ns].view(np.float64)
        for i, k in enumerate(_lib.REG_SUM_NAMES):
            res[k + "_sum"] = float(sums[i])
        div = lambda x, d: x / d if d else float("nan")
        n, nf = res["scored_elements"], res["elements"] - res["nonfinite_elements"]
        root = lambda v: math.sqrt(v) if v >= 0 else float("nan")
        res["rmse"] = root(div(res["sq_err_sum"], n))
        res["mae"] = div(res["abs_err_sum"], n)
        res["mean_log_density"] = div(res["log_density_sum"], n)
        sst = res["y2_sum"] - div(res["y_sum"] ** 2, n)
        res["r2"] = 1.0 - div(res["sq_err_sum"], sst) if n else float("nan")
        res["mean_epistemic_var"] = div(res["epistemic_var_sum"], nf)
        res["mean_total_var"] = div(res["total_var_sum"], nf)
        res["rmse_posterior_mean"] = root(div(res["posterior_mean_sq_err_sum"], n)) if self.posterior_mean_updates else None
        res["pit_hist"] = h[nc + ns:].copy()
        res["coverage"] = functools.partial(pit_coverage, res["pit_hist"])
        return res


def _score_levels(levels) -> Tuple[float, ...]:
    """``levels`` as a tuple of at most 4 central interval levels, each in [0.01, 0.999] as the float32 the kernel reads."""
    from . import _lib
    try:
        lv = tuple(float(p) for p in levels)
    except TypeError:
        raise ValueError("bnn_amd: levels must be a sequence of numbers, got %s" % type(levels).__name__)
    if len(lv) > _lib.SCORE_MAX_LEVELS:
        raise ValueError("bnn_amd: at most %d interval levels, got %d" % (_lib.SCORE_MAX_LEVELS, len(lv)))
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    for p in lv:
        if not f32(0.01) <= f32(p) <= f32(0.999):              # as the library compares them; a NaN fails both comparisons
            raise ValueError("bnn_amd: an interval level must lie in [0.01, 0.999], got %r" % (p,))
    return lv


def _scores_log_var(log_var, S: int, B: int, O: int, dev):
    """(tensor, member stride, row stride) of the log-variance operand of lbbnn_eval_regression_scores: a number or a (O,) tensor
    as ``_regression_log_var`` takes them -> (0, 0); a float32 (B, O) tensor -> (0, ld); a float32 (S, B, O) tensor -> (ms, ld),
    read in place where the last dimension is dense and the members do not overlap."""
    if not torch.is_tensor(log_var) or log_var.dim() < 2:
        return _regression_log_var(log_var, O, dev), 0, 0
    if log_var.dtype != torch.float32 or log_var.device != dev or tuple(log_var.shape) not in ((B, O), (S, B, O)):
        raise ValueError("bnn_amd: log_var must be a number, \"output\", or a float32 tensor of shape (%d,), (%d, %d) or (%d, %d, %d) "
                         "on %s, got %s %s on %s" % (O, B, O, S, B, O, dev, log_var.dtype, tuple(log_var.shape), log_var.device))
    lv = log_var.detach()
    if lv.dim() == 2:
        lv, ld = _dense_rows(lv, B, O)
        return lv, 0, ld
    ld = lv.stride(1) if B > 1 else O
    ms = lv.stride(0) if S > 1 else 0
    if (O > 1 and lv.stride(2) != 1) or ld < O or (S > 1 and B > 0 and ms < (B - 1) * ld + O):
        lv, ld, ms = lv.contiguous(), O, B * O
    if S == 1:
        ms = 0
    return lv, ms, ld


@torch.no_grad()
def ensemble_scores(outputs: torch.Tensor, target: Optional[torch.Tensor] = None, log_var=0.0,
                    mean_outputs: Optional[torch.Tensor] = None, *, levels=(0.9,),
                    acc: Optional["RegressionScoreAccumulator"] = None) -> Dict[str, object]:
    """``ensemble_regression`` for a noise level that may differ per element or per member, with two more scores: the
    per-element numbers of a regression ensemble from one (samples, B, units) block of member means under a normal likelihood,
    in ONE lbbnn_eval_regression_scores call (1 launch; 2 with ``acc``) and without a host synchronisation (arithmetic:
    include/lbbnn.h).  Each (B, units):

    * ``pred_mean``, ``epistemic_var``: ``ensemble_regression``'s, the same bits;
    * ``aleatoric_var`` = the members' mean of exp(log_var) and ``total_std`` = sqrt(epistemic_var + aleatoric_var);
    * with ``target``: ``sq_err``, ``log_density`` and ``pit`` of the members' mixture, each member with its own variance, and
      ``crps``: the continuous ranked probability score of that mixture in closed form; NaN without a valid target;

    and (len(levels), B, units): ``lower`` / ``upper``, the (1 - p) / 2 and (1 + p) / 2 quantiles of the mixture for each central
    level p of ``levels`` (at most 4, each in [0.01, 0.999]), and with ``target`` the ``interval_score``
    (upper - lower) + 2 / (1 - p) * (the distance by which the target misses the interval).  An element one of whose members has
    a non-finite mean, or a log-variance that is non-finite or beyond +-80, is NaN in every output.

    ``outputs``: as ``ensemble_regression`` takes it, at most 64 members.  ``log_var``: a number; a live float32 (units,) tensor;
    a float32 (B, units) tensor (one value per element); a float32 (samples, B, units) tensor (one per member and element); or
    the string ``"output"``: ``outputs`` is then (samples, B, 2 * units) with the means in columns [0, units) and the
    log-variances in [units, 2 * units) -- what a ``dims[-1] == 2 * units`` identity-head network trained with
    ``elbo_gaussian_loss(out[:, :units], y, out[:, units:])`` returns -- read in place, and ``mean_outputs`` is
    (B, 2 * units), of which only the mean columns are read.  ``acc``: a ``RegressionScoreAccumulator`` whose running totals this
    call adds to (its ``levels`` are used)."""
    import ctypes
    from . import _lib
    in_output = isinstance(log_var, str)
    if in_output and log_var != "output":
        raise ValueError("bnn_amd: log_var must be a number, a tensor or the string \"output\", got %r" % (log_var,))
    if acc is not None and not isinstance(acc, RegressionScoreAccumulator):
        raise ValueError("bnn_amd: ensemble_scores takes acc=RegressionScoreAccumulator, got %s" % type(acc).__name__)
    lev = acc.levels if acc is not None else _score_levels(levels)
    o, S, B, C, ms, ldp = _member_block(outputs, "ensemble_scores")
    if in_output and C % 2:
        raise ValueError("bnn_amd: log_var=\"output\" takes outputs with 2 * units columns, got %d" % C)
    O = C // 2 if in_output else C
    if O > 16:
        raise ValueError("bnn_amd: ensemble_scores takes 1 to 16 output units, got %d" % O)
    if S > _lib.SCORE_MAX_MEMBERS:
        raise ValueError("bnn_amd: ensemble_scores takes 1 to %d members, got %d" % (_lib.SCORE_MAX_MEMBERS, S))
    dev = outputs.device
    a = _lib.EvalScoresArgs()
    a.out, a.m_stride, a.ldp, a.S, a.B, a.O = o.data_ptr(), ms, ldp, S, B, O
    if in_output:
        # the upper columns of the members' own buffer; one member: its rows are one value per element
        lv, a.lv_mstride, a.lv_ld = o, ms, ldp
        a.log_var = o.data_ptr() + 4 * O
    else:
        lv, a.lv_mstride, a.lv_ld = _scores_log_var(log_var, S, B, O, dev)
        a.log_var = lv.data_ptr()
    keep = [o, lv]
    if mean_outputs is not None:
        mo, a.ldm = _mean_rows(mean_outputs, B, C, dev)
        a.mean_out = mo.data_ptr()
        keep.append(mo)
    if target is not None:
        t = _regression_target(target, B, O, dev)
        a.target, a.ldt = t.data_ptr(), O
        keep.append(t)
    a.n_levels = L = len(lev)
    for i, p in enumerate(lev):
        a.levels[i] = p
    rows, per_level = _lib.SCORE_ROW_KEYS, _lib.SCORE_LEVEL_KEYS
    buf = torch.empty((len(rows) + L * len(per_level), B, O), dtype=torch.float32, device=dev)    # one allocation
    res = {}
    for i, k in enumerate(rows):
        res[k] = buf[i]
        setattr(a, k, buf.data_ptr() + 4 * i * B * O)
    for j, k in enumerate(per_level):
        first = len(rows) + j * L
        res[k] = buf[first:first + L]
        if L:
            setattr(a, k, buf.data_ptr() + 4 * first * B * O)
    if acc is not None:
        acc._fill(a, S, B, O, dev)
    if B > 0:                                                # (an empty batch has no storage to point at, and nothing to add)
        _launch(dev, "lbbnn_eval_regression_scores", ctypes.byref(a))
    if acc is not None:
        acc._note(mean_outputs is not None)
    del keep
    return res


class RegressionScoreAccumulator(RegressionAccumulator):
    """A ``RegressionAccumulator`` for a noise level of any layout, with the CRPS and prediction intervals: ``update`` is
    ``ensemble_scores`` with the accumulator's ``log_var`` and ``levels``, its numbers added to totals on the device (no host
    read); ``result`` reads them in one copy.  ``evaluate_batches`` and ``graphs.make_graphed_eval_step`` take it wherever they
    take a ``RegressionAccumulator``.

    ``units`` (1 to 16), ``samples`` (1 to 64: the CRPS is quadratic in it), ``pit_bins`` and ``levels`` (at most 4 central
    interval levels, each in [0.01, 0.999]) are fixed for the accumulator's life.  ``log_var``: a number, a live float32 (units,)
    device tensor, or ``"output"`` -- the model then has ``dims[-1] == 2 * units`` and every member's outputs carry the
    log-variances in their upper ``units`` columns.  A per-batch (B, units) or (samples, B, units) tensor goes to ``update``."""

    _layout = ("SCORE_COUNTS", "SCORE_SUMS")

    def __init__(self, units: int, samples: int, device, log_var, pit_bins: int = 20, levels=(0.5, 0.9)):
        from . import _lib
        self.in_output = isinstance(log_var, str)
        if self.in_output and log_var != "output":
            raise ValueError("bnn_amd: log_var must be a number, a float32 (units,) tensor or the string \"output\", got %r" % (log_var,))
        super().__init__(units, samples, device, 0.0 if self.in_output else log_var, pit_bins)
        if self.samples > _lib.SCORE_MAX_MEMBERS:
            raise ValueError("bnn_amd: RegressionScoreAccumulator takes 1 to %d members, got %d" % (_lib.SCORE_MAX_MEMBERS, self.samples))
        self.levels = _score_levels(levels)

    def _work_bytes(self, S, B, O):
        from . import _lib
        return _lib.lib().lbbnn_eval_regression_scores_work_bytes(S, B, O, len(self.levels))

    def update(self, outputs: torch.Tensor, target: Optional[torch.Tensor] = None, mean_outputs: Optional[torch.Tensor] = None,
               *, log_var=None):
        """``ensemble_scores(outputs, target, log_var, mean_outputs)`` of one batch with the accumulator's levels, its numbers
        added to the totals.  ``log_var``: None for the accumulator's own, or this batch's float32 (B, units) /
        (samples, B, units) tensor."""
        if self.in_output:
            if log_var is not None:
                raise ValueError("bnn_amd: this RegressionScoreAccumulator reads log_var from the outputs (log_var=\"output\")")
            if outputs.dim() == 3 and outputs.shape[-1] != 2 * self.units:
                raise ValueError("bnn_amd: log_var=\"output\" with %d units takes outputs of 2 * units = %d columns (the model's "
                                 "dims[-1]), got %d" % (self.units, 2 * self.units, outputs.shape[-1]))
            return ensemble_scores(outputs, target, "output", mean_outputs, acc=self)
        if log_var is not None and not (torch.is_tensor(log_var) and log_var.dim() >= 2):
            raise ValueError("bnn_amd: update takes log_var=None or this batch's (B, units) / (samples, B, units) tensor")
        return ensemble_scores(outputs, target, self._log_var if log_var is None else log_var, mean_outputs, acc=self)

    def result(self, strict: bool = True) -> Dict[str, object]:
        """Everything ``RegressionAccumulator.result`` returns, under the same keys (``total_var`` is epistemic plus the
        members' mean aleatoric variance), and: ``aleatoric_var_sum`` / ``mean_aleatoric_var`` over the finite elements,
        ``crps_sum`` / ``crps`` (the mean over the scored elements), ``levels`` and ``intervals``: per level a dict of
        ``level``, ``inside`` (scored elements with lower <= y <= upper), ``coverage`` = inside / scored, ``width_sum`` /
        ``mean_width`` and ``interval_score_sum`` / ``mean_interval_score`` over the scored elements.  NaN where a denominator
        is 0.  ``strict``: as ``RegressionAccumulator.result``."""
        import numpy as np
        from . import _lib
        h = self._host()
        nc, ns, rc, rs, ml = _lib.SCORE_COUNTS, _lib.SCORE_SUMS, _lib.REG_COUNTS, _lib.REG_SUMS, _lib.SCORE_MAX_LEVELS
        res = self._result_of(np.concatenate([h[:rc], h[nc:nc + rs], h[nc + ns:]]), strict)
        sums = h[nc:nc + ns].view(np.float64)
        div = lambda x, d: x / d if d else float("nan")
        n, nf = res["scored_elements"], res["elements"] - res["nonfinite_elements"]
        res["aleatoric_var_sum"], res["crps_sum"] = float(sums[rs]), float(sums[rs + 1])
        res["mean_aleatoric_var"] = div(res["aleatoric_var_sum"], nf)
        res["crps"] = div(res["crps_sum"], n)
        res["levels"] = self.levels
        res["intervals"] = []
        for l, p in enumerate(self.levels):
            w, s, inside = float(sums[rs + 2 + l]), float(sums[rs + 2 + ml + l]), int(h[rc + l])
            res["intervals"].append(dict(level=p, inside=inside, coverage=div(inside, n), width_sum=w, mean_width=div(w, n),
                                         interval_score_sum=s, mean_interval_score=div(s, n)))
        return res


@torch.no_grad()
def predict_regression(model, x: torch.Tensor, samples: int, log_var, levels=(0.9,)) -> Dict[str, torch.Tensor]:
    """The predictive distribution of an identity-head LRT / MNF network or its frozen model at ``x`` as device tensors, nothing
    read on the host: the ensemble of ``samples`` members (at most 64) and one ``ensemble_scores`` call without a target.
    ``pred_mean``, ``total_std``, ``epistemic_var``, ``aleatoric_var``: (B, units); ``lower``, ``upper``: (len(levels), B, units),
    the bounds of the central ``levels`` intervals of the members' mixture.  ``log_var``: as ``ensemble_scores`` takes it;
    ``"output"`` for a model whose outputs carry the log-variances in their upper half (units = dims[-1] / 2)."""
    if _head_of(model) != "identity" or not (_is_frozen(model) or hasattr(model, "_forward_streams")):
        raise ValueError("bnn_amd: predict_regression takes an LRT / MNF network with head=\"identity\" or its frozen model, "
                         "got %s with head=%r" % (type(model).__name__, _head_of(model)))
    from . import _lib
    lev = _score_levels(levels)
    S = int(samples)
    if not 1 <= S <= _lib.SCORE_MAX_MEMBERS:
        raise ValueError("bnn_amd: predict_regression takes 1 to %d members, got %d" % (_lib.SCORE_MAX_MEMBERS, S))
    outputs = model.ensemble(x, S) if _is_frozen(model) else ensemble_forward(model, x, S)
    rows = ensemble_scores(outputs, None, log_var, levels=lev)
    return {k: rows[k] for k in ("pred_mean", "total_std", "epistemic_var", "aleatoric_var", "lower", "upper")}


def _regression_pass(net, acc, uncertainty, who: str) -> bool:
    """Whether ``net`` (head) and ``acc`` make a regression pass; ValueError naming the mismatch when only one of them does."""
    reg_net, reg_acc = _head_of(net) == "identity", isinstance(acc, RegressionAccumulator)
    if reg_net and not reg_acc:
        raise ValueError("bnn_amd: %s: this model has head=\"identity\" (regression): acc must be an "
                         "evaluate.RegressionAccumulator, got %s (EvalAccumulator and UncertaintyAccumulator are classification "
                         "tools)" % (who, "None" if acc is None else type(acc).__name__))
    if reg_acc and not reg_net:
        raise ValueError("bnn_amd: %s: a RegressionAccumulator takes a model with head=\"identity\", this one has head=%r"
                         % (who, _head_of(net)))
    if reg_net and uncertainty is not None:
        raise ValueError("bnn_amd: %s: uncertainty= is a classification tool (UncertaintyAccumulator); a head=\"identity\" model "
                         "takes acc=RegressionAccumulator alone" % who)
    if reg_net and not (_is_frozen(net) or hasattr(net, "_forward_streams")):
        raise ValueError("bnn_amd: %s: a regression pass takes an LRT / MNF network or its frozen model" % who)
    return reg_net


def _eval_forwards(net, data, samples: int, posterior_mean: bool, gates: str):
    """(outputs, mean_outputs or None) of one batch, by family, as ``ensemble_eval`` dispatches."""
    if _is_frozen(net):
        if gates != "sample":
            raise ValueError("bnn_amd: gates=%r: the gates of a frozen model were fixed by evaluate.freeze" % (gates,))
        binary = _binary_eval(net)
        outputs = net.ensemble(data, samples, log_probs=binary)
        return outputs, (net(data, sample=False, log_probs=binary) if posterior_mean else None)
    if _is_base(net):
        binary = _binary_eval(net)
        outputs = base_ensemble(net, data, samples, gates=gates, log_probs=binary)["outputs"]
        return outputs, (_base_mean_forward(net, data, binary) if posterior_mean else None)
    if _is_vd(net):
        return ensemble_forward(net, data, samples, gates=gates), None         # VD has no posterior-mean forward
    binary = _binary_eval(net)
    outputs = ensemble_forward(net, data, samples, gates=gates, log_probs=binary)
    return outputs, (_forward_head(net, data, False, binary) if posterior_mean else None)


@torch.no_grad()
def evaluate_batches(net, batches, samples: int = 10, *, acc: Optional[EvalAccumulator] = None, posterior_mean: bool = True,
                     gates: str = "sample", uncertainty: Optional[UncertaintyAccumulator] = None) -> Dict[str, object]:
    """A whole evaluation pass with ONE host synchronisation: for every ``(x, y)`` of ``batches`` (device tensors) the ensemble
    forward of the network's family -- ``ensemble_forward`` / ``FrozenNetwork.ensemble`` / ``base_ensemble`` / ``vd_ensemble``,
    the dispatch and the draws of ``ensemble_eval`` -- the posterior-mean forward where the family has one (``posterior_mean``;
    variational dropout has none) and ``acc.update``; returns ``acc.result()``.  ``acc``: an ``EvalAccumulator`` to add to
    (default: a fresh one).  ``gates="mpm"``: the median probability model of a baseline network.
    ``uncertainty``: an ``UncertaintyAccumulator`` that is updated from the same ``outputs`` in the same pass (one more
    lbbnn_eval_uncertainty call per batch, no host read); its ``result()`` -- one more copy at the end -- is merged into the
    returned dict under its own keys (the three counts both keep, ``rows``, ``rows_with_target`` and ``bad_targets``, are
    ``acc``'s).
    A network with ``head="identity"`` (LRT / MNF, or its frozen model) is a regression pass: ``acc`` is then required and must
    be a ``RegressionAccumulator`` (its ``update`` takes the raw outputs, the float32 (B, units) targets and the posterior-mean
    forward), ``uncertainty`` must be None; any other pairing is a ValueError naming the mismatch."""
    S = int(samples)
    if _regression_pass(net, acc, uncertainty, "evaluate_batches"):
        # a head="identity" LRT / MNF network or its frozen model: the raw outputs go to acc, a RegressionAccumulator
        if gates != "sample":
            raise ValueError("bnn_amd: gates=%r is not an option of a regression pass" % (gates,))
        for x, y in batches:
            outputs = net.ensemble(x, S) if _is_frozen(net) else ensemble_forward(net, x, S)
            mean = None
            if posterior_mean:
                mean = net(x, sample=False)
            acc.update(outputs, y, mean)
        return acc.result()
    binary = _head_of(net) == "sigmoid"
    for x, y in batches:
        outputs, mean = _eval_forwards(net, x, S, posterior_mean, gates)
        if binary and y is not None:
            y = _binary_target(y)                 # float 0 / 1 targets: converted on the device, no host read
        if acc is None:
            acc = EvalAccumulator(outputs.shape[-1], S, outputs.device)
        acc.update(outputs, y, mean)
        if uncertainty is not None:
            uncertainty.update(outputs, y)
    if acc is None:
        raise ValueError("bnn_amd: evaluate_batches got no batches and no accumulator")
    res = acc.result()
    if uncertainty is not None:
        res.update((k, v) for k, v in uncertainty.result().items() if k not in res)
    return res


# ----------------------------------------------------------------------------------------- frozen evaluation model
FROZEN_GATES = ("alpha", "mpm")


def _empty(*size, **kw):
    """Every device buffer of a FrozenNetwork comes from here (the tests hand out NaN-filled ones through it)."""
    return torch.empty(*size, **kw)


def _is_frozen(net) -> bool:
    return isinstance(net, _FrozenModel)


def _cut(threshold) -> float:
    """logit(threshold) as the fp32 value the kernels compare lambdal with (exactly 0 at 0.5); refuses a threshold outside
    (0, 1)."""
    if not 0.0 < float(threshold) < 1.0:
        raise ValueError("bnn_amd: threshold must lie strictly between 0 and 1 (0.5 = the median probability model), got %r"
                         % (threshold,))
    return float(torch.tensor(math.log(threshold / (1.0 - threshold)), dtype=torch.float32))


class _FrozenModel(nn.Module):
    """What every frozen evaluation model is, whichever family it froze: the checked arguments, the shapes (``full_dims`` the
    network's widths, ``dims`` this model's -- the compact widths when ``live`` is given), the statistics read from
    ``kept_rows``, the compact bookkeeping, the input rows as the first GEMM reads them, the head over the members' buffer,
    and the lifetime of cached device addresses.

    A subclass sets ``GATES`` / ``GATES_DOC`` (the gates it takes, and how the refusal words them), ``FREEZE`` (the function
    that builds it), ``_POINTER_STATE`` (the attributes that hold, or follow, device addresses of its buffers) and answers
    ``_device()`` and ``_point()``: ``_point`` builds every long-lived array of addresses from the buffers as they are now and
    drops the cached member buffers; it is the ONE place that does, called when the buffers are made, after ``nn.Module._apply``
    replaced them (``.to()``, ``.float()``, ``.double()``), and on a deep copy."""
    GATES, GATES_DOC, FREEZE = (), "", ""
    _POINTER_STATE = ()

    def __init__(self, full_dims, gates: str, threshold: float, device, head: str, live=None, needed=None):
        super().__init__()
        if head not in ("log_softmax", "sigmoid", "identity"):
            raise ValueError("bnn_amd: head must be 'log_softmax', 'sigmoid' or 'identity', got %r" % (head,))
        self._check_gates(gates)
        threshold = float(threshold)
        self.cut = _cut(threshold)
        self.full_dims = tuple(int(d) for d in full_dims)
        self.compact = live is not None
        if self.compact:
            if gates != "mpm":
                raise ValueError("bnn_amd: a compact model needs gates=\"mpm\"")
            if len(live) != len(self.full_dims) or len(needed) != len(self.full_dims):
                raise ValueError("bnn_amd: a network of %d layers has %d boundaries" % (len(self.full_dims) - 1, len(self.full_dims)))
            self.dims = tuple(int(t.numel()) for t in live)
            self.needed = [int(c) for c in needed]
            for b, t in enumerate(live):
                self.register_buffer("live_%d" % b, t.to(device=device, dtype=torch.int32).contiguous())
        else:
            self.dims = self.full_dims
        if head in ("sigmoid", "identity") and self.dims[-1] > 16:
            raise ValueError("bnn_amd: %s head takes at most 16 output units, got dims[-1] = %d"
                             % ("a sigmoid" if head == "sigmoid" else "an identity", self.dims[-1]))
        # head: carried over from the network: "sigmoid" -> probabilities (or, log_probs=True, 2 classes)
        self.head, self.gates, self.threshold = head, gates, threshold
        self._src = [None]              # the source network, in a list so that it is not registered as a submodule
        self._split, self._layer_ids = [], []
        self._input_identity = self.dims[0] == self.full_dims[0]     # sorted, unique, full width: every feature in place
        self._maps = None
        self._active = self._full_kept = None
        for i in range(len(self.dims) - 1):
            self.register_buffer("kept_rows_%d" % i, torch.zeros(self.dims[i + 1], dtype=torch.int32, device=device))

    @classmethod
    def _check_gates(cls, gates):
        if gates not in cls.GATES:
            raise ValueError("bnn_amd: gates must be %s, got %r" % (cls.GATES_DOC, gates))

    # ------------------------------------------------------------------------------------- statistics
    @property
    def n_layers(self) -> int:
        return len(self.dims) - 1

    def _buf(self, name: str, i: int) -> torch.Tensor:
        return getattr(self, "%s_%d" % (name, i))

    def _n_weights(self) -> int:
        return sum(self.full_dims[i] * self.full_dims[i + 1] for i in range(self.n_layers))

    @property
    def kept_rows(self) -> List[torch.Tensor]:
        """Per layer (O',) int32: weights of each output row past the threshold (lambdal > logit(threshold), that is alpha >
        threshold), in either gates mode; a compact model: among the live columns."""
        return [self._buf("kept_rows", i) for i in range(self.n_layers)]

    @property
    def kept(self) -> List[int]:
        return [int(k.sum()) for k in self.kept_rows]

    @property
    def density(self) -> float:
        """Kept weights / all weights over every layer of the FULL network -- the density the thesis reports for the median
        probability model (a compact model reports what its full model does)."""
        return (int(self._full_kept) if self.compact else sum(self.kept)) / self._n_weights()

    @property
    def live(self) -> List[torch.Tensor]:
        self._need_compact("live")
        return [self._buf("live", b) for b in range(len(self.dims))]

    @property
    def active_kept(self) -> int:
        """Kept weights whose row and column are both needed (over every layer); a compact model only."""
        self._need_compact("active_kept")
        return int(self._active)

    @property
    def active_density(self) -> float:
        return self.active_kept / self._n_weights()

    def _need_compact(self, what: str):
        if not self.compact:
            raise RuntimeError("bnn_amd: %s belongs to a compact model (%s(net, \"mpm\", compact=True))" % (what, self.FREEZE))

    # ------------------------------------------------------------------------------------- compact bookkeeping
    def _count_kept(self, need, masks):
        """``density`` and ``active_kept`` of a compact model from the full network's keep masks and ``live_structure``'s
        ``need``, as device scalars: they are read when asked for, not here."""
        self._full_kept = torch.stack([k.sum() for k in masks]).sum()
        self._active = torch.stack([(k & need[i + 1][:, None] & need[i][None, :]).sum() for i, k in enumerate(masks)]).sum()

    def _compact_maps(self):
        """lbbnn_compact_map_t of every layer of a compact model, addressing its ``live_<b>`` buffers; None for a full one."""
        if not self.compact:
            return None
        from . import _lib
        maps = (_lib.CompactMap * self.n_layers)()
        for i, m in enumerate(maps):
            m.rows, m.cols = self._buf("live", i + 1).data_ptr(), self._buf("live", i).data_ptr()
            m.O_full, m.I_full = self.full_dims[i + 1], self.full_dims[i]
        return maps

    # ------------------------------------------------------------------------------------- cached device addresses
    def _device(self):
        raise NotImplementedError

    def _point(self):
        raise NotImplementedError

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if self._src[0] is not None:
            self._point()                                    # .to() / .float() replaced the buffers the arrays address
        return out

    def __deepcopy__(self, memo):
        """A copy owns its buffers, so it gets arrays of its own (ctypes arrays of addresses are not copied)."""
        import copy
        bound = self._src[0] is not None
        held = dict((k, self.__dict__.pop(k)) for k in self._POINTER_STATE) if bound else {}
        try:
            new = type(self).__new__(type(self))
            memo[id(self)] = new
            new.__dict__ = copy.deepcopy(self.__dict__, memo)
        finally:
            self.__dict__.update(held)
        if bound:
            new._point()
        return new

    # ------------------------------------------------------------------------------------- evaluation
    def _input(self, data):
        """``data`` as the (B, dims[0]) fp32 rows the first GEMM reads: the tensor itself when every input feature is live
        (``_input_identity``) and it already has that form, else the live columns, gathered by ONE launch."""
        width = self.full_dims[0]
        x = data.reshape(-1, width)
        if not x.is_cuda:
            raise RuntimeError("bnn_amd: a frozen model evaluates on a HIP device tensor (data is on %s); there is no CPU path"
                               % data.device)
        dev = self._device()
        if x.device != dev:
            raise RuntimeError("bnn_amd: data is on %s, the frozen model on %s" % (x.device, dev))
        x = x.float() if x.dtype != torch.float32 else x
        if x.stride(1) != 1 or x.stride(0) < width:
            x = x.contiguous()
        B = x.shape[0]
        if self._input_identity:
            if self._split[0]:
                # the bf16 hi | lo kernels read x rows as 16-B vectors through 32-bit offsets
                if B * x.stride(0) * 4 >= 0x7FFFFFF0:
                    raise ValueError("bnn_amd: a batch of %d rows exceeds the 2 GiB the 16-bit kernels address; split it" % B)
                if x.stride(0) % 4 or x.data_ptr() % 16:
                    x = x.clone(memory_format=torch.contiguous_format)
            return x
        from . import _lib
        n_idx = self.dims[0]
        ldo = ops.pad4(n_idx)                                # dense rows on 16-B boundaries: what the bf16 hi | lo kernels read
        if self._split[0] and B * ldo * 4 >= 0x7FFFFFF0:
            raise ValueError("bnn_amd: a batch of %d rows exceeds the 2 GiB the 16-bit kernels address; split it" % B)
        out = _empty((B, ldo), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().lbbnn_gather_columns(x.data_ptr(), x.stride(0), self._buf("live", 0).data_ptr(), n_idx,
                                                       out.data_ptr(), ldo, B, torch.cuda.current_stream(dev).cuda_stream),
                       "lbbnn_gather_columns")
        return out[:, :n_idx] if ldo != n_idx else out

    def _finish(self, buf, S: int, B: int, log_probs: bool):
        """The (S, B, C) result from the (S, pad4(B * C)) buffer the last member GEMM wrote."""
        return _members_result(buf, S, B, self.dims[-1], self.head, log_probs)


def _z_copies(fz, layers):
    """(dst, src) of the copies that snapshot q0 and the z flow of every MNF layer into the buffers of ``fz`` (a frozen model
    or a threshold sweep)."""
    dst, src = [], []
    for i, l in enumerate(layers):
        if not l._mnf:
            continue
        dst += [fz._buf("q0_mean", i), fz._buf("q0_log_var", i)]
        src += [l.q0_mean.detach(), l.q0_log_var.detach()]
        for t, tr in enumerate(l.z_flow.transforms):
            if getattr(fz, "flows", None) == "dense":
                ps = dict(tr.named_parameters())
                for k in fz._zflow_names[i][t]:
                    dst.append(getattr(fz, fz._zflow_buf(i, t, k))); src.append(ps[k].detach())
            else:
                dst += [fz._buf("flow_u", i)[t], fz._buf("flow_w", i)[t], fz._buf("flow_b", i)[t]]
                src += [tr.u.detach().reshape(-1), tr.w.detach().reshape(-1), tr.bias.detach().reshape(-1)]
    return dst, src


class FrozenNetwork(_FrozenModel):
    """A trained LRT / MNF network frozen for evaluation (built by ``freeze``; no parameters, buffers only).

    Per layer it holds ``e0`` = weight_mu * a as plain fp32 rows, the GEMM operands ``e_w`` (of e0) and ``var_w`` (of
    sigma^2 a^2) in the format of the network's precision at freeze time (fp32, or bf16 hi | lo under any 16-bit setting: the
    member dimension of the ensemble kernels exists in that format only), ``bias_var``, a copy of ``bias_mu`` and -- MNF -- of
    ``q0_mean``, ``q0_log_var`` and the z flow (``flows`` = "planar": u, w, b per transform; "dense": every parameter of
    the RNVP / MNF-type coupling networks, buffers ``zflow_<layer>_<transform>_<name>``; the r flow is not copied: evaluation
    never runs it), and ``kept_rows``: per output row the number of weights with
    ``lambdal > logit(threshold)``.  The gate value a is alpha = sigmoid(lambdal) (``gates="alpha"``: today's evaluation
    forward) or the indicator of ``lambdal > logit(threshold)`` (``gates="mpm"``: the median probability model at the default
    threshold 0.5); the bias and z are never gated.  Nothing here follows the source network's parameters until ``refresh()``.
    """
    GATES, FREEZE = FROZEN_GATES, "freeze"
    GATES_DOC = "'alpha' (the gates as trained) or 'mpm' (the median probability model)"
    _POINTER_STATE = ("_zt", "_maps", "_mcap", "_zbuf", "_ewm")

    def __init__(self, dims, family: str = "lrt", gates: str = "alpha", threshold: float = 0.5, device=None,
                 flows: Optional[str] = None, head: str = "log_softmax"):
        super().__init__(dims, gates, threshold, device, head)
        self._init_family(family, flows)

    def _init_family(self, family, flows):
        if family not in ("lrt", "mnf"):
            raise ValueError("bnn_amd: family must be 'lrt' or 'mnf', got %r" % (family,))
        flows = ("planar" if family == "mnf" else None) if flows is None else flows
        if flows not in ((None,) if family == "lrt" else ("planar", "dense")):
            raise ValueError("bnn_amd: flows must be 'planar' or 'dense' for an MNF model and None for an LRT model, got %r"
                             % (flows,))
        self.family = family
        self.flows = flows              # the z flow family of an MNF model: "planar" | "dense" (RNVP / MNF type); LRT: None
        self.last_z = None
        self.last_masks = None
        # dense flows, per layer: the parameter names and the kind of the coupling networks / the lbbnn_dense_transform_t array
        self._zflow_names, self._zflow_kinds, self._zt = [], [], []
        self._row_offsets, self._T = [], []
        self._members_ok = True
        self._mcap, self._zbuf, self._ewm = 0, None, []
        self._xops = None              # explain's fp32 operands of this snapshot (LRT; made on first use)

    def _device(self):
        return self._buf("e0", 0).device

    def extra_repr(self) -> str:
        flows = ", flows=%s" % self.flows if self.flows else ""
        head = ", head=%s" % self.head if self.head != "log_softmax" else ""
        return "dims=%s, family=%s%s, gates=%s, threshold=%g%s" % (self.dims, self.family, flows, self.gates, self.threshold, head)

    # ------------------------------------------------------------------------------------- snapshot
    @torch.no_grad()
    def _bind(self, net, need=None, masks=None):
        """Allocate every buffer for ``net``'s layers (once), at this model's shapes -- z, q0 and the z flow of an MNF layer
        at the network's widths: the flow runs there -- and take the first snapshot."""
        layers = net._layers()
        f = dict(dtype=torch.float32, device=layers[0].weight_mu.device)
        self._src = [net]
        if masks is not None:
            self._count_kept(need, masks)
        for i, l in enumerate(layers):
            O, I, If = self.dims[i + 1], self.dims[i], self.full_dims[i]
            ld = ops.operand_ld(I)
            # the operand format, by the rule of ensemble_forward_batched (layer._split without an input) at this model's
            # shapes: any 16-bit precision -> bf16 hi | lo where the split kernels take the shape and the rows the previous
            # layer writes stay 16-B aligned
            self._split.append(bool(ops.split_precision(l)) and ops.split_eligible(I, O) and (i == 0 or I % 4 == 0))
            if I % 4 or ld > 2048:
                self._members_ok = False
            for name, shape in (("e0", (O, ld)), ("e_w", (O, ld)), ("var_w", (O, ld)), ("bias_var", (O,)), ("bias_mu", (O,))):
                self.register_buffer("%s_%d" % (name, i), _empty(shape, **f))
            if l._mnf:
                T = len(l.z_flow.transforms)
                self._T.append(T)
                vecs = [("q0_mean", (If,)), ("q0_log_var", (If,))]
                if self.flows == "planar":
                    vecs += [("flow_u", (T, If)), ("flow_w", (T, If)), ("flow_b", (T, 1))]
                for name, shape in vecs:
                    self.register_buffer("%s_%d" % (name, i), _empty(shape, **f))
                if self.flows == "dense":
                    names = []
                    for t, tr in enumerate(l.z_flow.transforms):
                        names.append([k for k, _ in tr.named_parameters()])
                        for k, p in tr.named_parameters():
                            self.register_buffer(self._zflow_buf(i, t, k), _empty(tuple(p.shape), **f))
                    self._zflow_names.append(names)
                    self._zflow_kinds.append(l.z_flow.kind)
            else:
                self._T.append(0)
        self._point()
        return self._snapshot(layers)

    def _point(self):
        """The arrays that outlive a call: the transforms of dense z flows and the maps of a compact model, addressing this
        model's buffers as they are now; the member buffers start over."""
        self._zt = [self._dense_transforms(i, kind) for i, kind in enumerate(self._zflow_kinds)]
        self._maps = self._compact_maps()
        self._mcap, self._zbuf, self._ewm = 0, None, []
        self._xops = None

    def _snapshot(self, layers):
        return self.refresh()

    @staticmethod
    def _zflow_buf(i: int, t: int, name: str) -> str:
        return "zflow_%d_%d_%s" % (i, t, name.replace(".", "_"))

    def _dense_transforms(self, i: int, kind: str):
        """lbbnn_dense_transform_t of every transform of layer i's z flow, pointing at this model's copies."""
        from . import _lib
        from .flows import dense_hidden
        T = self._T[i]
        hidden = [dense_hidden(kind, {k: getattr(self, self._zflow_buf(i, t, k)) for k in self._zflow_names[i][t]})
                  for t in range(T)]
        arr = (_lib.DenseTransform * max(T, 1))()
        for t in range(T):
            g = lambda k: getattr(self, self._zflow_buf(i, t, k))
            d = arr[t]
            if kind == "RNVP":                               # flows2.py:188-219: 4-layer MLP, shift (t) and scale (s) heads
                d.kind, d.hidden = 0, hidden[t]
                d.w_in, d.b_in = g("network.0.weight").data_ptr(), g("network.0.bias").data_ptr()
                for m, k in enumerate((2, 4, 6)):
                    d.w_mid[m], d.b_mid[m] = g("network.%d.weight" % k).data_ptr(), g("network.%d.bias" % k).data_ptr()
                a, b = "t", "s"
            else:                                            # flows2.py:225-241: f, then the g (mu) and k (sigma) heads
                d.kind, d.hidden = 1, hidden[t]
                d.w_in, d.b_in = g("f.weight").data_ptr(), g("f.bias").data_ptr()
                a, b = "g", "k"
            d.w_a, d.b_a = g(a + ".weight").data_ptr(), g(a + ".bias").data_ptr()
            d.w_b, d.b_b = g(b + ".weight").data_ptr(), g(b + ".bias").data_ptr()
        return arr

    def _descs(self, src_layers=None):
        """lbbnn_frozen_desc_t of every layer; with ``src_layers`` the parameter pointers are filled too (refresh)."""
        from . import _lib
        n = self.n_layers
        descs = (_lib.FrozenDesc * n)()
        for i in range(n):
            d = descs[i]
            d.O, d.I = self.dims[i + 1], self.dims[i]
            d.ld = ops.operand_ld(d.I)
            d.flags = ops.F_SPLIT16 if self._split[i] else 0
            d.mode = 1 if self.gates == "mpm" else 0
            d.cut, d.layer_id = self.cut, self._layer_ids[i]
            d.e0, d.e_w, d.var_w = (self._buf(k, i).data_ptr() for k in ("e0", "e_w", "var_w"))
            d.bias_var, d.kept_rows = self._buf("bias_var", i).data_ptr(), self._buf("kept_rows", i).data_ptr()
            if src_layers is not None:
                l = src_layers[i]
                for name in ("weight_mu", "weight_rho", "lambdal"):
                    if not getattr(l, name).is_contiguous():
                        raise RuntimeError("bnn_amd: %s of layer %d is not contiguous" % (name, i + 1))
                d.weight_mu, d.weight_rho, d.lambdal = l.weight_mu.data_ptr(), l.weight_rho.data_ptr(), l.lambdal.data_ptr()
                d.bias_rho = l.bias_rho.data_ptr()
            if self.family == "mnf":
                d.q0_mean, d.q0_log_var = self._buf("q0_mean", i).data_ptr(), self._buf("q0_log_var", i).data_ptr()
                if self.flows == "planar":
                    u, w, b = self._buf("flow_u", i), self._buf("flow_w", i), self._buf("flow_b", i)
                    d.z_flow.T = self._T[i]
                    for t in range(self._T[i]):
                        d.z_flow.u[t], d.z_flow.w[t], d.z_flow.b[t] = u[t].data_ptr(), w[t].data_ptr(), b[t].data_ptr()
        return descs

    @torch.no_grad()
    def refresh(self):
        """Take the snapshot again from the source network's current parameters, into the same buffers: ONE
        lbbnn_frozen_operands launch for all layers, plus copies of the small vectors (bias_mu; q0 and the z flow of an MNF
        layer -- the coupling networks of a dense flow ride in the same fused copy).  For evaluate-every-epoch loops."""
        from . import _lib
        net = self._src[0]
        if net is None:
            raise RuntimeError("bnn_amd: this FrozenNetwork is not bound to a network; build it with evaluate.freeze(net)")
        layers = net._layers()
        _check_freezable_layers(layers, dense=self.flows == "dense")
        if self.family == "mnf" and any(l._check_flows() != self.flows for l in layers):
            raise RuntimeError("bnn_amd: the source network's flows changed family since freeze(); freeze it again")
        dev = self._buf("e0", 0).device
        if layers[0].weight_mu.device != dev:
            raise RuntimeError("bnn_amd: the source network moved from %s to %s since freeze(); freeze it again"
                               % (dev, layers[0].weight_mu.device))
        self._layer_ids = [int(l._layer_id) for l in layers]
        self._row_offsets = [int(l.row_offset) for l in layers]
        self._xops = None                                    # explain's operands belong to the old snapshot
        dst, src = _z_copies(self, layers)
        dst += [self._buf("bias_mu", i) for i in range(self.n_layers)]
        src += [l.bias_mu.detach() for l in layers]
        torch._foreach_copy_(dst, src)                       # the small vectors of every layer in one fused copy
        descs = self._descs(layers)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for k, cnt in _lib.layer_groups(self.n_layers):
                _lib.check(_lib.lib().lbbnn_frozen_operands(_lib.group_slice(descs, k, cnt), cnt, stream), "lbbnn_frozen_operands")
        return self

    # ------------------------------------------------------------------------------------- evaluation
    def _member_buffers(self, c: int):
        """z [c][sum of ld] (every MNF layer's block side by side: one member stride, one flow launch; at the network's widths:
        the flow runs there, and the scale launch of a compact model gathers) and the member mean operands [c][O][ld] per
        layer at this model's shapes; allocated for the largest chunk seen, smaller chunks use a prefix."""
        if c > self._mcap:
            f = dict(dtype=torch.float32, device=self._device())
            self._zbuf = _empty((c, sum(ops.operand_ld(d) for d in self.full_dims[:-1])), **f)
            self._ewm = [_empty((c, self.dims[i + 1], ops.operand_ld(self.dims[i])), **f) for i in range(self.n_layers)]
            self._mcap = c
        return self._zbuf, self._ewm

    def _draw_members(self, c: int, rng, stream, masks=None):
        """MNF: member m's z at Philox offset rng[1] + m and its mean operand E0 * z_m (lbbnn_frozen_members; dense flows:
        lbbnn_frozen_members_dense, with ``masks`` a list that receives per layer the (c, T, I) masks the members used; a
        compact model: lbbnn_frozen_members_compact -- the flow launch of the full model at the full width, then one scale
        launch with the gather z_m[cols] fused in)."""
        from . import _lib
        zbuf, ewm = self._member_buffers(c)
        descs = self._descs()
        off = 0
        for i in range(self.n_layers):
            descs[i].z_fwd = zbuf.data_ptr() + 4 * off
            descs[i].z_mstride = zbuf.stride(0)
            descs[i].e_w_members = ewm[i].data_ptr()
            off += ops.operand_ld(self.full_dims[i])
        if self.flows == "dense":
            import ctypes
            fl = (_lib.DenseMembers * self.n_layers)()
            for i in range(self.n_layers):
                d = fl[i]
                d.q0_mean, d.q0_log_var = descs[i].q0_mean, descs[i].q0_log_var
                d.zt = ctypes.cast(self._zt[i], ctypes.POINTER(_lib.DenseTransform))
                d.T, d.I, d.layer_id = self._T[i], self.dims[i], self._layer_ids[i]
                d.z_fwd, d.z_mstride = descs[i].z_fwd, descs[i].z_mstride
                if masks is not None:
                    masks.append(_empty((c, self._T[i], self.dims[i]), dtype=torch.float32, device=zbuf.device))
                    d.mask_out = masks[-1].data_ptr()
            for k, cnt in _lib.layer_groups(self.n_layers):      # one z buffer, one call per group; the caller advances once
                _lib.check(_lib.lib().lbbnn_frozen_members_dense(_lib.group_slice(descs, k, cnt), _lib.group_slice(fl, k, cnt), cnt,
                                                                 c, rng.data_ptr(), 1, stream), "lbbnn_frozen_members_dense")
            return zbuf, ewm
        for k, cnt in _lib.layer_groups(self.n_layers):
            if self._maps is not None:
                _lib.check(_lib.lib().lbbnn_frozen_members_compact(_lib.group_slice(descs, k, cnt), _lib.group_slice(self._maps, k, cnt),
                                                                   cnt, c, rng.data_ptr(), 1, stream), "lbbnn_frozen_members_compact")
            else:
                _lib.check(_lib.lib().lbbnn_frozen_members(_lib.group_slice(descs, k, cnt), cnt, c, rng.data_ptr(), 1, stream),
                           "lbbnn_frozen_members")
        return zbuf, ewm

    def _z_of(self, zbuf, c):
        out, off = [], 0
        for i in range(self.n_layers):
            out.append(zbuf[:c, off:off + self.full_dims[i]].clone())
            off += ops.operand_ld(self.full_dims[i])
        return out

    def _chunk(self, x, c: int, st, head, zs, ms=None):
        """Members live .. live + c - 1 of the ensemble into head (c, pad4(B * classes)): MNF 2 launches for z and the member
        operands, then one lbbnn_lrt_gemm_members launch per layer."""
        dev, n = x.device, self.n_layers
        rng = st.t
        stream = torch.cuda.current_stream(dev).cuda_stream
        mnf = self.family == "mnf"
        if mnf:
            masks = [] if ms is not None else None
            zbuf, ewm = self._draw_members(c, rng, stream, masks)
            if zs is not None:
                zs.append(self._z_of(zbuf, c))
            if ms is not None:
                ms.append(masks)
        buf = self._buf
        chain = [(ewm[i] if mnf else buf("e_w", i), buf("bias_mu", i), self._split[i], buf("var_w", i), buf("bias_var", i),
                  ops.STREAM_EPS_OUT * 64 + self._layer_ids[i], self._row_offsets[i]) for i in range(n)]
        ops.member_gemm_chain(x, c, chain, head=self.head, out=head, empty=_empty, rng=rng, stream=stream)
        st.advance(c)                                        # as c single forwards would have

    def _chain(self, x, st, e_ws, stochastic: bool, log_probs: bool = False):
        """One member as a chain of single lbbnn_lrt_gemm calls on the frozen operands, drawing at the live offset."""
        h, n = x, self.n_layers
        for i in range(n):
            O, I = self.dims[i + 1], self.dims[i]
            last = i == n - 1
            h = ops.lrt_gemm(h, e_ws[i], self._buf("var_w", i), I=I, O=O, bias_mean=self._buf("bias_mu", i),
                             bias_var=self._buf("bias_var", i), rng=st.t, rng_stream=ops.STREAM_EPS_OUT * 64 + self._layer_ids[i],
                             row_offset=self._row_offsets[i], relu=not last, mean_only=not stochastic,
                             log_softmax=last and O <= 16 and self.head == "log_softmax", split=self._split[i], single=False)
        if self.head == "sigmoid":
            return ops.binary_head(h, log_probs=True, want_probs=False) if log_probs else ops.binary_head(h, probs=h)
        if self.head == "identity":
            return h
        return h if self.dims[-1] <= 16 else torch.log_softmax(h, dim=1)

    def _chain_keep(self, x, st, e_ws):
        """``_chain``'s posterior-mean forward for ``evaluate.explain``: the same lbbnn_lrt_gemm calls on the same operands,
        with the hidden activations kept and the last layer left before the head -- (logits, [h_1 .. h_{L-1}]).  The hidden
        layers are the bits ``_chain`` computes; the logits are what ``head="identity"`` returns."""
        h, n, hs = x, self.n_layers, []
        for i in range(n):
            O, I = self.dims[i + 1], self.dims[i]
            last = i == n - 1
            h = ops.lrt_gemm(h, e_ws[i], self._buf("var_w", i), I=I, O=O, bias_mean=self._buf("bias_mu", i),
                             bias_var=self._buf("bias_var", i), rng=st.t, rng_stream=ops.STREAM_EPS_OUT * 64 + self._layer_ids[i],
                             row_offset=self._row_offsets[i], relu=not last, mean_only=True, log_softmax=False,
                             split=self._split[i], single=False)
            if not last:
                hs.append(h)
        return h, hs

    def _explain_operands(self, e_ws, stream):
        """What the sweep of ``evaluate.explain`` multiplies by, per layer: ``rows`` -- the mean operand the forward read, as
        fp32 rows [O][operand_ld(I)] (an fp32 operand is used where it lies; a bf16 hi | lo operand becomes hi + lo, exact in
        fp32: lbbnn_explain_operand) -- and ``wt`` -- its transpose as an fp32 GEMM operand [I][operand_ld(O)]
        (lbbnn_transpose_operand; None for the last layer, whose rows seed the sweep).  An LRT model keeps them until the next
        snapshot (``refresh``, ``.to()``); an MNF model's operands carry this call's z and are made per call."""
        from . import _lib
        keep = self.family == "lrt"
        if keep and self._xops is not None:
            return self._xops
        rows, wts = [], []
        for i in range(self.n_layers):
            O, I = self.dims[i + 1], self.dims[i]
            ld = ops.operand_ld(I)
            w = e_ws[i]
            if self._split[i]:
                w32 = _empty((O, ld), dtype=torch.float32, device=w.device)
                _lib.check(_lib.lib().lbbnn_explain_operand(w.data_ptr(), O, I, ld, w32.data_ptr(), stream), "lbbnn_explain_operand")
                w = w32
            rows.append(w)
            wts.append(ops.transpose_operand(w[:, :I]) if i < self.n_layers - 1 else None)
        if keep:
            self._xops = (rows, wts)
        return rows, wts

    @torch.no_grad()
    def ensemble(self, data: torch.Tensor, samples: int = 10, *, max_members: Optional[int] = None,
                 keep_z: bool = False, keep_masks: bool = False, log_probs: bool = False) -> torch.Tensor:
        """(samples, B, classes) log-probabilities of ``samples`` stochastic forwards of the frozen model.  Member m draws where
        the m-th member of ``ensemble_forward_batched`` draws: eps of layer i from stream STREAM_EPS_OUT * 64 + layer id with the
        layer's row_offset at Philox offset live + m, z of an MNF layer from its q0 and z flow at the same offset.  The live
        offset advances by ``samples``.  ``max_members``: members per launch (default: all); chunked and unchunked results are
        the same bits.  ``keep_z``: ``self.last_z`` = per layer the (samples, in_features) z every member used (None entries for
        an LRT model).  ``keep_masks`` (dense flows): ``self.last_masks`` = per layer the (samples, T, in_features) Bernoulli
        masks of the coupling transforms every member used (None for any other model).  An LRT model with a layer the member GEMM does not take (in_features % 4 != 0 or an operand row wider
        than 2048) runs every member as a chain of single GEMM calls on the frozen operands instead -- same draws, same shape.
        A model with ``head == "sigmoid"``: (samples, B, units) probabilities -- one lbbnn_binary_head launch over the members'
        logits, no draws of its own -- or, with ``log_probs=True`` (one unit), the (samples, B, 2) log-probabilities of the two
        classes from the same launch."""
        _check_log_probs(self, log_probs)
        S, chunk = _member_counts(samples, max_members)
        x = self._input(data)
        B, C, dev = x.shape[0], self.dims[-1], x.device
        st = ops.RngState.get(dev)
        self.last_z = self.last_masks = None
        with torch.cuda.device(dev):
            if B == 0:
                if self.flows == "dense" and (keep_z or keep_masks):   # no rows to evaluate, but the members' draws exist
                    zs, ms = [], []
                    stream = torch.cuda.current_stream(dev).cuda_stream
                    for m0 in range(0, S, chunk):
                        c = min(chunk, S - m0)
                        ms.append([])
                        zs.append(self._z_of(self._draw_members(c, st.t, stream, ms[-1])[0], c))
                        st.advance(c)
                    self.last_z = [torch.cat(parts) for parts in zip(*zs)] if keep_z else None
                    self.last_masks = [torch.cat(parts) for parts in zip(*ms)] if keep_masks else None
                else:
                    st.advance(S)
                return torch.zeros((S, 0, 2 if log_probs else C), dtype=torch.float32, device=dev)
            if not self._members_ok:                         # (LRT only: freeze refuses such an MNF network)
                outs = []
                for _ in range(S):
                    outs.append(self._chain(x, st, [self._buf("e_w", i) for i in range(self.n_layers)], True, log_probs))
                    st.advance(1)
                if keep_z:
                    self.last_z = [None] * self.n_layers
                return torch.stack(outs)
            head = _empty((S, ops.pad4(B * C)), dtype=torch.float32, device=dev)
            zs = [] if (keep_z and self.family == "mnf") else None
            ms = [] if (keep_masks and self.flows == "dense") else None
            for m0 in range(0, S, chunk):
                c = min(chunk, S - m0)
                self._chunk(x, c, st, head[m0:m0 + c], zs, ms)
        if ms is not None:
            self.last_masks = [torch.cat(parts) for parts in zip(*ms)]
        if keep_z:
            self.last_z = [torch.cat(parts) for parts in zip(*zs)] if zs is not None else [None] * self.n_layers
        return self._finish(head, S, B, log_probs)

    @torch.no_grad()
    def forward(self, data: torch.Tensor, sample: bool = False, *, log_probs: bool = False) -> torch.Tensor:
        """(B, classes) log-probabilities of one member.  ``sample=True``: member 0 of ``ensemble(data, 1)``.
        ``sample=False``: the posterior-mean branch x . E0^T + bias_mu (LBBNN-GP-MF-LRT.py:178-180); an MNF model still draws
        its z (LBBNN-GP-MF-MNF.py:203) and advances the live offset by 1, an LRT model draws nothing.  A sigmoid head:
        (B, units) probabilities, or with ``log_probs=True`` (one unit) the (B, 2) log-probabilities."""
        _check_log_probs(self, log_probs)
        if sample:
            return self.ensemble(data, 1, log_probs=log_probs)[0]
        x = self._input(data)
        dev = x.device
        st = ops.RngState.get(dev)
        with torch.cuda.device(dev):
            if self.family == "mnf":
                _, ewm = self._draw_members(1, st.t, torch.cuda.current_stream(dev).cuda_stream)
                out = self._chain(x, st, [e[0] for e in ewm], False, log_probs)
                st.advance(1)
                return out
            return self._chain(x, st, [self._buf("e_w", i) for i in range(self.n_layers)], False, log_probs)


def _check_freezable_layers(layers, dense: bool = False):
    from . import _lib
    if len(layers) > _lib.MAX_DEPTH:
        raise ValueError("bnn_amd: freeze takes networks of at most %d layers" % _lib.MAX_DEPTH)
    for i, l in enumerate(layers):
        if l.noise:
            raise ValueError("bnn_amd: layer %d has injected noise (layer.noise); a frozen model draws in-kernel noise only -- "
                             "clear it, or evaluate with ensemble_forward(net, data, samples, batched=False)" % (i + 1))
        if getattr(l, "as_written", False):
            raise ValueError("bnn_amd: layer %d has as_written set; a frozen model implements the corrected forward only -- "
                             "evaluate such a network with ensemble_forward(net, data, samples, batched=False)" % (i + 1))
        if l._mnf and dense and l._check_flows() == "dense":
            I, T = l.in_features, len(l.z_flow.transforms)
            loop = "evaluate this network with the loop form, ensemble_forward(net, data, samples)"
            if any(ll._mnf and ll._check_flows() != "dense" for ll in layers):
                raise ValueError("bnn_amd: layer %d has dense z flows, another layer has not; a frozen model takes one flow "
                                 "family for all layers; %s" % (i + 1, loop))
            if I % 4:
                raise ValueError("bnn_amd: layer %d: a frozen model with dense z flows needs in_features %% 4 == 0 "
                                 "(in_features = %d); %s" % (i + 1, I, loop))
            lim = int(_lib.lib().lbbnn_flow_dense_members_max_dim())
            if I > lim:
                raise ValueError("bnn_amd: layer %d: in_features = %d is beyond what the member kernel of the dense z flows holds "
                                 "in LDS (%d); %s" % (i + 1, I, lim, loop))
            if T > _lib.MAX_DENSE_T:
                raise ValueError("bnn_amd: layer %d: z_flow has %d transforms, the member kernel of the dense z flows takes at "
                                 "most %d; %s" % (i + 1, T, _lib.MAX_DENSE_T, loop))
            from .flows import dense_hidden
            for tr in l.z_flow.transforms:
                try:
                    dense_hidden(l.z_flow.kind, dict(tr.named_parameters()))
                except ValueError as e:
                    # (no forward of this library takes such a flow: the loop form refuses it with the same words)
                    raise ValueError("bnn_amd: layer %d: z_flow: %s" % (i + 1, str(e).replace("bnn_amd: ", ""))) from None
        elif l._mnf:
            if l._check_flows() != "planar" or len(l.z_flow.transforms) > 4:
                raise ValueError("bnn_amd: layer %d: a frozen MNF model needs planar flows with at most 4 transforms (it has "
                                 "z_flow=%s with %d); evaluate this network with ensemble_forward(net, data, samples)"
                                 % (i + 1, l.z_flow.kind, len(l.z_flow.transforms)))
            if l.in_features % 4 or ops.operand_ld(l.in_features) > 2048:
                raise ValueError("bnn_amd: layer %d: a frozen MNF model needs in_features %% 4 == 0 and operand rows of at most "
                                 "2048 (in_features = %d); evaluate this network with ensemble_forward(net, data, samples)"
                                 % (i + 1, l.in_features))


# ----------------------------------------------------------------------------------------- compact median-probability model
def _live_structure(keep_masks, align: int):
    """``live_structure`` plus the needed counts as host integers (ONE device read for all boundaries)."""
    n = len(keep_masks)
    if n < 1:
        raise ValueError("bnn_amd: live_structure needs at least one keep mask")
    align = int(align)
    if align < 1:
        raise ValueError("bnn_amd: align must be >= 1, got %d" % align)
    for i, k in enumerate(keep_masks):
        if k.dim() != 2 or k.dtype != torch.bool:
            raise ValueError("bnn_amd: keep mask %d must be a 2-d bool tensor (out_features, in_features)" % i)
        if i and k.shape[1] != keep_masks[i - 1].shape[0]:
            raise ValueError("bnn_amd: keep mask %d has %d columns, the layer below %d rows" % (i, k.shape[1], keep_masks[i - 1].shape[0]))
    dev = keep_masks[0].device
    need = [None] * (n + 1)
    need[n] = torch.ones(keep_masks[-1].shape[0], dtype=torch.bool, device=dev)
    for i in range(n - 1, -1, -1):                           # one backward sweep: a unit is needed iff a needed unit keeps it
        need[i] = (keep_masks[i] & need[i + 1][:, None]).any(0)
    counts = torch.stack([nd.sum() for nd in need]).tolist()
    live = []
    for b, nd in enumerate(need):
        w = nd.numel()
        size = w if b == n else min(w, max(align, -(-counts[b] // align) * align))
        idx = torch.arange(w, device=dev)
        # needed units first (by index), then the unneeded ones by index: the first `size` of that order, sorted again
        order = torch.sort(torch.where(nd, idx, idx + w)).indices[:size]
        live.append(torch.sort(order).values.to(torch.int32))
    return need, live, [int(c) for c in counts]


def live_structure(keep_masks, align: int = 8):
    """The units of a pruned network that some output depends on.  ``keep_masks``: per layer the (out_features, in_features)
    bool mask of the kept weights (CPU or HIP tensors).  A network of n layers has n + 1 boundaries: 0 = the input features,
    n = the output units.  Returns ``(need, live)``:

    ``need[b]`` (bool, width of boundary b): ``need[n]`` is all true and ``need[i][j] = any_o(need[i+1][o] & keep_i[o][j])``
    -- a unit is needed iff a needed unit keeps a weight from it.  A needed unit with no kept input stays: it still emits
    relu(bias + noise).
    ``live[b]`` (sorted int32 indices): the needed units of boundary b, topped up with the lowest-index unneeded units to
    ``min(width_b, max(align, ceil_to_align(count)))`` units; ``live[n]`` is every output unit.  Topping up with dead units
    is exact -- everything that consumes them has weight 0 and variance 0 -- and keeps the widths multiples of ``align``
    (8: what the member GEMM, in_features % 4, and the bf16 hi | lo kernels, in_features % 8, take)."""
    need, live, _ = _live_structure(keep_masks, align)
    return need, live


# ----------------------------------------------------------------------------------------- posterior over structures
@torch.no_grad()
def structure_posterior(net, samples: int = 1000, *, rng: Optional[torch.Tensor] = None, max_members: Optional[int] = None,
                        keep_need: bool = False) -> Dict[str, object]:
    """The posterior over the sparse architectures of a latent-binary network (LRT, MNF or baseline, any depth), from
    ``samples`` draws of every gate matrix: ONE lbbnn_gate_structure launch per chunk of at most ``max_members`` samples
    (default: all) draws gamma ~ Bernoulli(sigmoid(lambdal)) from Philox and runs ``live_structure``'s sweep on it without
    storing a gate.  A network of n layers has n + 1 boundaries (0 = the input features, n = the outputs).  Device tensors:

    ``kept`` (S, n) int32: the gates drawn 1 per layer; ``needed`` (S, n + 1) int32: the units of each boundary some output
    depends on; ``active_kept`` (S, n) int32: the kept weights of needed rows (their columns are needed by construction);
    ``density`` / ``active_density`` (S,) fp64: their sums over the layers divided by all weights (``density[s]`` is the
    ``density[i]`` of the reference's ``test_ensemble``); ``feature_count`` (I0,) int32 and ``feature_prob`` = count / S: how
    often an input feature lies on an active path to some output; ``unit_count`` / ``unit_prob``: the same per hidden
    boundary (a list, empty for one layer); with ``keep_need``: ``need``, per boundary the (S, width) bool masks.

    Sample s draws at Philox offset (live offset + s) with the gate stream of each layer, and the live offset advances by
    ``samples`` -- what ``base_ensemble`` does: for a baseline network with hard gates (``layer.gamma.exact``) these are the
    structures of the very members ``base_ensemble(net, x, samples)`` draws from the same state.  ``rng``: an explicit
    {seed, offset} int64 device tensor to draw from instead; nothing is advanced then.  Chunked and unchunked calls give the
    same bits.  No host read: with ``rng`` the call can be captured in a HIP graph.  Layers are at most 4096 wide."""
    from . import _lib, layers as L
    if _is_frozen(net):
        raise ValueError("bnn_amd: structure_posterior draws the gates of a live network; a frozen model has fixed its gates "
                         "(its structure is net.density / evaluate.live_structure)")
    if _is_vd(net):
        raise ValueError("bnn_amd: structure_posterior takes a latent-binary network (LRT, MNF or baseline); a "
                         "variational-dropout network has no gates")
    if not (_is_base(net) or isinstance(net, L._NetworkBase)):
        raise ValueError("bnn_amd: structure_posterior takes an LRT, MNF or baseline LBBNN network, got %s" % type(net).__name__)
    S, chunk = _member_counts(samples, max_members)
    chunk = min(chunk, 65535)
    layers = net._layers()
    n = len(layers)
    for i, l in enumerate(layers):
        if max(l.in_features, l.out_features) > _lib.STRUCTURE_MAX_WIDTH:
            raise ValueError("bnn_amd: layer %d is %d x %d: structure_posterior takes layers of at most %d units a side"
                             % (i + 1, l.out_features, l.in_features, _lib.STRUCTURE_MAX_WIDTH))
    lams = [l.lambdal.detach() for l in layers]
    dev = lams[0].device
    if not all(t.is_cuda for t in lams):
        raise RuntimeError("bnn_amd: structure_posterior needs the network on a HIP device (lambdal is on %s); there is no CPU path"
                           % dev)
    if rng is not None and (not rng.is_cuda or rng.dtype != torch.int64 or rng.numel() < 2 or not rng.is_contiguous()):
        raise RuntimeError("bnn_amd: rng must be a contiguous int64 {seed, offset} tensor on a HIP device; there is no CPU path")
    descs, width = ops.structure_descs(lams, [int(l._layer_id) for l in layers])
    widths = [layers[0].in_features] + [l.out_features for l in layers]
    if width != sum(widths):
        raise ValueError("bnn_amd: structure_posterior: the layers do not chain (widths %s)" % (widths,))
    i32 = dict(dtype=torch.int32, device=dev)
    kept, needed, active = torch.empty((S, n), **i32), torch.empty((S, n + 1), **i32), torch.empty((S, n), **i32)
    feature_count = torch.zeros(widths[0], **i32)
    unit_count = torch.zeros(sum(widths[1:-1]), **i32) if n > 1 else None
    need_out = torch.empty((S, width), dtype=torch.uint8, device=dev) if keep_need else None
    st = ops.RngState.get(dev) if rng is None else None
    # an explicit state and more than one chunk: a copy walks the chunks' offsets, the caller's tensor stays as it is
    state = st.t if st is not None else (rng if chunk >= S else rng[:2].clone())
    for m0 in range(0, S, chunk):
        c = min(chunk, S - m0)
        ops.gate_structure(descs, n, c, state, kept=kept[m0:m0 + c], needed=needed[m0:m0 + c], active=active[m0:m0 + c],
                           feature_count=feature_count, unit_count=unit_count,
                           need_out=need_out[m0:m0 + c] if keep_need else None)
        if st is not None:
            st.advance(c)
        elif m0 + c < S:
            _lib.check(_lib.lib().lbbnn_rng_advance(state.data_ptr(), c, ops._stream()), "lbbnn_rng_advance")
    # divisors as device tensors: a true fp64 division (by a Python scalar torch multiplies with the rounded reciprocal)
    weights = torch.full((), float(sum(l.in_features * l.out_features for l in layers)), dtype=torch.float64, device=dev)
    count = torch.full((), float(S), dtype=torch.float64, device=dev)
    bounds = [sum(widths[:b]) for b in range(n + 2)]
    hidden = [unit_count[bounds[b] - widths[0]:bounds[b + 1] - widths[0]] for b in range(1, n)]
    res = {"kept": kept, "needed": needed, "active_kept": active,
           "density": kept.sum(1, dtype=torch.float64) / weights, "active_density": active.sum(1, dtype=torch.float64) / weights,
           "feature_count": feature_count, "feature_prob": feature_count.double() / count,
           "unit_count": hidden, "unit_prob": [h.double() / count for h in hidden]}
    if keep_need:
        res["need"] = [need_out[:, bounds[b]:bounds[b + 1]].bool() for b in range(n + 1)]
    return res


class CompactFrozenNetwork(FrozenNetwork):
    """The median probability model without the units no output depends on (``freeze(net, "mpm", compact=True)``): a
    ``FrozenNetwork`` whose ``dims`` are the compact widths, so every GEMM, the ensemble, the accumulators and the graphed
    evaluation step run as for any frozen model, at the smaller shapes.

    ``full_dims``: the source network's widths; ``live``: per boundary the sorted int32 indices of the units that stay
    (buffers ``live_<b>``, ``evaluate.live_structure``); ``needed``: per boundary the number of needed units before the
    top-up to a multiple of 8; ``active_kept`` / ``active_density``: the kept weights whose row and column are both needed,
    and their share of all weights of the full network (the "active paths" density); ``density``: the FULL network's
    density, to compare with; ``kept_rows``: per compact row the kept weights among the live columns.

    Draws: z of an MNF layer is drawn at the full width -- member m's z is the full model's, bit for bit (``keep_z`` returns
    it at full width) -- and gathered inside the launch that scales the member operands; eps_out of a layer is indexed by the
    COMPACT column, so a stochastic member equals the full model's member in distribution, not in numbers.  The
    posterior-mean forward draws no eps_out and equals the full model's to fp32 rounding.  Input rows are gathered to the
    live features by one lbbnn_gather_columns launch; when every input feature is live there is no launch and no copy."""

    def __init__(self, full_dims, live, needed, family: str = "lrt", threshold: float = 0.5, device=None, head: str = "log_softmax"):
        _FrozenModel.__init__(self, full_dims, "mpm", threshold, device, head, live, needed)
        self._init_family(family, None)

    def extra_repr(self) -> str:
        return "full_dims=%s, %s" % (self.full_dims, super().extra_repr())

    def _snapshot(self, layers):
        """THE snapshot: one lbbnn_frozen_operands_compact launch per layer group, index_select of bias_mu, copies of the
        full-width q0 and z flow of an MNF layer."""
        from . import _lib
        if self.family == "mnf" and not self._members_ok:
            raise ValueError("bnn_amd: a compact MNF model needs compact in_features %% 4 == 0 and operand rows of at most 2048 "
                             "(compact dims %s); use freeze(net, \"mpm\") without compact=True" % (self.dims,))
        self._layer_ids = [int(l._layer_id) for l in layers]
        self._row_offsets = [int(l.row_offset) for l in layers]
        for i, l in enumerate(layers):
            torch.index_select(l.bias_mu.detach(), 0, self._buf("live", i + 1).long(), out=self._buf("bias_mu", i))
        dst, src = _z_copies(self, layers)
        if dst:
            torch._foreach_copy_(dst, src)
        descs = self._descs(layers)
        dev = self._device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for k, cnt in _lib.layer_groups(self.n_layers):
                _lib.check(_lib.lib().lbbnn_frozen_operands_compact(_lib.group_slice(descs, k, cnt), _lib.group_slice(self._maps, k, cnt),
                                                                    cnt, stream), "lbbnn_frozen_operands_compact")
        return self

    def refresh(self):
        raise NotImplementedError("bnn_amd: a compact model does not refresh: the structure, and with it every shape, may have "
                                  "changed with the parameters -- freeze again (evaluate.freeze(net, \"mpm\", compact=True))")


def _freeze_compact(net, layers, family, threshold) -> CompactFrozenNetwork:
    dev = layers[0].weight_mu.device
    cut = _cut(threshold)
    # the tie rule of lbbnn_frozen_operands: lambdal > cut compared in fp32 (NaN is never kept)
    masks = [l.lambdal.detach().float() > cut for l in layers]
    need, live, needed = _live_structure(masks, 8)           # the ONE device read: the live counts size every buffer
    fz = CompactFrozenNetwork(net.dims, live, needed, family, threshold, device=dev, head=net.head)
    fz.eval()
    return fz._bind(net, need, masks)


class _SparseModel:
    """What the sparse median probability models share (mixed in before the frozen base): per layer a CSR ``row_ptr_<i>`` /
    ``col_<i>`` / the two value arrays named by ``VALUES``, two dense bias vectors, and ``_nnz``, the kept weights per layer."""

    VALUES = ("mean", "var")

    def _device(self):
        return self._buf("kept_rows", 0).device

    @property
    def nnz(self) -> int:
        """Kept weights over every layer."""
        return sum(self._nnz)

    @property
    def operand_bytes(self) -> int:
        """Bytes of everything the launches read of this model: row_ptr, col, the two value arrays and the two bias vectors."""
        return sum(4 * (self.dims[i + 1] + 1) + 12 * n + 8 * self.dims[i + 1] for i, n in enumerate(self._nnz))

    def csr(self, i: int):
        """(row_ptr, col) and the two value arrays (``VALUES``) of layer i."""
        return tuple(self._buf(k, i) for k in ("row_ptr", "col") + self.VALUES)

    def refresh(self):
        raise NotImplementedError("bnn_amd: a sparse model does not refresh: the structure, and with it the size of every CSR "
                                  "buffer, may have changed with the parameters -- freeze again (evaluate.%s(net, \"mpm\", "
                                  "sparse=True))" % self.FREEZE)


def _pack_csr(mod, descs, count: str, pack: str, extra=(), third: str = "var", kept_out=None):
    """Count, scan, size (the ONE host read), pack -- two batched launches per layer group and one cumsum per layer -- for the
    layers described by ``descs`` (sources, ``kept_rows`` and the per-row destinations filled in): registers ``row_ptr_<i>``,
    ``col_<i>``, ``mean_<i>`` and ``<third>_<i>`` on ``mod`` and returns the kept weights as host ints, [layer][level].
    ``count`` / ``pack``: the C entry points, called with ``extra`` before the stream.  ``kept_rows_<i>`` is (O,), or a sweep's
    (K, O): the scan then runs level after level, and ``kept_out`` (K, layers) takes the level totals on the device."""
    from . import _lib
    n = mod.n_layers
    dev = mod._buf("kept_rows", 0).device
    f = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for k, cnt in _lib.layer_groups(n):
            _lib.check(getattr(_lib.lib(), count)(_lib.group_slice(descs, k, cnt), cnt, *extra, stream), count)
        rows = [mod._buf("kept_rows", i) for i in range(n)]
        levels = rows[0].dim() == 2                          # a sweep's (K, O)
        for i, r in enumerate(rows):
            mod.register_buffer("row_ptr_%d" % i, ops.sparse_row_ptr(r.view(-1) if levels else r))
        # the totals (layers,), the scans' last entries -- a sweep's (layers, K), level by level
        kept = torch.stack([r.sum(1) for r in rows] if levels else [mod._buf("row_ptr", i)[-1] for i in range(n)])
        if kept_out is not None:
            kept_out.copy_(kept.t())
        tot = kept.tolist() if levels else [[t] for t in kept.tolist()]                      # the host read
        for i, t in enumerate(tot):
            cap = sum(t)
            # (col comes from _empty too, as fp32 words: a NaN-filled slot that was never packed is an index out of range)
            mod.register_buffer("col_%d" % i, _empty((cap,), **f).view(torch.int32))
            mod.register_buffer("mean_%d" % i, _empty((cap,), **f))
            mod.register_buffer("%s_%d" % (third, i), _empty((cap,), **f))
            d = descs[i]
            d.row_ptr, d.nnz = mod._buf("row_ptr", i).data_ptr(), cap
            d.col, d.mean = mod._buf("col", i).data_ptr(), mod._buf("mean", i).data_ptr()
            setattr(d, third, mod._buf(third, i).data_ptr())
        for k, cnt in _lib.layer_groups(n):
            _lib.check(getattr(_lib.lib(), pack)(_lib.group_slice(descs, k, cnt), cnt, *extra, stream), pack)
    return tot


def _sparse_sources(mod, net, descs):
    """The LRT / MNF source side of a sparse bind (a model's or a sweep's): the contiguity refusals, the ``bias_mu`` /
    ``bias_var`` buffers and an MNF layer's ``q0_*`` / ``flow_*`` buffers with ONE fused copy of the small vectors into them,
    and every field of ``descs`` but the cuts and what ``_pack_csr`` fills in."""
    layers = net._layers()
    f = dict(dtype=torch.float32, device=layers[0].weight_mu.device)
    mod._src = [net]
    mod._layer_ids = [int(l._layer_id) for l in layers]
    mod._row_offsets = [int(l.row_offset) for l in layers]
    for i, l in enumerate(layers):
        O, If = mod.dims[i + 1], mod.dims[i]
        for name in ("weight_mu", "weight_rho", "lambdal"):
            if not getattr(l, name).is_contiguous():
                raise RuntimeError("bnn_amd: %s of layer %d is not contiguous" % (name, i + 1))
        for name in ("bias_var", "bias_mu"):
            mod.register_buffer("%s_%d" % (name, i), _empty((O,), **f))
        T = len(l.z_flow.transforms) if l._mnf else 0
        mod._T.append(T)
        if l._mnf:
            for name, shape in (("q0_mean", (If,)), ("q0_log_var", (If,)), ("flow_u", (T, If)), ("flow_w", (T, If)),
                                ("flow_b", (T, 1))):
                mod.register_buffer("%s_%d" % (name, i), _empty(shape, **f))
        d = descs[i]
        d.weight_mu, d.weight_rho, d.lambdal = l.weight_mu.data_ptr(), l.weight_rho.data_ptr(), l.lambdal.data_ptr()
        d.bias_rho = l.bias_rho.data_ptr()
        d.bias_var, d.kept_rows = mod._buf("bias_var", i).data_ptr(), mod._buf("kept_rows", i).data_ptr()
        d.O, d.I = O, If
    dst, src = _z_copies(mod, layers)
    dst += [mod._buf("bias_mu", i) for i in range(len(layers))]
    src += [l.bias_mu.detach() for l in layers]
    torch._foreach_copy_(dst, src)                           # the small vectors of every layer in one fused copy


class SparseFrozenNetwork(_SparseModel, FrozenNetwork):
    """The median probability model as its kept weights alone (``freeze(net, "mpm", sparse=True)``): per layer a CSR of the
    weights with ``lambdal > logit(threshold)`` -- buffers ``row_ptr_<i>`` (O + 1) int32, ``col_<i>`` (nnz) int32 ascending
    within a row, ``mean_<i>`` (nnz) = weight_mu, ``var_<i>`` (nnz) = sigma^2 -- plus the dense ``bias_mu``, ``bias_var`` and
    ``kept_rows``.  There is no dense e0 / e_w / var_w operand and no per-member operand: a layer is ONE
    lbbnn_sparse_layer_members launch for all members, on the vector ALU, over the kept weights only, whatever the network's
    precision setting (the model is fp32).  ``csr(i)``: the four tensors of layer i; ``nnz`` / ``operand_bytes``: plain ints.

    Draws: member m draws at Philox offset live + m; eps_out of layer i from stream STREAM_EPS_OUT * 64 + layer id at counter
    (row_offset + b, o / 4) with o the network's own output index, z of an MNF layer from the flow launch of
    ``freeze(net, "mpm")`` (lbbnn_frozen_members_z) -- the draws of the dense median model bit for bit, so a member equals
    that model's member to fp32 rounding (the sums run over the kept weights in column order, sequentially).  The bits of an
    output depend on its member, row and unit alone.  No ``refresh()`` and no ``evaluate.explain``: freeze again, or use
    ``freeze(net, "mpm")``.  ``evaluate.explain_ensemble`` explains this model's sampled-weight members; its first call adds the
    buffers ``col_ptr_<i>`` (I + 1), ``trow_<i>``, ``tslot_<i>``, ``tpos_<i>`` (nnz): the pattern column by column."""

    def __init__(self, dims, family: str = "lrt", threshold: float = 0.5, device=None, head: str = "log_softmax"):
        _FrozenModel.__init__(self, dims, "mpm", threshold, device, head)
        self._init_family(family, None)
        self._nnz = []

    def extra_repr(self) -> str:
        return "%s, sparse, nnz=%d" % (super().extra_repr(), self.nnz)

    @torch.no_grad()
    def _bind(self, net, need=None, masks=None):
        from . import _lib
        n = self.n_layers
        self._split = [False] * n
        descs = (_lib.SparseDesc * n)()
        _sparse_sources(self, net, descs)
        for d in descs:
            d.cut = self.cut
        self._nnz = [t[0] for t in _pack_csr(self, descs, "lbbnn_sparse_count", "lbbnn_sparse_pack")]
        self._point()
        return self

    def _member_buffers(self, c: int):
        """z [c][sum of ld], every MNF layer's block side by side (one member stride, one flow launch); no member operands."""
        if c > self._mcap:
            self._zbuf = _empty((c, sum(ops.operand_ld(d) for d in self.dims[:-1])), dtype=torch.float32, device=self._device())
            self._mcap = c
        return self._zbuf, []

    def _take_z(self, c: int):
        """The z of the c members just drawn, [c][sum of ld], for a caller that hands it on with its result: the buffer itself
        where it holds exactly those members (the model lets go of it; the next draw allocates anew), a copy where the model
        holds a larger one (which it keeps)."""
        zbuf = self._zbuf
        if zbuf.shape[0] > c:
            return zbuf[:c].clone()
        self._zbuf, self._mcap = None, 0
        return zbuf

    def _draw_members(self, c: int, rng, stream, masks=None):
        """MNF: member m's z at Philox offset rng[1] + m -- the flow launch of the dense model alone (lbbnn_frozen_members_z)."""
        from . import _lib
        zbuf, _ = self._member_buffers(c)
        n = self.n_layers
        descs = (_lib.FrozenDesc * n)()
        off = 0
        for i in range(n):
            d = descs[i]
            d.O, d.I, d.layer_id = self.dims[i + 1], self.dims[i], self._layer_ids[i]
            d.q0_mean, d.q0_log_var = self._buf("q0_mean", i).data_ptr(), self._buf("q0_log_var", i).data_ptr()
            u, w, b = self._buf("flow_u", i), self._buf("flow_w", i), self._buf("flow_b", i)
            d.z_flow.T = self._T[i]
            for t in range(self._T[i]):
                d.z_flow.u[t], d.z_flow.w[t], d.z_flow.b[t] = u[t].data_ptr(), w[t].data_ptr(), b[t].data_ptr()
            d.z_fwd, d.z_mstride = zbuf.data_ptr() + 4 * off, zbuf.stride(0)
            off += ops.operand_ld(self.dims[i])
        for k, cnt in _lib.layer_groups(n):
            _lib.check(_lib.lib().lbbnn_frozen_members_z(_lib.group_slice(descs, k, cnt), cnt, c, rng.data_ptr(), 1, stream),
                       "lbbnn_frozen_members_z")
        return zbuf, []

    def _layers_of(self, zbuf, c: int):
        """The per-layer tuples ops.sparse_member_chain takes; zbuf None: an LRT model."""
        out, off = [], 0
        for i in range(self.n_layers):
            z = None if zbuf is None else zbuf[:c, off:off + self.dims[i]]
            off += ops.operand_ld(self.dims[i])
            out.append(self.csr(i) + (self._buf("bias_mu", i), self._buf("bias_var", i), z,
                                      ops.STREAM_EPS_OUT * 64 + self._layer_ids[i], self._row_offsets[i]))
        return out

    def _chunk(self, x, c: int, st, head, zs, ms=None):
        """Members live .. live + c - 1 of the ensemble into head (c, pad4(B * classes)): MNF one flow launch for z, then the
        input transpose and one lbbnn_sparse_layer_members launch per layer."""
        dev = x.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        zbuf = None
        if self.family == "mnf":
            zbuf, _ = self._draw_members(c, st.t, stream)
            if zs is not None:
                zs.append(self._z_of(zbuf, c))
        ops.sparse_member_chain(x, c, self._layers_of(zbuf, c), head=self.head, out=head, empty=_empty, rng=st.t, stream=stream)
        st.advance(c)                                        # as c single forwards would have

    @torch.no_grad()
    def forward(self, data: torch.Tensor, sample: bool = False, *, log_probs: bool = False) -> torch.Tensor:
        """(B, classes) of one member, as ``FrozenNetwork.forward``: ``sample=True`` is member 0 of ``ensemble(data, 1)``;
        ``sample=False`` the posterior-mean branch, for which an MNF model still draws its z and advances the live offset by
        1 and an LRT model draws nothing."""
        _check_log_probs(self, log_probs)
        if sample:
            return self.ensemble(data, 1, log_probs=log_probs)[0]
        x = self._input(data)
        B, C, dev = x.shape[0], self.dims[-1], x.device
        st = ops.RngState.get(dev)
        with torch.cuda.device(dev):
            if B == 0:
                if self.family == "mnf":
                    st.advance(1)
                return torch.zeros((0, 2 if log_probs else C), dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            zbuf = self._draw_members(1, st.t, stream)[0] if self.family == "mnf" else None
            head = _empty((1, ops.pad4(B * C)), dtype=torch.float32, device=dev)
            ops.sparse_member_chain(x, 1, self._layers_of(zbuf, 1), head=self.head, out=head, empty=_empty, stochastic=False,
                                    stream=stream)
            if zbuf is not None:
                st.advance(1)
        return self._finish(head, 1, B, log_probs)[0]


def _freeze_sparse(net, layers, family, threshold) -> SparseFrozenNetwork:
    fz = SparseFrozenNetwork(net.dims, family, threshold, device=layers[0].weight_mu.device, head=net.head)
    fz.eval()
    return fz._bind(net)


# ----------------------------------------------------------------------------------------- threshold sweep
class ThresholdSweep(nn.Module):
    """The sparse median probability models of K ascending thresholds in one set of buffers (``threshold_sweep(net,
    thresholds)``; LRT and planar MNF networks, every head, 1 to 16 layers; buffers only, fp32 whatever the precision setting).

    Per layer i with O rows: ``kept_rows_<i>`` (K, O) int32, ``row_ptr_<i>`` (K * O + 1) int32 -- the exclusive scan of
    kept_rows level after level -- and ``col_<i>`` / ``mean_<i>`` / ``var_<i>``, in which level j, row o owns the slots
    [row_ptr[j * O + o], row_ptr[j * O + o + 1]); ``bias_mu_<i>``, ``bias_var_<i>`` and the q0 / planar-flow copies of an MNF
    layer are shared by the levels.  Level j's segment holds the bits ``freeze(net, "mpm", threshold=thresholds[j],
    sparse=True)`` packs (lbbnn_sparse_count_levels / _pack_levels: every parameter read once, ONE host read of the
    (layers, K) level totals).

    ``ensemble(x, S)`` -> (K, S, B, classes): one lbbnn_frozen_members_z launch for S draws (MNF), one input transpose, and one
    lbbnn_sparse_layer_levels launch per layer for all K * S members.  Member (j, s) is bit for bit member s of level j's own
    model from the same Philox offset: draw s is common to the levels (common random numbers), and the live offset advances by
    S, as ONE model's ensemble advances it.  ``sw(x)`` -> (K, B, classes): the posterior-mean forward of every level; an MNF
    network draws one z, shared by the levels, and advances the offset by 1; an LRT network draws nothing.
    ``model(j)``: level j as a ``SparseFrozenNetwork`` on this sweep's value buffers.

    ``thresholds`` / ``cuts``: the K thresholds and their fp32 logits; ``nnz``: K host ints, the kept weights of each level;
    ``kept``: (K, layers) int64 on the device; ``density``: (K,) float64 on the device, kept / all weights -- the thesis'
    density per level; ``operand_bytes``: what the layer launches read of the sweep."""

    def __init__(self, dims, thresholds, family: str = "lrt", device=None, head: str = "log_softmax"):
        super().__init__()
        from . import _lib
        if head not in ("log_softmax", "sigmoid", "identity"):
            raise ValueError("bnn_amd: head must be 'log_softmax', 'sigmoid' or 'identity', got %r" % (head,))
        if family not in ("lrt", "mnf"):
            raise ValueError("bnn_amd: family must be 'lrt' or 'mnf', got %r" % (family,))
        self.thresholds = tuple(float(t) for t in thresholds)
        if not 1 <= len(self.thresholds) <= _lib.MAX_LEVELS:
            raise ValueError("bnn_amd: a threshold sweep takes 1 to %d thresholds, got %d" % (_lib.MAX_LEVELS, len(self.thresholds)))
        self.cuts = tuple(_cut(t) for t in self.thresholds)
        for j in range(1, len(self.cuts)):
            if not self.thresholds[j - 1] < self.thresholds[j]:
                raise ValueError("bnn_amd: the thresholds of a sweep ascend strictly, got %r" % (self.thresholds,))
            if not self.cuts[j - 1] < self.cuts[j]:
                raise ValueError("bnn_amd: thresholds %r and %r have the same fp32 cut logit(threshold) = %r: they are one level"
                                 % (self.thresholds[j - 1], self.thresholds[j], self.cuts[j]))
        self.dims = self.full_dims = tuple(int(d) for d in dims)
        if head in ("sigmoid", "identity") and self.dims[-1] > 16:
            raise ValueError("bnn_amd: %s head takes at most 16 output units, got dims[-1] = %d"
                             % ("a sigmoid" if head == "sigmoid" else "an identity", self.dims[-1]))
        self.family, self.head = family, head
        self._src = [None]              # the source network, in a list so that it is not registered as a submodule
        self._layer_ids, self._row_offsets, self._T = [], [], []
        self._tot = []                  # [layer][level] kept weights, host ints: the sizes and bases of the segments
        self._level0 = [None]           # model(0), which draws z and lays out x for every level (dropped when the buffers move)
        K = len(self.cuts)
        for i in range(len(self.dims) - 1):
            self.register_buffer("kept_rows_%d" % i, torch.zeros((K, self.dims[i + 1]), dtype=torch.int32, device=device))
        self.register_buffer("kept", torch.zeros((K, len(self.dims) - 1), dtype=torch.int64, device=device))

    def extra_repr(self) -> str:
        head = ", head=%s" % self.head if self.head != "log_softmax" else ""
        return "dims=%s, family=%s, thresholds=%s%s, sparse, nnz=%s" % (self.dims, self.family, self.thresholds, head, self.nnz)

    @property
    def n_layers(self) -> int:
        return len(self.dims) - 1

    def _buf(self, name: str, i: int) -> torch.Tensor:
        return getattr(self, "%s_%d" % (name, i))

    @property
    def nnz(self) -> List[int]:
        """Kept weights of each level, over every layer."""
        return [sum(t[j] for t in self._tot) for j in range(len(self.cuts))]

    @property
    def density(self) -> torch.Tensor:
        """(K,) float64 on the device: kept weights / all weights of each level."""
        kept = self.kept.sum(1).double()
        # (a tensor divisor: dividing by a Python number multiplies by its rounded reciprocal on the device)
        return kept / torch.full_like(kept, sum(self.dims[i] * self.dims[i + 1] for i in range(self.n_layers)))

    @property
    def operand_bytes(self) -> int:
        """Bytes of everything the layer launches read of this sweep: row_ptr, col, mean, var, bias_mu and bias_var."""
        K = len(self.cuts)
        return sum(4 * (K * self.dims[i + 1] + 1) + 12 * sum(t) + 8 * self.dims[i + 1] for i, t in enumerate(self._tot))

    @torch.no_grad()
    def _bind(self, net):
        from . import _lib
        descs = (_lib.SparseLevelsDesc * self.n_layers)()
        _sparse_sources(self, net, descs)
        for d in descs:
            d.levels = len(self.cuts)
            for j, c in enumerate(self.cuts):
                d.cut[j] = c
        self._tot = _pack_csr(self, descs, "lbbnn_sparse_count_levels", "lbbnn_sparse_pack_levels", kept_out=self.kept)
        return self

    # ------------------------------------------------------------------------------------- the buffers move
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._level0 = [None]                                # its views addressed the buffers that were replaced
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._level0 = [None]
        return out

    def __deepcopy__(self, memo):
        """A copy owns its buffers and builds its own level models."""
        import copy
        held = self.__dict__.pop("_level0")
        try:
            new = type(self).__new__(type(self))
            memo[id(self)] = new
            new.__dict__ = copy.deepcopy(self.__dict__, memo)
        finally:
            self._level0 = held
        new._level0 = [None]
        return new

    # ------------------------------------------------------------------------------------- levels
    def model(self, j: int) -> SparseFrozenNetwork:
        """Level j as a ``SparseFrozenNetwork`` that shares this sweep's buffers: ``col`` / ``mean`` / ``var`` / ``kept_rows``
        are views of level j's segment, ``row_ptr`` is the level's slice minus its base (a small tensor of its own), the bias
        and flow vectors are the sweep's.  ``ensemble_eval``, ``make_graphed_eval_step`` and ``explain_ensemble`` take it
        without another freeze; nothing is read from the host."""
        import operator
        j = operator.index(j)
        if not 0 <= j < len(self.cuts):
            raise IndexError("bnn_amd: a sweep of %d thresholds has no level %d" % (len(self.cuts), j))
        if self._src[0] is None:
            raise RuntimeError("bnn_amd: this ThresholdSweep is not bound to a network; build it with evaluate.threshold_sweep(net)")
        n = self.n_layers
        fz = SparseFrozenNetwork(self.dims, self.family, self.thresholds[j], device=self.kept.device, head=self.head)
        fz.eval()
        fz._src = [self._src[0]]
        fz._layer_ids, fz._row_offsets, fz._T = list(self._layer_ids), list(self._row_offsets), list(self._T)
        fz._split = [False] * n
        shared = ("bias_mu", "bias_var") + (("q0_mean", "q0_log_var", "flow_u", "flow_w", "flow_b") if self.family == "mnf" else ())
        for i, tot in enumerate(self._tot):
            O, base, nz = self.dims[i + 1], sum(tot[:j]), tot[j]
            fz.register_buffer("kept_rows_%d" % i, self._buf("kept_rows", i)[j])
            fz.register_buffer("row_ptr_%d" % i, self._buf("row_ptr", i)[j * O:(j + 1) * O + 1] - base)
            for name in ("col", "mean", "var"):
                fz.register_buffer("%s_%d" % (name, i), self._buf(name, i)[base:base + nz])
            for name in shared:
                fz.register_buffer("%s_%d" % (name, i), self._buf(name, i))
        fz._nnz = [tot[j] for tot in self._tot]
        fz._point()
        return fz

    def _first(self) -> SparseFrozenNetwork:
        if self._level0[0] is None:
            self._level0 = [self.model(0)]
        return self._level0[0]

    def _run(self, data, S: int, stochastic: bool, log_probs: bool):
        """(K * S, B, classes) of every level under S draws (``stochastic`` False: S = 1, the posterior-mean branch)."""
        _check_log_probs(self, log_probs)
        K = len(self.cuts)
        m0 = self._first()
        x = m0._input(data)
        B, C, dev = x.shape[0], self.dims[-1], x.device
        st = ops.RngState.get(dev)
        mnf = self.family == "mnf"
        with torch.cuda.device(dev):
            if B == 0:
                if stochastic or mnf:
                    st.advance(S)
                return torch.zeros((K * S, 0, 2 if log_probs else C), dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            zbuf = m0._draw_members(S, st.t, stream)[0] if mnf else None
            layers = [tuple(self._buf(k, i) for k in ("row_ptr", "col", "mean", "var")) + t[4:]
                      for i, t in enumerate(m0._layers_of(zbuf, S))]
            head = _empty((K * S, ops.pad4(B * C)), dtype=torch.float32, device=dev)
            ops.sparse_member_chain(x, S, layers, head=self.head, out=head, empty=_empty, rng=st.t if stochastic else None,
                                    stochastic=stochastic, stream=stream, levels=K)
            if stochastic or mnf:
                st.advance(S)                                # as ONE model's call would have
        return _members_result(head, K * S, B, C, self.head, log_probs)

    @torch.no_grad()
    def ensemble(self, data: torch.Tensor, samples: int = 10, *, log_probs: bool = False) -> torch.Tensor:
        """(K, samples, B, classes): ``[j, s]`` is member s of ``model(j).ensemble(data, samples)`` from the same Philox offset,
        bit for bit; the live offset advances by ``samples``.  ``log_probs``: as ``FrozenNetwork.ensemble``."""
        S, K = int(samples), len(self.cuts)
        if S < 1:
            raise ValueError("bnn_amd: samples must be >= 1")
        if K * S > 65535:
            raise ValueError("bnn_amd: a sweep evaluates thresholds * samples members in one launch, at most 65535; got %d * %d"
                             % (K, S))
        return self._run(data, S, True, log_probs).unflatten(0, (K, S))

    @torch.no_grad()
    def forward(self, data: torch.Tensor, *, log_probs: bool = False) -> torch.Tensor:
        """(K, B, classes): ``[j]`` is ``model(j)(data, sample=False)`` from the same Philox offset, bit for bit."""
        return self._run(data, 1, False, log_probs)


def threshold_sweep(net, thresholds=(0.5, 0.9, 0.99)) -> ThresholdSweep:
    """The sparse median probability models of an LRT / planar MNF network at every one of ``thresholds`` (1 to 16 numbers in
    (0, 1), strictly ascending, no two with the same fp32 logit) from ONE pass over the parameters: see ``ThresholdSweep``.
    Refused, each naming what to use: baseline and variational-dropout networks (TypeError), dense coupling z flows and layers
    with ``noise`` / ``as_written`` (ValueError), a network on the CPU (RuntimeError)."""
    from . import layers as L
    if _is_base(net):
        raise TypeError("bnn_amd: threshold_sweep takes an LRT / MNF network; the sparse model of a baseline LBBNN network draws "
                        "explicit weights -- freeze it per threshold: freeze_base(net, \"mpm\", threshold=t, sparse=True)")
    if _is_vd(net):
        raise TypeError("bnn_amd: threshold_sweep takes an LRT / MNF network; a variational-dropout network has no gates -- use "
                        "vd_ensemble(net, data, samples)")
    if not isinstance(net, L._NetworkBase):
        raise TypeError("bnn_amd: threshold_sweep takes an lrt.BayesianNetwork or mnf.BayesianNetwork, got %s" % type(net).__name__)
    layers = net._layers()
    family = "mnf" if layers[0]._mnf else "lrt"
    sw = ThresholdSweep(net.dims, thresholds, family, device=layers[0].weight_mu.device, head=net.head)
    if any(l._mnf and l._check_flows() == "dense" for l in layers):
        raise ValueError("bnn_amd: threshold_sweep is not built for dense coupling z flows -- freeze the dense median probability "
                         "model per threshold: freeze(net, \"mpm\", threshold=t, dense=True)")
    _check_freezable_layers(layers)
    if not layers[0].weight_mu.is_cuda:
        raise RuntimeError("bnn_amd: threshold_sweep needs the network on a HIP device (it is on %s); there is no CPU path"
                           % layers[0].weight_mu.device)
    sw.eval()
    return sw._bind(net)


@torch.no_grad()
def sweep_batches(sw: ThresholdSweep, batches, samples: int = 10, posterior_mean: bool = True, accs=None) -> Dict[str, object]:
    """A whole evaluation pass of every level of a ``ThresholdSweep`` with no host read until the last batch is done: per
    ``(x, y)`` of ``batches`` ONE ``sw.ensemble``, ONE ``sw(x)`` (``posterior_mean``) and one accumulator update per level --
    ``evaluate_batches`` of every ``sw.model(j)`` from the same Philox offset, under common draws.  ``accs``: K accumulators to
    add to; default K fresh ``EvalAccumulator``s (a one-unit sigmoid head counts as two classes); a ``head="identity"`` sweep
    requires K ``RegressionAccumulator``s; any other pairing is a ValueError naming the mismatch.
    Returns ``{"thresholds", "density", "kept", "results"}`` with ``results[j]`` = ``accs[j].result()``."""
    if not isinstance(sw, ThresholdSweep):
        raise TypeError("bnn_amd: sweep_batches takes a ThresholdSweep (evaluate.threshold_sweep(net, thresholds)), got %s"
                        % type(sw).__name__)
    S, K = int(samples), len(sw.thresholds)
    reg = sw.head == "identity"
    if accs is not None:
        accs = list(accs)
        if len(accs) != K:
            raise ValueError("bnn_amd: sweep_batches: accs must hold one accumulator per threshold (%d), got %d" % (K, len(accs)))
    if reg:
        if accs is None or not all(isinstance(a, RegressionAccumulator) for a in accs):
            raise ValueError("bnn_amd: sweep_batches: this sweep has head=\"identity\" (regression): accs must be %d "
                             "evaluate.RegressionAccumulator, got %s"
                             % (K, "None" if accs is None else sorted(set(type(a).__name__ for a in accs))))
    elif accs is not None and not all(isinstance(a, EvalAccumulator) for a in accs):
        raise ValueError("bnn_amd: sweep_batches: a head=%r sweep takes EvalAccumulators, got %s (a RegressionAccumulator takes a "
                         "head=\"identity\" sweep)" % (sw.head, sorted(set(type(a).__name__ for a in accs))))
    binary = False if reg else _binary_eval(sw)
    for x, y in batches:
        outputs = sw.ensemble(x, S, log_probs=binary)
        mean = sw(x, log_probs=binary) if posterior_mean else None
        if binary and y is not None:
            y = _binary_target(y)                 # float 0 / 1 targets: converted on the device, no host read
        if accs is None:
            accs = [EvalAccumulator(outputs.shape[-1], S, outputs.device) for _ in range(K)]
        for j, acc in enumerate(accs):
            acc.update(outputs[j], y, None if mean is None else mean[j])
    if accs is None:
        raise ValueError("bnn_amd: sweep_batches got no batches and no accumulators")
    return {"thresholds": sw.thresholds, "density": sw.density, "kept": sw.kept, "results": [a.result() for a in accs]}


def freeze(net, gates: str = "alpha", *, threshold: float = 0.5, dense: bool = False, compact: bool = False,
           sparse: bool = False) -> FrozenNetwork:
    """Frozen evaluation model of an LRT / MNF network (``lrt.BayesianNetwork``, ``mnf.BayesianNetwork``) on a HIP device.

    ``gates="alpha"``: the gates as trained, a = sigmoid(lambdal) -- ``frozen.ensemble(x, S)`` computes what
    ``ensemble_forward(net, x, S)`` computes from the same Philox offset.  ``gates="mpm"``: the median probability model of
    ``outofsample(net, loader, medimod=True)``: a weight is kept (a = 1) iff ``lambdal > logit(threshold)``, compared in fp32;
    at the default threshold 0.5 that is ``alpha > 0.5``, which an fp32 ``sigmoid(lambdal) > 0.5`` matches except for
    0 < lambdal < ~6e-8 (alpha rounds to exactly 0.5 there; the frozen model keeps those weights).  The operand format is the
    network's precision at this moment ("fp32" -> fp32 operands, any 16-bit setting -> bf16 hi | lo).

    ``dense=True`` also accepts an MNF network whose z flows are dense coupling flows (RNVP / MNF type: the reference's
    default, LBBNN-GP-MF-MNF.py:46-47), with ``in_features % 4 == 0``, ``in_features`` within
    ``lbbnn_flow_dense_members_max_dim()`` (1408), at most 8 transforms, and no ``noise`` / ``as_written``; the model then also
    carries a snapshot of the coupling networks of every z flow, and every member's z is one lbbnn_flow_dense_members launch for
    all layers and members.  The keyword is opt-in because the promise above is weaker there: member m has the SAME DRAWS
    (eps_z, the Bernoulli masks, eps_out) as the m-th forward of the loop, but the member kernel sums the coupling networks'
    affine steps on the matrix cores in another order than the single forward's GEMVs, so the outputs are EQUAL TO FP32
    ROUNDING, not bit for bit.  The loop draws its masks from torch's generator when LBBNN_TORCH_MASKS=1 is set; a frozen
    model always draws them in the kernel (Philox stream LBBNN_STREAM_MASK).  A planar or LRT network with ``dense=True``
    takes the path, and gives the bits, of ``dense=False``.  Each refusal is a ValueError that names the layer; the loop form
    ``ensemble_forward(net, data, samples)`` takes every network but one whose coupling networks are not of one hidden width
    of at most ``_lib.MAX_HIDDEN`` units (``flows.dense_hidden``): no HIP kernel of this library takes those, and the loop's
    forward refuses them with the same ValueError.

    ``compact=True`` (with ``gates="mpm"``; LRT and planar MNF networks) returns a ``CompactFrozenNetwork``: the median
    probability model without the hidden units and input features no output depends on (``live_structure``), evaluated by
    the same kernels at the smaller shapes.  Its posterior-mean forward equals the full model's to fp32 rounding; its
    stochastic members equal the full model's in distribution (z is the same bits, eps_out is indexed by the compact column).
    The one device read that sizes its buffers happens here.  Refused, each with a ValueError that says what to use instead:
    ``gates="alpha"``, ``dense=True``, and a network with dense coupling z flows.

    ``sparse=True`` (with ``gates="mpm"``; LRT and planar MNF networks, every head, 1 to 16 layers) returns a
    ``SparseFrozenNetwork``: the median probability model as a CSR of its kept weights, evaluated by a vector-ALU kernel that
    touches no pruned weight and writes no per-member operand.  Its members have the draws of ``freeze(net, "mpm")`` bit for bit
    (z and eps_out at the network's own indices) and equal that model's members to fp32 rounding; it is fp32 whatever the
    precision setting, and it takes any ``in_features`` of an LRT network.  Opt-in: nothing chooses it by density.  The one
    device read that sizes its buffers happens here.  Refused, each with a ValueError that says what to use instead:
    ``gates="alpha"``, ``compact=True``, ``dense=True``, and a network with dense coupling z flows."""
    from . import layers as L
    FrozenNetwork._check_gates(gates)
    _cut(threshold)
    if _is_base(net):
        raise TypeError("bnn_amd: freeze takes an LRT / MNF network; a baseline LBBNN network has its own median probability "
                        "model: ensemble_forward(net, data, samples, gates=\"mpm\")")
    if _is_vd(net):
        raise TypeError("bnn_amd: freeze takes an LRT / MNF network; a variational-dropout network has no gates -- use "
                        "vd_ensemble(net, data, samples)")
    if not isinstance(net, L._NetworkBase):
        raise TypeError("bnn_amd: freeze takes an lrt.BayesianNetwork or mnf.BayesianNetwork, got %s" % type(net).__name__)
    layers = net._layers()
    if compact:
        if gates != "mpm":
            raise ValueError("bnn_amd: compact=True needs gates=\"mpm\": alpha gates are never exactly zero, so no unit can be "
                             "dropped -- use freeze(net, \"mpm\", compact=True), or freeze(net) for the gates as trained")
        if dense:
            raise ValueError("bnn_amd: compact=True does not take dense=True (the member kernel of the dense z flows keeps z in "
                             "LDS at full width) -- use freeze(net, \"mpm\", dense=True) for the full median probability model")
        if any(l._mnf and l._check_flows() == "dense" for l in layers):
            raise ValueError("bnn_amd: compact=True is not built for dense coupling z flows (the member kernel keeps z in LDS at "
                             "full width) -- use freeze(net, \"mpm\", dense=True) for the full median probability model")
    if sparse:
        if gates != "mpm":
            raise ValueError("bnn_amd: sparse=True needs gates=\"mpm\": alpha gates are never exactly zero, so there is no zero "
                             "to skip -- use freeze(net, \"mpm\", sparse=True), or freeze(net) for the gates as trained")
        if compact:
            raise ValueError("bnn_amd: sparse=True does not take compact=True (a dropped unit already costs a sparse model only "
                             "its epilogue) -- use freeze(net, \"mpm\", sparse=True) or freeze(net, \"mpm\", compact=True)")
        if dense:
            raise ValueError("bnn_amd: sparse=True does not take dense=True (the sparse model draws z through the planar flow "
                             "launch only) -- use freeze(net, \"mpm\", dense=True) for the dense median probability model")
        if any(l._mnf and l._check_flows() == "dense" for l in layers):
            raise ValueError("bnn_amd: sparse=True is not built for dense coupling z flows -- use freeze(net, \"mpm\", "
                             "dense=True) for the dense median probability model")
    _check_freezable_layers(layers, dense=bool(dense))
    if not layers[0].weight_mu.is_cuda:
        raise RuntimeError("bnn_amd: freeze needs the network on a HIP device (it is on %s); there is no CPU path"
                           % layers[0].weight_mu.device)
    family = "mnf" if layers[0]._mnf else "lrt"
    if compact:
        return _freeze_compact(net, layers, family, float(threshold))
    if sparse:
        return _freeze_sparse(net, layers, family, float(threshold))
    flows = layers[0]._check_flows() if family == "mnf" else None          # "planar" | "dense" (checked above)
    fz = FrozenNetwork(net.dims, family, gates, threshold, device=layers[0].weight_mu.device, flows=flows, head=net.head)
    fz.eval()
    return fz._bind(net)


# ----------------------------------------------------------------------------------------- frozen baseline model
BASE_FROZEN_GATES = ("sample", "mpm")


class FrozenBaseNetwork(_FrozenModel):
    """A trained baseline LBBNN network (``base.BayesianNetwork``) frozen for evaluation (built by ``freeze_base``; no
    parameters, buffers only): what ``test_ensemble`` and ``outofsample(net, medimod=True)`` evaluate (LBBNN-GP-MF.py:345-502).

    Per layer it holds the planes ``w_mu`` and ``w_sigma`` = softplus(weight_rho) as plain fp32 rows (``gates="mpm"``: zero
    where alpha = sigmoid(lambdal) <= threshold), ``alpha`` (``gates="sample"`` only), the posterior-mean operand ``e_w``
    (alpha * mu, or the medimean's gated mu) in the format of the precision in force at freeze time, ``b_mu``, ``b_sigma``,
    ``kept_rows`` (per row the weights with alpha > threshold) and ``alpha_rows`` (per row the sum of alpha); it records every
    layer's ``exact`` bits and Philox layer id, and the head.  One lbbnn_base_frozen_members launch per group of 4 layers then
    draws every member's weights and biases from the planes -- at the streams, offsets and counters of ``base_ensemble``, so
    a full model's members are ``base_ensemble``'s, bit for bit -- and one lbbnn_gemm_members_mean launch per layer runs
    them.  The relaxed gates' temperature is ``distributions.TEMPER_PRIOR`` at call time, as for ``base_ensemble``.

    A compact model (``freeze_base(net, "mpm", compact=True)``) holds the rows and columns of the units some output depends
    on (``live_structure``): ``dims`` are the compact widths, ``full_dims`` the network's, ``live`` / ``needed`` /
    ``active_kept`` / ``active_density`` as for ``CompactFrozenNetwork``.  Every kept weight is drawn at its FULL Philox
    counter, so member weight (o', j') and every bias are bit for bit the full model's at (live[i+1][o'], live[i][j']), and
    the outputs equal the full model's to fp32 rounding (the order of the sums).  Nothing here follows the source network's
    parameters until ``refresh()``."""

    GATES, FREEZE = BASE_FROZEN_GATES, "freeze_base"
    GATES_DOC = "'sample' (the gates drawn as trained) or 'mpm' (the median probability model)"
    _POINTER_STATE = ("_layer_descs", "_maps", "_mcap", "_mw", "_mb", "_mptr")

    def __init__(self, full_dims, gates: str = "sample", threshold: float = 0.5, device=None, head: str = "log_softmax",
                 live=None, needed=None):
        super().__init__(full_dims, gates, threshold, device, head, live, needed)
        self._exact = []
        self._layer_descs = None
        self._mcap, self._mw, self._mb, self._mptr = 0, [], [], None
        self.last_weights = self.last_biases = None

    def _device(self):
        return self._buf("w_mu", 0).device

    @property
    def density(self) -> float:
        """``gates="mpm"``: kept weights / all weights of the full network.  ``gates="sample"``: the EXPECTED density
        sum(alpha) / weights (from ``alpha_rows``) -- the mean of what the members' gates draw, not a sampled value."""
        if self.gates == "sample":
            return float(torch.stack([self._buf("alpha_rows", i).double().sum() for i in range(self.n_layers)]).sum()) / self._n_weights()
        return super().density

    def extra_repr(self) -> str:
        full = "full_dims=%s, " % (self.full_dims,) if self.compact else ""
        head = ", head=%s" % self.head if self.head != "log_softmax" else ""
        return "%sdims=%s, family=base, gates=%s, threshold=%g%s" % (full, self.dims, self.gates, self.threshold, head)

    # ------------------------------------------------------------------------------------- snapshot
    @torch.no_grad()
    def _bind(self, net, need=None, masks=None):
        """Allocate every buffer (once), build the descriptors that point at them, and take the first snapshot."""
        layers = net._layers()
        dev = layers[0].weight_mu.device
        f = dict(dtype=torch.float32, device=dev)
        n = self.n_layers
        self._src = [net]
        if masks is not None:
            self._count_kept(need, masks)
        split_now = ops.split_precision()
        for i in range(n):
            O, I = self.dims[i + 1], self.dims[i]
            ld = ops.operand_ld(I)
            # the operand format by the rule of base_ensemble, at this model's shapes
            self._split.append(bool(split_now and ops.split_eligible(I, O) and (i == 0 or self.dims[i] % 4 == 0)))
            planes = ("w_mu", "w_sigma", "e_w") + (("alpha",) if self.gates == "sample" else ())
            for name in planes:
                self.register_buffer("%s_%d" % (name, i), _empty((O, ld), **f))
            for name in ("b_mu", "b_sigma", "alpha_rows"):
                self.register_buffer("%s_%d" % (name, i), _empty((O,), **f))
        self._point()
        return self._snapshot()

    def _point(self):
        """The descriptors and maps of every layer, pointing at this model's buffers as they are now; the member buffers start
        over."""
        from . import _lib
        n = self.n_layers
        self._layer_descs = (_lib.BaseFrozenDesc * n)()
        for i in range(n):
            d = self._layer_descs[i]
            d.O, d.I = self.dims[i + 1], self.dims[i]
            d.ld = ops.operand_ld(d.I)
            d.flags = ops.F_SPLIT16 if self._split[i] else 0
            d.w_mu, d.w_sigma, d.e_w = (self._buf(k, i).data_ptr() for k in ("w_mu", "w_sigma", "e_w"))
            d.alpha = self._buf("alpha", i).data_ptr() if self.gates == "sample" else None
            d.b_mu, d.b_sigma = self._buf("b_mu", i).data_ptr(), self._buf("b_sigma", i).data_ptr()
            d.kept_rows, d.alpha_rows = self._buf("kept_rows", i).data_ptr(), self._buf("alpha_rows", i).data_ptr()
            if self._exact:
                d.exact, d.layer_id = self._exact[i], self._layer_ids[i]
        self._maps = self._compact_maps()
        self._mcap, self._mw, self._mb, self._mptr = 0, [], [], None

    def _snapshot(self):
        from . import _lib
        net = self._src[0]
        if net is None:
            raise RuntimeError("bnn_amd: this FrozenBaseNetwork is not bound to a network; build it with evaluate.freeze_base(net)")
        layers = net._layers()
        _check_base_freezable(layers)
        dev = self._device()
        if layers[0].weight_mu.device != dev or dev.type != "cuda":
            raise RuntimeError("bnn_amd: the source network (on %s) and this model (on %s) must share a HIP device; freeze it "
                               "again" % (layers[0].weight_mu.device, dev))
        self._layer_ids = [int(l._layer_id) for l in layers]
        self._exact = [int(l._exact_bits()) for l in layers]
        for i, l in enumerate(layers):
            d = self._layer_descs[i]
            _base_sources(d, l, i)
            d.exact, d.layer_id = self._exact[i], self._layer_ids[i]
        mode = ops.GATES_MPM if self.gates == "mpm" else ops.GATES_SAMPLE
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for k, cnt in _lib.layer_groups(self.n_layers):
                maps = _lib.group_slice(self._maps, k, cnt) if self._maps is not None else None
                _lib.check(_lib.lib().lbbnn_base_frozen_operands(_lib.group_slice(self._layer_descs, k, cnt), maps, cnt, mode,
                                                                 self.threshold, stream), "lbbnn_base_frozen_operands")
        return self

    @torch.no_grad()
    def refresh(self):
        """Take the snapshot again from the source network's current parameters, into the same buffers: one
        lbbnn_base_frozen_operands launch per group of 4 layers.  A compact model cannot: its shapes follow the structure."""
        if self.compact:
            raise NotImplementedError("bnn_amd: a compact model does not refresh: the structure, and with it every shape, may "
                                      "have changed with the parameters -- freeze again (evaluate.freeze_base(net, \"mpm\", "
                                      "compact=True))")
        return self._snapshot()

    # ------------------------------------------------------------------------------------- evaluation
    def _member_weights(self, c: int):
        """Member weights [c][O'][ld'] and biases [c][O'] per layer and the pointer arrays of the members call; allocated for
        the largest chunk seen, smaller chunks use a prefix."""
        from . import _lib
        if c > self._mcap:
            f = dict(dtype=torch.float32, device=self._device())
            n = self.n_layers
            self._mw = [_empty((c, self.dims[i + 1], ops.operand_ld(self.dims[i])), **f) for i in range(n)]
            self._mb = [_empty((c, self.dims[i + 1]), **f) for i in range(n)]
            self._mptr = ((_lib.c_p * n)(*[t.data_ptr() for t in self._mw]), (_lib.c_p * n)(*[t.data_ptr() for t in self._mb]))
            self._mcap = c
        return self._mw, self._mb

    def _chunk(self, x, c: int, st, head, kept):
        """Members live .. live + c - 1 into head (c, pad4(B * classes)): ceil(n / 4) lbbnn_base_frozen_members launches, then
        one GEMM launch per layer."""
        from . import _lib, distributions
        dev = x.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        mw, mb = self._member_weights(c)
        mode = ops.GATES_MPM if self.gates == "mpm" else ops.GATES_SAMPLE
        T = float(distributions.TEMPER_PRIOR)
        for k, cnt in _lib.layer_groups(self.n_layers):      # every group reads the same offset; advanced once below
            maps = _lib.group_slice(self._maps, k, cnt) if self._maps is not None else None
            rc = _lib.lib().lbbnn_base_frozen_members(_lib.group_slice(self._layer_descs, k, cnt), maps, cnt, c, mode, T,
                                                     _lib.group_slice(self._mptr[0], k, cnt), _lib.group_slice(self._mptr[1], k, cnt),
                                                     None, st.t.data_ptr(), 1, stream)
            _lib.check(rc, "lbbnn_base_frozen_members")
        if kept is not None:
            kept.append(([w[:c].clone() for w in mw], [b[:c].clone() for b in mb]))
        ops.member_gemm_chain(x, c, list(zip(mw, mb, self._split)), head=self.head, out=head, empty=_empty, stream=stream)
        st.advance(c)                                        # as c single forwards would have

    @torch.no_grad()
    def ensemble(self, data: torch.Tensor, samples: int = 10, *, max_members: Optional[int] = None, log_probs: bool = False,
                 keep_weights: bool = False) -> torch.Tensor:
        """(samples, B, classes) log-probabilities of ``samples`` members.  Member m draws at Philox offset live + m with the
        streams and counters of ``base_ensemble``: a full model returns ``base_ensemble(net, data, samples,
        gates=self.gates)["outputs"]`` from the same offset, bit for bit.  The live offset advances by ``samples``.
        ``max_members``: members per launch (default: all); chunked and unchunked results are the same bits.  The member
        buffers are kept for the largest chunk seen, and nothing here reads the device.  ``keep_weights``:
        ``self.last_weights`` / ``self.last_biases`` = per layer the (samples, O', ld') operands as the GEMMs read them (fp32
        rows with a zero tail; under a 16-bit precision the raw bf16 hi | lo rows of a layer the split kernels take) and the
        (samples, O') biases.  A model with ``head == "sigmoid"``: (samples, B, units) probabilities, or with ``log_probs``
        (one unit) the (samples, B, 2) log-probabilities of the two classes."""
        _check_log_probs(self, log_probs)
        S, chunk = _member_counts(samples, max_members)
        x = self._input(data)
        B, C, dev = x.shape[0], self.dims[-1], x.device
        st = ops.RngState.get(dev)
        self.last_weights = self.last_biases = None
        kept = [] if keep_weights else None
        with torch.cuda.device(dev):
            if B == 0:
                st.advance(S)
                return torch.zeros((S, 0, 2 if log_probs else C), dtype=torch.float32, device=dev)
            head = _empty((S, ops.pad4(B * C)), dtype=torch.float32, device=dev)
            for m0 in range(0, S, chunk):
                c = min(chunk, S - m0)
                self._chunk(x, c, st, head[m0:m0 + c], kept)
        if kept is not None:
            self.last_weights = [torch.cat(p) for p in zip(*[k[0] for k in kept])]
            self.last_biases = [torch.cat(p) for p in zip(*[k[1] for k in kept])]
        return self._finish(head, S, B, log_probs)

    @torch.no_grad()
    def forward(self, data: torch.Tensor, sample: bool = False, *, log_probs: bool = False) -> torch.Tensor:
        """(B, classes) log-probabilities.  ``sample=True``: member 0 of ``ensemble(data, 1)``.  ``sample=False``: the
        posterior-mean forward x . e_w^T + b_mu -- weight = alpha * mu (``gates="sample"``: the mode-2 branch,
        LBBNN-GP-MF.py:413) or the medimean's mu * [alpha > threshold] (``gates="mpm"``, :236-238); it draws nothing.  A
        sigmoid head: (B, units) probabilities, or with ``log_probs`` (one unit) the (B, 2) log-probabilities."""
        _check_log_probs(self, log_probs)
        if sample:
            return self.ensemble(data, 1, log_probs=log_probs)[0]
        x = self._input(data)
        B, C, dev, n = x.shape[0], self.dims[-1], x.device, self.n_layers
        if B == 0:
            return torch.zeros((0, 2 if log_probs else C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            out = _empty((1, ops.pad4(B * C)), dtype=torch.float32, device=dev)
            chain = [(self._buf("e_w", i), self._buf("b_mu", i), self._split[i]) for i in range(n)]
            ops.member_gemm_chain(x, 1, chain, head=self.head, out=out, empty=_empty,
                                  stream=torch.cuda.current_stream(dev).cuda_stream)
        return self._finish(out, 1, B, log_probs)[0]


def _base_sources(d, l, i: int):
    """The source pointers of descriptor ``d`` from baseline layer ``l`` (layer i, for the messages)."""
    for name in ("weight_mu", "weight_rho", "lambdal", "bias_mu", "bias_rho"):
        if not getattr(l, name).is_contiguous():
            raise RuntimeError("bnn_amd: %s of layer %d is not contiguous" % (name, i + 1))
    d.mu, d.rho, d.lambdal = l.weight_mu.data_ptr(), l.weight_rho.data_ptr(), l.lambdal.data_ptr()
    d.bias_mu, d.bias_rho = l.bias_mu.data_ptr(), l.bias_rho.data_ptr()


def _check_base_freezable(layers, dense: bool = True):
    """``dense`` False: a sparse model, which holds no operand rows and so has no widest row."""
    for i, l in enumerate(layers):
        if l.noise:
            raise ValueError("bnn_amd: layer %d has injected noise (layer.noise); a frozen model draws in-kernel noise only -- "
                             "clear layer.noise first" % (i + 1))
        if dense and ops.operand_ld(l.in_features) > ops.GATE_MEMBERS_MAX_LD:
            raise ValueError("bnn_amd: layer %d: in_features = %d gives operand rows wider than the member kernels take "
                             "(operand_ld(in_features) <= %d); evaluate this network with base_ensemble(net, data, samples)"
                             % (i + 1, l.in_features, ops.GATE_MEMBERS_MAX_LD))


def _base_keep_masks(layers, threshold: float):
    """Per layer the (O, I) bool mask alpha > threshold as lbbnn_base_frozen_operands compares it (a call with the keep planes
    as its only outputs): the kernel's own fp32 sigmoid and comparison, never a host-side restatement of them."""
    from . import _lib
    dev = layers[0].weight_mu.device
    n = len(layers)
    descs = (_lib.BaseFrozenDesc * n)()
    planes = []
    for i, l in enumerate(layers):
        d = descs[i]
        _base_sources(d, l, i)
        d.O, d.I = l.out_features, l.in_features
        d.ld = ops.operand_ld(d.I)
        planes.append(_empty((d.O, d.I), dtype=torch.uint8, device=dev))
        d.keep = planes[-1].data_ptr()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for k, cnt in _lib.layer_groups(n):
            _lib.check(_lib.lib().lbbnn_base_frozen_operands(_lib.group_slice(descs, k, cnt), None, cnt, ops.GATES_MPM,
                                                             threshold, stream), "lbbnn_base_frozen_operands")
    return [p.bool() for p in planes]


def freeze_base(net, gates: str = "sample", *, threshold: float = 0.5, compact: bool = False, sparse: bool = False):
    """Frozen evaluation model of a baseline LBBNN network (``base.BayesianNetwork``) on a HIP device.

    ``gates="sample"``: every member draws its gates as trained (the hard draw when ``gamma.exact`` is set, else the relaxed
    gate) -- ``frozen.ensemble(x, S)`` is ``base_ensemble(net, x, S)["outputs"]`` from the same Philox offset, bit for bit, and
    ``frozen(x)`` the posterior mean (weight = alpha * mu).  ``gates="mpm"``: the median probability model of
    ``outofsample(net, medimod=True)`` (LBBNN-GP-MF.py:450-502): a weight is kept iff sigmoid(lambdal) > threshold, compared in
    fp32 by the kernel; at the default 0.5 that is ``base_ensemble(..., gates="mpm")``, bit for bit, and ``frozen(x)`` is the
    medimean forward.  The operand format is the precision in force at this moment.

    ``compact=True`` (with ``gates="mpm"``): the model without the hidden units and input features no output depends on
    (``live_structure`` of the kernel's own keep masks); its members' weights are the full model's, bit for bit, at the rows
    and columns that stay, its outputs equal the full model's to fp32 rounding.  The one device read that sizes its buffers
    happens here.

    ``sparse=True`` (with ``gates="mpm"``): a ``SparseFrozenBaseNetwork`` -- the kept weights alone, in CSR, whose members are
    drawn on that pattern (the dense model's members, bit for bit, at the kept positions) and evaluated on the vector ALU
    without touching a pruned weight; fp32 whatever the precision setting.  It is also what ``explain_ensemble`` explains for
    this family.  The one device read (nnz per layer, to size the buffers) happens here.

    Refused, each with a ValueError / TypeError that names the cause: a network that is not a
    ``base.BayesianNetwork``, unknown ``gates``, a threshold outside (0, 1), ``compact=True`` or ``sparse=True`` with
    ``gates="sample"``, ``sparse=True`` with ``compact=True``, a layer with injected ``noise``, a layer wider than
    ``ops.GATE_MEMBERS_MAX_LD`` operand columns (dense models), a network on the CPU."""
    if not _is_base(net):
        raise TypeError("bnn_amd: freeze_base takes a baseline LBBNN network (bnn_amd.base.BayesianNetwork), got %s; an LRT / "
                        "MNF network has evaluate.freeze" % type(net).__name__)
    FrozenBaseNetwork._check_gates(gates)
    threshold = float(threshold)
    _cut(threshold)
    if compact and gates != "mpm":
        raise ValueError("bnn_amd: compact=True needs gates=\"mpm\": sampled gates are never fixed at zero, so no unit can be "
                         "dropped -- use freeze_base(net, \"mpm\", compact=True), or freeze_base(net) for the gates as trained")
    if sparse and gates != "mpm":
        raise ValueError("bnn_amd: sparse=True needs gates=\"mpm\": sampled gates are never fixed at zero, so every weight "
                         "stays -- use freeze_base(net, \"mpm\", sparse=True), or freeze_base(net) for the gates as trained")
    if sparse and compact:
        raise ValueError("bnn_amd: sparse=True with compact=True is not built: the sparse model already touches no pruned "
                         "weight (pruning it further to the active paths is out of scope) -- use freeze_base(net, \"mpm\", "
                         "sparse=True) or freeze_base(net, \"mpm\", compact=True)")
    layers = net._layers()
    _check_base_freezable(layers, dense=not sparse)
    dev = layers[0].weight_mu.device
    if not layers[0].weight_mu.is_cuda:
        raise ValueError("bnn_amd: freeze_base needs the network on a HIP device (it is on %s); there is no CPU path" % dev)
    if sparse:
        fz = SparseFrozenBaseNetwork(net.dims, threshold, device=dev, head=net.head)
        fz.eval()
        return fz._bind(net)
    live = needed = need = masks = None
    if compact:
        masks = _base_keep_masks(layers, threshold)
        need, live, needed = _live_structure(masks, 8)       # the ONE device read: the live counts size every buffer
    fz = FrozenBaseNetwork(net.dims, gates, threshold, device=dev, head=net.head, live=live, needed=needed)
    fz.eval()
    return fz._bind(net, need, masks)



def _transposed_input(x, stream):
    """x^T [I0][sparse_row_pad(B)], what the first layer of every explicit-weight member reads: one launch."""
    from . import _lib
    B, I = x.shape
    ldb = ops.sparse_row_pad(B)
    xT = _empty((I, ldb), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().lbbnn_transpose_operand(ops._ptr_rows(x, "x"), B, I, x.stride(0), xT.data_ptr(), ldb, 0, 0, stream),
               "lbbnn_transpose_operand")
    return xT


def _stored_forward(fz, xT, B: int, wb, out, stream, hidden=None):
    """The forward of explicit-weight members of a sparse model on their stored values ``wb`` (per layer (w, b, ...), rows =
    members), from ``_transposed_input``: one lbbnn_sparse_gather_members FORWARD launch per layer -- hidden layers transposed
    [member][unit][sparse_row_pad(B)] with ReLU (appended to ``hidden`` where the caller keeps them), the last written
    row-major into ``out`` (members, B * classes)."""
    from . import _lib
    n, dims, ldb, c = fz.n_layers, fz.dims, xT.shape[1], out.shape[0]
    a, a_ms = xT, 0
    for i in range(n):
        O, last = dims[i + 1], i == n - 1
        o = out if last else _empty((c, O * ldb), dtype=torch.float32, device=xT.device)
        ops.sparse_gather_members(_lib.GATHER_FORWARD, fz._buf("row_ptr", i), fz._buf("col", i), None, wb[i][0], a, o,
                                  B=B, K=dims[i], N=O, lda=ldb, a_mstride=a_ms, ldo=O if last else ldb,
                                  o_mstride=out.stride(0) if last else O * ldb, blocks=c, bias=wb[i][1], relu=not last,
                                  out_rows=last, stream=stream)
        if hidden is not None and not last:
            hidden.append(o)
        a, a_ms = o, O * ldb                                 # (a keeps the buffer alive until the launch that reads it is queued)


class SparseFrozenBaseNetwork(_SparseModel, _FrozenModel):
    """The median probability model of a baseline LBBNN network as its kept weights alone (``freeze_base(net, "mpm",
    sparse=True)``): per layer a CSR of the weights with sigmoid(lambdal) > threshold (the comparison of the dense frozen
    model, made by the kernel in fp32) -- buffers ``row_ptr_<i>`` (O + 1) int32, ``col_<i>`` (nnz) int32 ascending within a row,
    ``mean_<i>`` (nnz) = weight_mu, ``sigma_<i>`` (nnz) = softplus(weight_rho) -- plus the dense ``b_mu``, ``b_sigma`` and
    ``kept_rows``.  It holds no dense plane and no dense member operand: the members' weights are (members, nnz) values, and a
    layer is ONE lbbnn_sparse_gather_members launch for all members, on the vector ALU, over the kept weights only.  The model
    is fp32 whatever the precision setting.  ``csr(i)``: the four tensors of layer i; ``nnz`` / ``operand_bytes``: plain ints.

    Draws: member m draws at Philox offset live + m, every kept weight at its counter in the FULL network -- the weights and
    biases of ``freeze_base(net, "mpm", threshold=t)``'s member m at the kept positions, bit for bit (the pruned ones are that
    model's zeros), so a member equals the dense model's to fp32 rounding (the sums run over the kept weights in column order,
    sequentially).  The bits of an output depend on its member, row and unit alone.  The baseline member is an explicit-weight
    member, so ``evaluate.explain_ensemble`` explains exactly the members ``ensemble`` evaluates; its first call adds the buffers
    ``col_ptr_<i>`` (I + 1), ``trow_<i>``, ``tslot_<i>``, ``tpos_<i>`` (nnz): the pattern column by column.  No ``refresh()``:
    freeze again."""

    GATES, FREEZE, VALUES = ("mpm",), "freeze_base", ("mean", "sigma")
    GATES_DOC = "'mpm' (a sparse model is the median probability model)"
    _POINTER_STATE = ("_draw_descs",)

    def __init__(self, dims, threshold: float = 0.5, device=None, head: str = "log_softmax"):
        super().__init__(dims, "mpm", threshold, device, head)
        self.family = "base"
        self._nnz = []
        self._draw_descs = None
        self.last_weights = self.last_biases = None

    def extra_repr(self) -> str:
        head = ", head=%s" % self.head if self.head != "log_softmax" else ""
        return "dims=%s, family=base, gates=mpm, threshold=%g%s, sparse, nnz=%d" % (self.dims, self.threshold, head, self.nnz)

    @torch.no_grad()
    def _bind(self, net):
        from . import _lib
        layers = net._layers()
        f = dict(dtype=torch.float32, device=layers[0].weight_mu.device)
        n = self.n_layers
        self._src = [net]
        self._layer_ids = [int(l._layer_id) for l in layers]
        self._split = [False] * n
        descs = (_lib.BaseSparseDesc * n)()
        for i, l in enumerate(layers):
            O = self.dims[i + 1]
            d = descs[i]
            _base_sources(d, l, i)
            for name in ("b_mu", "b_sigma"):
                self.register_buffer("%s_%d" % (name, i), _empty((O,), **f))
            d.b_mu, d.b_sigma = self._buf("b_mu", i).data_ptr(), self._buf("b_sigma", i).data_ptr()
            d.kept_rows = self._buf("kept_rows", i).data_ptr()
            d.O, d.I = O, self.dims[i]
        self._nnz = [t[0] for t in _pack_csr(self, descs, "lbbnn_base_sparse_count", "lbbnn_base_sparse_pack", (self.threshold,),
                                             "sigma")]
        self._point()
        return self

    def _point(self):
        """The draw descriptors of every layer, pointing at this model's buffers as they are now (a call fills in its own
        member buffers)."""
        from . import _lib
        n = self.n_layers
        self._draw_descs = (_lib.BaseSparseDrawDesc * n)()
        for i in range(n):
            d = self._draw_descs[i]
            d.row_ptr, d.col, d.mean, d.sigma = (t.data_ptr() for t in self.csr(i))
            d.b_mu, d.b_sigma = self._buf("b_mu", i).data_ptr(), self._buf("b_sigma", i).data_ptr()
            d.O, d.I, d.nnz, d.layer_id = self.dims[i + 1], self.dims[i], self._nnz[i], self._layer_ids[i]

    # ------------------------------------------------------------------------------------- evaluation
    def _draw(self, c: int, rng, stream, tpos=None, weight_noise: bool = True):
        """Members live .. live + c - 1: per layer (w (c, pad4(nnz)), b (c, pad4(O)), wt) from ceil(n / 4)
        lbbnn_base_sparse_draw_members launches; ``tpos`` (per layer the place of every slot in the column-by-column order):
        wt holds the values once more in that order (None without).  Every group reads the same offset; the caller advances it."""
        from . import _lib
        n, descs, out = self.n_layers, self._draw_descs, []
        f = dict(dtype=torch.float32, device=self._device())
        for i in range(n):
            ldw, ldo = ops.pad4(self._nnz[i]), ops.pad4(self.dims[i + 1])
            w, b = _empty((c, ldw), **f), _empty((c, ldo), **f)
            wt = None if tpos is None else _empty((c, ldw), **f)
            d = descs[i]
            d.w, d.w_mstride, d.b, d.b_mstride = w.data_ptr(), ldw, b.data_ptr(), ldo
            d.tpos, d.wt = (None, None) if tpos is None else (tpos[i].data_ptr(), wt.data_ptr())
            out.append((w, b, wt))
        for k, cnt in _lib.layer_groups(n):
            rc = _lib.lib().lbbnn_base_sparse_draw_members(_lib.group_slice(descs, k, cnt), cnt, c,
                                                           rng.data_ptr() if weight_noise else None, 1,
                                                           0 if weight_noise else ops.F_MEAN_ONLY, stream)
            _lib.check(rc, "lbbnn_base_sparse_draw_members")
        return out

    def _head(self, buf, S: int, B: int, log_probs: bool):
        """The (S, B, C) result from the (S, B * C) logits: at most one launch, whatever S."""
        C = self.dims[-1]
        if self.head == "sigmoid":
            return _binary_members(buf, S, B, C, log_probs)
        out = buf.view(S, B, C)
        if self.head == "identity":
            return out
        if C <= 64:
            rows = buf.view(S * B, C)
            ops.log_softmax_rows(rows, out=rows)             # in place: one thread per row
            return out
        return torch.log_softmax(out, dim=-1)

    @torch.no_grad()
    def ensemble(self, data: torch.Tensor, samples: int = 10, *, max_members: Optional[int] = None, log_probs: bool = False,
                 keep_weights: bool = False) -> torch.Tensor:
        """(samples, B, classes) log-probabilities of ``samples`` members, as ``FrozenBaseNetwork.ensemble``.  Member m draws at
        Philox offset live + m; the live offset advances by ``samples``.  Per chunk of ``max_members`` members (default: all):
        one draw launch per group of 4 layers and one layer launch per layer, after ONE input transpose per call; then the head,
        at most one launch.  Chunked and unchunked results are the same bits, and nothing here reads the device.
        ``keep_weights``: ``self.last_weights`` / ``self.last_biases`` = per layer the (samples, nnz) values in CSR order and the
        (samples, O) biases."""
        _check_log_probs(self, log_probs)
        S, chunk = _member_counts(samples, max_members)
        x = self._input(data)
        B, C, dev = x.shape[0], self.dims[-1], x.device
        st = ops.RngState.get(dev)
        self.last_weights = self.last_biases = None
        kept = [] if keep_weights else None
        with torch.cuda.device(dev):
            if B == 0:
                st.advance(S)
                return torch.zeros((S, 0, 2 if log_probs else C), dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            xT = _transposed_input(x, stream)
            buf = _empty((S, B * C), dtype=torch.float32, device=dev)
            for m0 in range(0, S, chunk):
                c = min(chunk, S - m0)
                wb = self._draw(c, st.t, stream)
                if kept is not None:
                    kept.append(wb)
                _stored_forward(self, xT, B, wb, buf[m0:m0 + c], stream)
                st.advance(c)                                # as c single forwards would have
            if kept is not None:
                self.last_weights = [torch.cat([k[i][0] for k in kept])[:, :nz] for i, nz in enumerate(self._nnz)]
                self.last_biases = [torch.cat([k[i][1] for k in kept])[:, :self.dims[i + 1]] for i in range(self.n_layers)]
            return self._head(buf, S, B, log_probs)

    @torch.no_grad()
    def forward(self, data: torch.Tensor, sample: bool = False, *, log_probs: bool = False) -> torch.Tensor:
        """(B, classes) of one member.  ``sample=True``: member 0 of ``ensemble(data, 1)``.  ``sample=False``: the medimean
        forward (LBBNN-GP-MF.py:236-238) -- the layer launches on ``mean_<i>`` / ``b_mu_<i>`` as a one-member value vector; no
        draw launch, nothing is drawn and the live offset stays."""
        _check_log_probs(self, log_probs)
        if sample:
            return self.ensemble(data, 1, log_probs=log_probs)[0]
        x = self._input(data)
        B, C, dev = x.shape[0], self.dims[-1], x.device
        if B == 0:
            return torch.zeros((0, 2 if log_probs else C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            buf = _empty((1, B * C), dtype=torch.float32, device=dev)
            wb = [(self._buf("mean", i).view(1, -1), self._buf("b_mu", i).view(1, -1)) for i in range(self.n_layers)]
            _stored_forward(self, _transposed_input(x, stream), B, wb, buf, stream)
            return self._head(buf, 1, B, log_probs)[0]


# ----------------------------------------------------------------------------------------- local explanations
def _check_explainable(fz):
    """``explain`` takes a FrozenNetwork of family LRT or planar MNF; everything else is refused with what to use instead."""
    from . import layers as L
    if isinstance(fz, SparseFrozenBaseNetwork):
        raise ValueError("bnn_amd: explain is not built for sparse=True models (its sweep multiplies by dense operands, which a "
                         "sparse model does not hold); the point explanation of this model, its medimean network: "
                         "evaluate.explain_ensemble(fz, data, samples=1, weight_noise=False)")
    if isinstance(fz, FrozenBaseNetwork) or _is_base(fz):
        raise TypeError("bnn_amd: explain is not built for the baseline family (its frozen model draws its weights per member); "
                        "explain an LRT / MNF network: evaluate.explain(evaluate.freeze(net, \"mpm\"), data)")
    if _is_vd(fz):
        raise TypeError("bnn_amd: explain takes a frozen LRT / MNF model; a variational-dropout network has no gates and no frozen "
                        "model -- train an lrt.BayesianNetwork and use evaluate.explain(evaluate.freeze(net, \"mpm\"), data)")
    if isinstance(fz, L._NetworkBase):
        raise TypeError("bnn_amd: explain takes a frozen model, not the network itself: evaluate.explain(evaluate.freeze(net, "
                        "\"mpm\"), data) (or gates=\"alpha\" for the gates as trained)")
    if not isinstance(fz, FrozenNetwork):
        raise TypeError("bnn_amd: explain takes a FrozenNetwork (evaluate.freeze(net, \"alpha\" | \"mpm\")), got %s"
                        % type(fz).__name__)
    if isinstance(fz, SparseFrozenNetwork):
        raise ValueError("bnn_amd: explain is not built for sparse=True models (its sweep multiplies by dense operands, which a "
                         "sparse model does not hold); explain the dense median probability model: "
                         "evaluate.explain(evaluate.freeze(net, \"mpm\"), data)")
    if fz.flows == "dense":
        raise ValueError("bnn_amd: explain is not built for dense=True models (RNVP / MNF-type z flows); use planar z flows "
                         "(mnf.BayesianNetwork(..., z_flow_type=\"Planar\")) or an LRT network")


def _check_explain_rows(B: int, Cp: int):
    from . import _lib
    if B * Cp > _lib.EXPLAIN_MAX_ROWS:
        raise ValueError("bnn_amd: explain takes at most 2**24 rows of (batch x explained outputs) per call, got %d x %d; split "
                         "the batch" % (B, Cp))


def _explain_step(a, what, stream):
    import ctypes
    from . import _lib
    _lib.check(_lib.lib().lbbnn_explain_step(ctypes.byref(a), stream), "lbbnn_explain_step (%s)" % what)


@torch.no_grad()
def explain(fz, data: torch.Tensor, *, targets=None, keep_masks: bool = False, acc=None) -> Dict[str, object]:
    """Which inputs drove which output of the frozen posterior-mean forward ``fz(data, sample=False)``, row by row.  That
    forward is a ReLU chain on fixed operands, so its pre-head output is exactly ``logits[b, c] = sum_i J[b, c, i] x[b, i] +
    k[b, c]`` with ``J(b) = W_L D_{L-1}(b) .. D_1(b) W_1``; this computes the terms of that sum on the device.

    ``fz``: a ``FrozenNetwork`` (LRT or planar MNF, gates "alpha" or "mpm", full or compact, any head, 1 to 16 layers).
    ``targets``: None -- every output (C' = C, needs C <= 16); a (B,) int64 device tensor -- one output per row (C' = 1; a value
    outside [0, C) raises IndexError, found by one host read); ``"pred"`` -- the row's largest logit, taken on the device.
    Returns device tensors: ``logits`` (B, C), the last layer before the head; ``contributions`` (B, C', full_dims[0]) =
    J * x at the network's own feature index (a compact model's dropped features are exactly 0.0); ``intercept`` (B, C'), the
    bias path b_L + sum_l <G_l D_l, b_l>, computed on its own; ``residual`` (B, C') = logits - (sum_i contributions +
    intercept), the caller's self-check; ``active`` (B, L - 1) int32, hidden units with h_l > 0; ``targets`` (None, or the (B,)
    tensor in force); with ``keep_masks`` ``masks``, per hidden layer a (B, O_l) bool tensor of h_l > 0 (a compact model: its
    own units); an MNF model: ``z``, per layer the (in_features,) z this call drew.
    An MNF model draws one z per layer at the live Philox offset and advances it by 1, as ``fz(data)`` does; an LRT model
    draws nothing.  The masks are h_l > 0 of the very forward that produced ``logits``.  The sweep is fp32 whatever the model's
    precision: its operands are the values the forward's products multiplied by (``FrozenNetwork._explain_operands``).
    ``acc``: an ``ExplanationAccumulator`` that takes this batch in the same call."""
    import ctypes
    from . import _lib
    _check_explainable(fz)
    if not isinstance(data, torch.Tensor):
        raise TypeError("bnn_amd: explain takes a device tensor of input rows, got %s" % type(data).__name__)
    if not data.is_cuda:
        raise ValueError("bnn_amd: explain runs on the HIP device (data is on %s); there is no CPU path -- move it with "
                         "data.to(device)" % data.device)
    if fz._src[0] is None:
        raise ValueError("bnn_amd: this FrozenNetwork is not bound to a network; build it with evaluate.freeze(net)")
    n, C, F = fz.n_layers, fz.dims[-1], fz.full_dims[0]
    x = fz._input(data)
    B, dev = x.shape[0], x.device
    pred = isinstance(targets, str)
    if pred and targets != "pred":
        raise ValueError("bnn_amd: targets must be None, \"pred\" or a (B,) int64 device tensor, got %r" % (targets,))
    if targets is None:
        if C > _lib.EXPLAIN_MAX_OUTPUTS:
            raise ValueError("bnn_amd: explaining every output takes at most %d outputs, this model has %d; pass targets= (one "
                             "output per row, e.g. targets=\"pred\")" % (_lib.EXPLAIN_MAX_OUTPUTS, C))
        Cp = C
    else:
        Cp = 1
        if not pred:
            if not isinstance(targets, torch.Tensor) or targets.dtype != torch.int64 or tuple(targets.shape) != (B,):
                raise ValueError("bnn_amd: targets must be a (%d,) int64 tensor (one output per row)" % B)
            if targets.device != dev:
                raise ValueError("bnn_amd: targets is on %s, the model on %s; move it with targets.to(device)" % (targets.device, dev))
            targets = targets.contiguous()
            if B and bool(((targets < 0) | (targets >= C)).any()):
                raise IndexError("bnn_amd: a target lies outside [0, %d)" % C)
    _check_explain_rows(B, Cp)
    f = dict(dtype=torch.float32, device=dev)
    st = ops.RngState.get(dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        zs = None
        if fz.family == "mnf":
            zbuf, ewm = fz._draw_members(1, st.t, stream)
            e_ws = [e[0] for e in ewm]
            zs = [z[0] for z in fz._z_of(zbuf, 1)]
        else:
            e_ws = [fz._buf("e_w", i) for i in range(n)]
        if B == 0:
            if zs is not None:
                st.advance(1)
            res = dict(logits=torch.zeros((0, C), **f), contributions=torch.zeros((0, Cp, F), **f),
                       intercept=torch.zeros((0, Cp), **f), residual=torch.zeros((0, Cp), **f),
                       active=torch.zeros((0, n - 1), dtype=torch.int32, device=dev),
                       targets=torch.zeros(0, dtype=torch.int64, device=dev) if targets is not None else None)
            if keep_masks:
                res["masks"] = [torch.zeros((0, fz.dims[i + 1]), dtype=torch.bool, device=dev) for i in range(n - 1)]
            if zs is not None:
                res["z"] = zs
            if acc is not None:
                acc.update(res)
            return res
        logits, hs = fz._chain_keep(x, st, e_ws)
        if zs is not None:
            st.advance(1)
        if pred:
            targets = torch.argmax(logits, dim=1)
        rows, wts = fz._explain_operands(e_ws, stream)
        R = B * Cp
        intercept, residual = _empty((B, Cp), **f), _empty((B, Cp), **f)
        active = _empty((B, n - 1), dtype=torch.int32, device=dev)
        masks = [_empty((B, fz.dims[i + 1]), dtype=torch.bool, device=dev) for i in range(n - 1)] if keep_masks else None
        scatter = fz.compact and not fz._input_identity
        contributions = torch.zeros((B, Cp, F), **f) if scatter else _empty((B, Cp, F), **f)
        a = _lib.ExplainStepArgs()
        a.B, a.C, a.w_rows = B, Cp, C
        a.targets = targets.data_ptr() if targets is not None else None
        a.intercept = intercept.data_ptr()
        g = None
        for l in range(n - 2, -1, -1):                       # hidden layer l: h_l = hs[l], width dims[l + 1]
            width = fz.dims[l + 1]
            h = hs[l]
            if g is None:                                    # seed: the last layer's rows, no product
                g = _empty((R, ops.pad4(width)), **f)
                a.mode, a.w, a.ldw, a.bias_out = _lib.EXPLAIN_SEED, rows[n - 1].data_ptr(), rows[n - 1].stride(0), \
                    fz._buf("bias_mu", n - 1).data_ptr()
            else:                                            # G_l = (G_{l+1} W_{l+1}) D_l
                g = ops.lrt_gemm(g[:, :fz.dims[l + 2]], wts[l + 1], None, I=fz.dims[l + 2], O=width, mean_only=True,
                                 out=_empty((R, ops.pad4(width)), **f)[:, :width])
                a.mode, a.w, a.bias_out = _lib.EXPLAIN_MASK, None, None
            a.width, a.g, a.ldg = width, g.data_ptr(), g.stride(0)
            a.h, a.ldh, a.bias = h.data_ptr(), h.stride(0), fz._buf("bias_mu", l).data_ptr()
            a.active, a.ld_active = active.data_ptr() + 4 * l, n - 1
            a.mask_out, a.ldm = (masks[l].data_ptr(), masks[l].stride(0)) if keep_masks else (None, 0)
            _explain_step(a, "seed" if a.mode == _lib.EXPLAIN_SEED else "mask", stream)
        width = fz.dims[0]
        if g is not None:
            g = ops.lrt_gemm(g[:, :fz.dims[1]], wts[0], None, I=fz.dims[1], O=width, mean_only=True,
                             out=_empty((R, ops.pad4(width)), **f)[:, :width])
            a.g, a.ldg, a.w, a.bias_out = g.data_ptr(), g.stride(0), None, None
        else:                                                # one layer: J is the rows of W_1, the intercept its bias
            a.g, a.ldg = None, 0
            a.w, a.ldw, a.bias_out = rows[0].data_ptr(), rows[0].stride(0), fz._buf("bias_mu", 0).data_ptr()
        a.mode, a.width = _lib.EXPLAIN_FINISH, width
        a.h, a.ldh, a.bias = x.data_ptr(), x.stride(0) if B > 1 else max(x.stride(0), width), None
        a.active, a.mask_out = None, None
        a.logits, a.ldl = logits.data_ptr(), logits.stride(0) if B > 1 else C
        a.map, a.full_width = (fz._buf("live", 0).data_ptr() if scatter else None), F
        a.contributions, a.ldc, a.residual = contributions.data_ptr(), F, residual.data_ptr()
        _explain_step(a, "finish", stream)
        res = dict(logits=logits, contributions=contributions, intercept=intercept, residual=residual, active=active,
                   targets=targets)
        if keep_masks:
            res["masks"] = masks
        if zs is not None:
            res["z"] = zs
        if acc is not None:
            acc.update(res)
    return res


def _explanation_means(rows, total, abs_total):
    """(mean_contribution, mean_abs_contribution) of an ExplanationAccumulator from its totals: each output's sums over its
    rows; NaN for an output no row was counted for."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int64)
    den = np.where(rows > 0, rows, 1).astype(np.float64)[:, None]
    nan = np.where(rows > 0, 0.0, np.nan)[:, None]
    return np.asarray(total, dtype=np.float64) / den + nan, np.asarray(abs_total, dtype=np.float64) / den + nan


class ExplanationAccumulator(_DeviceTotals):
    """Running totals of ``explain`` over an evaluation pass, kept on the device: per output the number of explained rows and
    the fp64 sums of the contributions and of their absolute values per input feature.  ``update`` adds a batch with no host
    read (lbbnn_explain_totals: per-workgroup fp64 partials, then a fixed-order add -- the same bits on every run, no float
    atomics); ``result`` is the one read.  With ``targets`` (one output per row) a row is counted under its target.
    ``outputs`` <= 16 and ``features`` (the network's ``full_dims[0]``) are fixed for the accumulator's life."""

    def __init__(self, outputs: int, features: int, device):
        from . import _lib
        C, F = int(outputs), int(features)
        if not 1 <= C <= _lib.EXPLAIN_MAX_OUTPUTS:
            raise ValueError("bnn_amd: ExplanationAccumulator takes 1 to %d outputs, got %d" % (_lib.EXPLAIN_MAX_OUTPUTS, C))
        if F < 1:
            raise ValueError("bnn_amd: ExplanationAccumulator takes at least one feature, got %d" % F)
        self.outputs, self.features = C, F
        # one buffer, one read: rows | the sums (bit patterns of doubles) | the sums of absolute values
        self._start(C + 2 * C * F, device)

    def update(self, result: Dict[str, object]):
        """Add the batch an ``explain`` call returned."""
        from . import _lib
        contributions, targets = result["contributions"], result.get("targets")
        B, Cp, F = contributions.shape
        C = self.outputs
        if F != self.features or (targets is None and Cp != C) or (targets is not None and Cp != 1):
            raise ValueError("bnn_amd: this ExplanationAccumulator was built for %d outputs and %d features, the result has "
                             "%d explained outputs per row and %d features" % (C, self.features, Cp, F))
        if result["logits"].shape[1] != C:
            raise ValueError("bnn_amd: this ExplanationAccumulator was built for %d outputs, the model has %d"
                             % (C, result["logits"].shape[1]))
        dev = contributions.device
        if not contributions.is_cuda or dev != self._totals.device:
            raise ValueError("bnn_amd: the result is on %s, the accumulator on %s" % (dev, self._totals.device))
        self.updates += 1
        if B == 0:
            return self
        work, base = self._work_ptr(_lib.lib().lbbnn_explain_work_bytes(B, C, F)), self._totals.data_ptr()
        _launch(dev, "lbbnn_explain_totals", contributions.data_ptr(), F, targets.data_ptr() if targets is not None else None,
                B, C, F, base + 8 * C, base + 8 * (C + C * F), base, work)
        return self

    def result(self) -> Dict[str, object]:
        """``rows`` (outputs,) int64: explained rows per output; ``mean_contribution`` and ``mean_abs_contribution`` (outputs,
        features) float64: the sums over those rows divided by ``rows`` (NaN for an output without rows) --
        ``mean_abs_contribution`` is the global importance that sits beside ``structure_posterior``'s ``feature_prob``; and the
        raw ``sum_contribution`` / ``sum_abs_contribution``."""
        import numpy as np
        h = self._host()
        C, F = self.outputs, self.features
        rows = h[:C].copy()
        total = h[C:C + C * F].view(np.float64).reshape(C, F).copy()
        abs_total = h[C + C * F:].view(np.float64).reshape(C, F).copy()
        mean, mean_abs = _explanation_means(rows, total, abs_total)
        return dict(rows=rows, mean_contribution=mean, mean_abs_contribution=mean_abs, sum_contribution=total,
                    sum_abs_contribution=abs_total)


@torch.no_grad()
def explain_batches(fz, batches, acc: Optional[ExplanationAccumulator] = None, targets: str = "all") -> ExplanationAccumulator:
    """A whole pass of ``explain`` with no host read: every batch of ``batches`` (a device tensor, or a tuple whose first entry
    is one) goes through ``explain(fz, x, acc=acc)``; ``targets="all"`` explains every output, ``"pred"`` each row's predicted
    output (the totals are then indexed by the predicted class).  Returns the accumulator (default: a fresh one); its
    ``result()`` is the one read."""
    if targets not in ("all", "pred"):
        raise ValueError("bnn_amd: explain_batches takes targets=\"all\" or \"pred\", got %r" % (targets,))
    _check_explainable(fz)
    if acc is None:
        acc = ExplanationAccumulator(fz.dims[-1], fz.full_dims[0], fz._device())
    for batch in batches:
        x = batch[0] if isinstance(batch, (tuple, list)) else batch
        explain(fz, x, targets=None if targets == "all" else "pred", acc=acc)
    return acc


# ----------------------------------------------------------------------------------------- explanations of sampled-weight members
def _check_ensemble_explainable(fz):
    """``explain_ensemble`` takes a SparseFrozenNetwork or a SparseFrozenBaseNetwork; everything else is refused with what to
    use instead."""
    from . import layers as L
    if isinstance(fz, (SparseFrozenNetwork, SparseFrozenBaseNetwork)):
        return
    if isinstance(fz, FrozenNetwork):
        raise TypeError("bnn_amd: explain_ensemble explains sampled-weight members of the sparse median probability model (it "
                        "keeps every member's weights, which only the kept weights of a sparse model make small); build it with "
                        "evaluate.freeze(net, \"mpm\", sparse=True).  For a point explanation of this dense model: "
                        "evaluate.explain(fz, data)")
    if isinstance(fz, FrozenBaseNetwork) or _is_base(fz):
        raise TypeError("bnn_amd: explain_ensemble explains the members of the SPARSE median probability model of a baseline "
                        "network, got %s; build it with evaluate.freeze_base(net, \"mpm\", sparse=True): "
                        "evaluate.explain_ensemble(evaluate.freeze_base(net, \"mpm\", sparse=True), data)" % type(fz).__name__)
    if _is_vd(fz):
        raise TypeError("bnn_amd: explain_ensemble is built for LRT, planar MNF and baseline networks: "
                        "evaluate.explain_ensemble(evaluate.freeze(net, \"mpm\", sparse=True), data) of an lrt / mnf "
                        "BayesianNetwork, got %s" % type(fz).__name__)
    if isinstance(fz, L._NetworkBase):
        raise TypeError("bnn_amd: explain_ensemble takes a sparse frozen model, not the network itself: "
                        "evaluate.explain_ensemble(evaluate.freeze(net, \"mpm\", sparse=True), data)")
    raise TypeError("bnn_amd: explain_ensemble takes a SparseFrozenNetwork (evaluate.freeze(net, \"mpm\", sparse=True)), got %s"
                    % type(fz).__name__)


def _transposed_pattern(fz, i: int):
    """(col_ptr, trow, tslot, tpos) of layer i of a sparse model, built at the first use and kept as buffers ``col_ptr_<i>``
    (I + 1), ``trow_<i>``, ``tslot_<i>`` (nnz): ops.sparse_transposed_pattern, and ``tpos_<i>`` (nnz), the inverse of tslot (the
    place of CSR slot k in the column-by-column order); no host read."""
    if not hasattr(fz, "col_ptr_%d" % i):
        row_ptr, col, _, _ = fz.csr(i)
        pat = ops.sparse_transposed_pattern(row_ptr, col, fz.dims[i])
        tpos = torch.empty_like(pat[2])
        tpos[pat[2].long()] = torch.arange(pat[2].numel(), dtype=torch.int32, device=tpos.device)
        for name, t in zip(("col_ptr", "trow", "tslot", "tpos"), pat + (tpos,)):
            fz.register_buffer("%s_%d" % (name, i), t)
    return tuple(fz._buf(k, i) for k in ("col_ptr", "trow", "tslot", "tpos"))


def explain_ensemble_work_bytes(dims, B: int, samples: int, outputs: int) -> int:
    """Bytes of the work buffers of one ``explain_ensemble`` call: per member the kept hidden activations, per (member,
    explained output) two G buffers of the widest hidden layer and the transposed contributions, each line
    ops.sparse_row_pad(B) floats."""
    hidden = list(dims[1:-1])
    per_member = sum(hidden) + outputs * (2 * max(hidden, default=0) + dims[0])
    return 4 * ops.sparse_row_pad(B) * int(samples) * per_member


@torch.no_grad()
def explain_ensemble(fz, data: torch.Tensor, samples: int = 10, *, targets=None, weight_noise: bool = True,
                     keep_members: bool = False, keep_weights: bool = False, levels=None,
                     max_bytes: int = 2 << 30, keep_masks: bool = False) -> Dict[str, object]:
    """Which inputs drove which output, row by row, WITH the posterior's uncertainty: the explanation of ``samples``
    sampled-weight members of the sparse median probability model ``fz`` (``freeze(net, "mpm", sparse=True)``; LRT or planar
    MNF, any head, 1 to 16 layers), and its mean, spread and sign probability over the members.

    A member draws explicit weights on the kept pattern: per CSR slot ``w = mean * z[col] + sqrt(var) * eps`` (an LRT layer has
    no z factor), per unit ``b = bias_mu + sqrt(bias_var) * eps``.  It is then an ordinary ReLU network, so its pre-head output
    is exactly ``logits_m[b, c] = sum_i J_m[b, c, i] x[b, i] + k_m[b, c]``; the member of ``fz.ensemble`` draws per activation
    (local reparameterisation, the row-wise marginal of this draw), is not linear in x and has no such sum.  Member m draws at
    Philox offset live + m: z of an MNF layer from the flow launch of ``fz.ensemble`` (the same z, bit for bit), eps of the
    weights from stream STREAM_EPS_W * 64 + layer id (slot k: counter (k / 4, 0), word k % 4), of the biases from STREAM_EPS_B *
    64 + layer id (unit o: counter (o / 4, 0), word o % 4).  The live offset advances by ``samples`` (not at all when nothing is
    drawn: an LRT model with ``weight_noise=False``).  ``weight_noise=False``: eps = 0, every member is the mean network under
    its own z; an LRT model then has one member (``samples`` must be 1): the sparse counterpart of
    ``explain(freeze(net, "mpm"), data)``.

    ``targets`` as for ``explain``: None -- every output (C' = C <= 16); a (B,) int64 device tensor -- one output per row
    (C' = 1; a value outside [0, C) raises IndexError, found by one host read); ``"pred"`` -- the largest member-mean logit of
    the row, taken on the device.  Returns device tensors: ``mean``, ``std`` (B, C', F) over the members of J_m(b) * x (fp64 sum
    in member order; the unbiased deviation, 0.0 for one member); ``prob_positive``, ``prob_negative`` (B, C', F), the share of
    members with a contribution > 0 / < 0; ``logits`` (S, B, C); ``intercept`` (S, B, C') = b_L + sum_l <G_l D_l, b_l>, summed on
    its own; ``residual`` (S, B, C') = logits - (sum_i contributions + intercept) in fp64 from the fp32 terms, the caller's
    self-check; ``targets``; an MNF model: ``z``, per layer (S, in_features) (views of one buffer); ``keep_members``: ``members`` (S, B, C', F);
    ``keep_weights``: ``weights`` / ``biases``, per layer (S, nnz) / (S, O); ``levels=(0.9, ...)``: ``lower`` / ``upper``, per
    level the (B, C', F) bounds of the central interval, ``torch.quantile`` over ``members`` (which are then kept);
    ``keep_masks`` (as for ``explain``): ``masks``, per hidden layer the (S, B, O_l) bool pattern h_l > 0 of the members' own
    forward.  A feature without a kept path to the output contributes exactly 0.0 in every member.

    A baseline model (``freeze_base(net, "mpm", sparse=True)``, a ``SparseFrozenBaseNetwork``): its member is an explicit-weight
    member already -- per CSR slot ``w = mean + sigma * eps`` with eps at the weight's counter in the FULL network, per unit ``b =
    b_mu + b_sigma * eps`` (lbbnn_base_sparse_draw_members) -- so from the same Philox offset the members explained are the
    members ``fz.ensemble`` evaluates: ``weights`` / ``biases`` are its ``last_weights`` / ``last_biases`` and, with an identity
    head, ``logits`` its result, bit for bit.  There is no z.  ``weight_noise=False`` (``samples`` must be 1) is the medimean
    network: the family's point explanation.

    The statistics are over one chunk of members.  Refused before any launch: a model that is not a sparse frozen model, CPU
    data, ``samples`` < 1 or ``samples * C'`` > 65535, work buffers (``explain_ensemble_work_bytes``) above ``max_bytes``."""
    import ctypes
    from . import _lib
    _check_ensemble_explainable(fz)
    if not isinstance(data, torch.Tensor):
        raise TypeError("bnn_amd: explain_ensemble takes a device tensor of input rows, got %s" % type(data).__name__)
    if not data.is_cuda:
        raise ValueError("bnn_amd: explain_ensemble runs on the HIP device (data is on %s); there is no CPU path -- move it with "
                         "data.to(device)" % data.device)
    S = int(samples)
    if S < 1:
        raise ValueError("bnn_amd: explain_ensemble takes samples >= 1, got %r" % (samples,))
    base = isinstance(fz, SparseFrozenBaseNetwork)
    mnf = fz.family == "mnf"
    if not weight_noise and not mnf and S != 1:
        raise ValueError("bnn_amd: %s model with weight_noise=False has ONE member (the mean network), got samples=%d; pass "
                         "samples=1, or weight_noise=True for members that differ" % ("a baseline" if base else "an LRT", S))
    if levels is not None:
        levels = tuple(float(v) for v in levels)
        if not levels or any(not 0.0 < v < 1.0 for v in levels):
            raise ValueError("bnn_amd: levels must be coverages inside (0, 1), e.g. levels=(0.9,), got %r" % (levels,))
        keep_members = True
    n, dims = fz.n_layers, tuple(fz.dims)
    C, F = dims[-1], dims[0]
    x = fz._input(data)
    B, dev = x.shape[0], x.device
    pred = isinstance(targets, str)
    if pred and targets != "pred":
        raise ValueError("bnn_amd: targets must be None, \"pred\" or a (B,) int64 device tensor, got %r" % (targets,))
    if targets is None:
        if C > _lib.EXPLAIN_MAX_OUTPUTS:
            raise ValueError("bnn_amd: explaining every output takes at most %d outputs, this model has %d; pass targets= (one "
                             "output per row, e.g. targets=\"pred\")" % (_lib.EXPLAIN_MAX_OUTPUTS, C))
        Cp = C
    else:
        Cp = 1
        if not pred:
            if not isinstance(targets, torch.Tensor) or targets.dtype != torch.int64 or tuple(targets.shape) != (B,):
                raise ValueError("bnn_amd: targets must be a (%d,) int64 tensor (one output per row)" % B)
            if targets.device != dev:
                raise ValueError("bnn_amd: targets is on %s, the model on %s; move it with targets.to(device)" % (targets.device, dev))
    if S * Cp > _lib.MEMBER_BLOCKS_MAX:
        raise ValueError("bnn_amd: explain_ensemble takes at most %d (members x explained outputs) per call, got %d x %d; lower "
                         "samples or pass targets=" % (_lib.MEMBER_BLOCKS_MAX, S, Cp))
    work = explain_ensemble_work_bytes(dims, B, S, Cp)
    if work > max_bytes:
        raise ValueError("bnn_amd: explain_ensemble needs %d bytes of work buffers for %d rows x %d members x %d explained "
                         "outputs, max_bytes is %d; split the batch or lower samples" % (work, B, S, Cp, max_bytes))
    if targets is not None and not pred:
        targets = targets.contiguous()
        if B and bool(((targets < 0) | (targets >= C)).any()):
            raise IndexError("bnn_amd: a target lies outside [0, %d)" % C)
    f = dict(dtype=torch.float32, device=dev)
    st = ops.RngState.get(dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        pats = [_transposed_pattern(fz, i) for i in range(n)]
        csrs = [fz.csr(i) for i in range(n)]
        zbuf = None
        if mnf:
            fz._draw_members(S, st.t, stream)
            zbuf = fz._take_z(S)                              # the members' z go out with the result
        zs = [] if mnf else None
        layers, off = [], 0
        for i in range(n):
            z = None if zbuf is None else zbuf[:, off:off + dims[i]]
            off += ops.operand_ld(dims[i])
            if mnf:
                zs.append(z)
            if base:
                continue
            _, col, mean, var = csrs[i]
            layers.append((col, mean, var, fz._buf("bias_mu", i), fz._buf("bias_var", i), z, fz._layer_ids[i], dims[i],
                           pats[i][3]))
        if base:
            # the baseline member IS an explicit-weight member: the draw of fz.ensemble, with the column-by-column copy
            wb = fz._draw(S, st.t, stream, tpos=[p[3] for p in pats], weight_noise=weight_noise)
        else:
            wb = ops.sparse_draw_members(layers, S, st.t, weight_noise=weight_noise, empty=_empty, stream=stream)
        # the live offset moves on in the seed launch, behind the launches that drew (with no rows: a launch of its own)
        advance = S if (mnf or weight_noise) else 0
        if advance and B == 0:
            st.advance(S)
        res = dict(targets=targets)
        if zs is not None:
            res["z"] = zs
        if keep_weights:
            res["weights"] = [t[0][:, :csrs[i][1].numel()] for i, t in enumerate(wb)]
            res["biases"] = [t[1][:, :dims[i + 1]] for i, t in enumerate(wb)]
        if B == 0:
            res.update(logits=torch.zeros((S, 0, C), **f), intercept=torch.zeros((S, 0, Cp), **f),
                       residual=torch.zeros((S, 0, Cp), **f))
            for k in ("mean", "std", "prob_positive", "prob_negative"):
                res[k] = torch.zeros((0, Cp, F), **f)
            if pred:
                res["targets"] = torch.zeros(0, dtype=torch.int64, device=dev)
            if keep_members:
                res["members"] = torch.zeros((S, 0, Cp, F), **f)
            if keep_masks:
                res["masks"] = [torch.zeros((S, 0, dims[l + 1]), dtype=torch.bool, device=dev) for l in range(n - 1)]
            if levels is not None:
                res["lower"] = [torch.zeros((0, Cp, F), **f) for _ in levels]
                res["upper"] = [torch.zeros((0, Cp, F), **f) for _ in levels]
            return res
        # the members' forward: every hidden layer kept, transposed [member][unit][ldb]
        ldb = ops.sparse_row_pad(B)
        xT, hs = _transposed_input(x, stream), []
        logits = _empty((S, B, C), **f)
        _stored_forward(fz, xT, B, wb, logits.view(S, B * C), stream, hidden=hs)
        if keep_masks:
            res["masks"] = [(h.view(S, dims[l + 1], ldb)[:, :, :B] > 0).transpose(1, 2).contiguous() for l, h in enumerate(hs)]
        # where the sweep starts, one launch: the explained output ("pred": the largest member-mean logit), the one-hot seed
        # G_L [c'][c][b] the members share, and the intercept's first term b_L
        if pred:
            targets = res["targets"] = _empty((B,), dtype=torch.int64, device=dev)
        R = S * Cp
        seed, intercept = _empty((Cp, C, ldb), **f), _empty((S, B, Cp), **f)
        _lib.check(_lib.lib().lbbnn_explain_seed(logits.data_ptr(), None if pred or targets is None else targets.data_ptr(),
                                                 int(pred), targets.data_ptr() if pred else None, wb[n - 1][1].data_ptr(),
                                                 wb[n - 1][1].stride(0), seed.data_ptr(), ldb, intercept.data_ptr(), S, B, C, Cp,
                                                 st.t.data_ptr() if advance else None, advance, stream), "lbbnn_explain_seed")
        # the sweep: the member layer on the transposed pattern, G_l = D_l W_{l+1}^T G_{l+1}, then J * x = (W_1^T G_1) * x^T; a
        # launch whose input is a hidden layer's G also adds that layer's bias path <G, b> to the intercept
        wmax = max(dims[1:-1], default=0)
        gbufs = [_empty((R, wmax * ldb), **f) for _ in range(min(2, n - 1))]
        g, g_ms, shared = seed, C * ldb, True
        for l in range(n - 1, 0, -1):                        # hidden layer l: hs[l - 1], width dims[l]; the pattern of layer l + 1
            width = dims[l]
            col_ptr, trow = pats[l][:2]
            o = gbufs[(n - 1 - l) % 2]
            ops.sparse_gather_members(_lib.GATHER_SWEEP, col_ptr, trow, None, wb[l][2], g, o, B=B, K=dims[l + 1], N=width,
                                      lda=ldb, a_mstride=g_ms, ldo=ldb, o_mstride=width * ldb, blocks=R, per_member=Cp,
                                      h=hs[l - 1], ldh=ldb, h_mstride=width * ldb, a_shared=shared,
                                      dot_bias=None if shared else wb[l][1], dot_acc=None if shared else intercept, stream=stream)
            g, g_ms, shared = o, width * ldb, False
        col_ptr, trow = pats[0][:2]
        contrib = _empty((R, F * ldb), **f)
        ops.sparse_gather_members(_lib.GATHER_FINISH, col_ptr, trow, None, wb[0][2], g, contrib, B=B, K=dims[1], N=F, lda=ldb,
                                  a_mstride=g_ms, ldo=ldb, o_mstride=F * ldb, blocks=R, per_member=Cp, h=xT, ldh=ldb,
                                  a_shared=shared, dot_bias=None if shared else wb[0][1], dot_acc=None if shared else intercept,
                                  stream=stream)
        # the statistics over the members, row-major
        out = dict((k, _empty((B, Cp, F), **f)) for k in ("mean", "std", "prob_positive", "prob_negative"))
        members = _empty((S, B, Cp, F), **f) if keep_members else None
        residual = _empty((S, B, Cp), **f)
        sa = _lib.MemberStatsArgs(contrib.data_ptr(), F * ldb, ldb, S, Cp, F, B, out["mean"].data_ptr(), out["std"].data_ptr(),
                                  out["prob_positive"].data_ptr(), out["prob_negative"].data_ptr(),
                                  members.data_ptr() if keep_members else None, logits.data_ptr(), C, C,
                                  targets.data_ptr() if targets is not None else None, intercept.data_ptr(), residual.data_ptr())
        _lib.check(_lib.lib().lbbnn_explain_member_stats(ctypes.byref(sa), stream), "lbbnn_explain_member_stats")
        res.update(out, logits=logits, intercept=intercept, residual=residual)
        if keep_members:
            res["members"] = members
        if levels is not None:
            res["lower"] = [torch.quantile(members, (1.0 - v) / 2.0, dim=0) for v in levels]
            res["upper"] = [torch.quantile(members, (1.0 + v) / 2.0, dim=0) for v in levels]
    return res
