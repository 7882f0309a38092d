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
"""
from typing import Dict, Optional

import torch

from . import ops


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
def ensemble_forward_batched(net, data: torch.Tensor, samples: int = 10) -> torch.Tensor:
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
    keep, e_all, z_all = [], [], []
    for i, l in enumerate(layers):
        cfg = (True, False, i < n - 1)
        # (the member dimension of the batched ensemble exists in the bf16 hi | lo format: any 16-bit precision selects it)
        l._split_now = int(bool(l._split(x if i == 0 else None)) and (i == 0 or layers[i - 1].out_features % 4 == 0))
        keep.append(l._fill_desc(descs[i], cfg, None))
        ld = ops.operand_ld(l.in_features)
        e = torch.empty((S, l.out_features, ld), **f)
        e_all.append(e)
        descs[i].e_w = e.data_ptr()
        if l._mnf:
            z = torch.empty((S, ld), **f)
            z_all.append(z)
            descs[i].z_fwd = z.data_ptr()
        descs[i].eps_z = None
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib().lbbnn_ensemble_operands(descs, n, S, rng.data_ptr(), 1, stream), "lbbnn_ensemble_operands")
    h, h_ms = x, 0                                             # the first layer reads the same rows for every member
    for i, l in enumerate(layers):
        O, I = l.out_features, l.in_features
        ws = l._workspace()
        o_ms = -(-(B * O) // 4) * 4                           # member stride padded to 16 B (vector loads / stores per member)
        out = torch.empty((S, o_ms), **f)[:, :B * O].view(S, B, O) if o_ms != B * O else torch.empty((S, B, O), **f)
        last = i == n - 1
        flags = (0 if last else ops.F_RELU) | (ops.F_SPLIT16 if l._split_now else 0) | \
                (ops.F_LOG_SOFTMAX if (last and O <= 16) else 0)
        rc = _lib.lib().lbbnn_lrt_gemm_members(
            h.data_ptr(), h.stride(-2), h_ms, e_all[i].data_ptr(), O * ops.operand_ld(I), ws.var_w.data_ptr(),
            ops.operand_ld(I), l.bias_mu.data_ptr(), ws.bias_var.data_ptr(), rng.data_ptr(),
            ops.STREAM_EPS_OUT * 64 + l._layer_id, l.row_offset, 1, out.data_ptr(), O, o_ms, B, I, O, flags, S, stream)
        _lib.check(rc, "lbbnn_lrt_gemm_members")
        h, h_ms = out, o_ms
    st.advance(S)                                              # as S single forwards would have
    if layers[-1].out_features > 16:
        h = torch.log_softmax(h, dim=-1)
    for l in layers:
        l.kl = 0
    net._kl_total = None
    del keep
    return h


def _is_vd(net) -> bool:
    from . import vd
    return isinstance(net, vd.BNN)


def _vd_check(net, data, samples, max_members):
    if not _is_vd(net):
        raise ValueError("bnn_amd: vd_ensemble takes a variational-dropout network (bnn_amd.vd.BNN)")
    S = int(samples)
    if S < 1:
        raise ValueError("bnn_amd: samples must be >= 1")
    chunk = S if max_members is None else int(max_members)
    if chunk < 1:
        raise ValueError("bnn_amd: max_members must be >= 1")
    return S, chunk


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
    pad = lambda n: -(-n // 4) * 4                             # member strides padded to 16 B
    head = torch.empty((S, pad(B * C)), **f)
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
            out = outputs[m0:m0 + c] if last else torch.empty((c, pad(B * l.m)), **f)[:, :B * l.m].view(c, B, l.m)
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
                  keep_gates: bool = False) -> Dict[str, object]:
    """``samples`` evaluation forwards of a baseline LBBNN network in 1 + 3 launches per chunk of at most ``max_members``
    members (default: all in one).  Member m draws at Philox offset (live offset + m) and equals, bit for bit, what
    ``net.sample_predict`` / the layers' ``sample_forward`` compute at that offset; chunked and unchunked results are the same
    bits.  The live offset advances by ``samples``.  Returns ``outputs`` (samples, B, classes) log-probabilities,
    ``gate_rows`` (per layer (samples, O): the sum over each row of the gates the member used) and, with ``keep_gates``,
    ``gates`` (per layer (samples, O, I)).  A network with a layer wider than lbbnn_gate_members takes
    (``ops.operand_ld(in_features) > ops.GATE_MEMBERS_MAX_LD``) runs each member as its ``sample_forward`` chain instead
    (``BayesianNetwork._predict_members_loop``; ``gates="mpm"`` raises there)."""
    if not _is_base(net):
        raise ValueError("bnn_amd: base_ensemble takes a baseline LBBNN network (bnn_amd.base.BayesianNetwork)")
    if not data.is_cuda:
        raise RuntimeError("bnn_amd: ensemble evaluation needs a HIP device tensor (data is on %s); there is no CPU path"
                           % data.device)
    S = int(samples)
    if S < 1:
        raise ValueError("bnn_amd: samples must be >= 1")
    chunk = S if max_members is None else int(max_members)
    if chunk < 1:
        raise ValueError("bnn_amd: max_members must be >= 1")
    net.eval()
    B, C = data.reshape(-1, net.dims[0]).shape[0], net.dims[-1]
    st = ops.RngState.get(data.device)
    head = torch.empty((S, -(-(B * C) // 4) * 4), dtype=torch.float32, device=data.device)   # 16-B aligned member rows
    rows, kept, outs = [], [], []
    for m0 in range(0, S, chunk):
        c = min(chunk, S - m0)
        o, r, g = net._predict_members(data, st.t, c, gates, out=head[m0:m0 + c], rows=True, keep_gates=keep_gates)
        st.advance(c)
        outs.append(o)
        rows.append(r)
        kept.append(g)
    if C <= 16:
        outputs = head[:, :B * C].view(S, B, C)             # the chunks wrote their log-probabilities into `head`
    else:
        outputs = outs[0] if len(outs) == 1 else torch.cat(outs)
    cat = lambda parts: [p[0] if len(parts) == 1 else torch.cat(p) for p in zip(*parts)]
    return {"outputs": outputs, "gate_rows": cat(rows), "gates": cat(kept) if keep_gates else None}


@torch.no_grad()
def ensemble_forward(net, data: torch.Tensor, samples: int = 10, batched=None, *, gates: str = "sample",
                     max_members: Optional[int] = None) -> torch.Tensor:
    """(samples, B, classes) log-probabilities of ``samples`` stochastic forwards (net left in eval mode).
    ``batched``: None = the one-launch-per-kernel form when the network qualifies (``_batched_ok``; a baseline network on a
    HIP device: ``base_ensemble``), else the loop of fused single forwards (``net.sample_predict`` for a baseline network);
    True / False force one of them.  Either form advances the live Philox offset by ``samples``.
    ``gates`` ("sample" or "mpm") applies to baseline networks only, ``max_members`` (members per launch of the batched form)
    to baseline and variational-dropout networks.  A variational-dropout network (``vd.BNN``): None = ``vd_ensemble`` on a
    HIP device when no layer has injected noise, else the loop of ``net(data)``; True with injected noise raises ValueError."""
    net.eval()
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
            return base_ensemble(net, data, samples, gates=gates, max_members=max_members)["outputs"]
        return torch.stack([net.sample_predict(data, gates=gates) for _ in range(samples)])
    if gates != "sample":
        raise ValueError("bnn_amd: gates=%r (the median probability model) exists for baseline LBBNN networks only" % (gates,))
    if max_members is not None:
        raise ValueError("bnn_amd: max_members applies to baseline LBBNN networks only")
    if batched is None:
        batched = _batched_ok(net, data)
    if batched:
        return ensemble_forward_batched(net, data, samples)
    outs = [net(data, sample=True) for _ in range(samples)]
    return torch.stack(outs)


@torch.no_grad()
def ensemble_eval(net, data: torch.Tensor, target: Optional[torch.Tensor] = None, samples: int = 10) -> Dict[str, object]:
    """test_ensemble's numbers for one batch: ``outputs``, ``pred_ensemble``, ``pred_posterior_mean``, ``density`` (and
    ``correct_*`` with a target).  Variational-dropout networks: ``outputs``, ``pred_ensemble``, and ``loss`` and
    ``correct_ensemble`` with a target (``_vd_ensemble_eval``).  Baseline networks: ``density[s]`` is the mean gate of member s over all weights -- the gates
    the member actually used (the reference draws a separate set, LBBNN-GP-MF.py:390-394) -- and the posterior mean is the
    mode-2 forward (weight = alpha * mu) with alpha = sigmoid(lambdal) set as the reference sets it (:369-374, :413)."""
    if _is_base(net):
        return _base_ensemble_eval(net, data, target, samples)
    if _is_vd(net):
        return _vd_ensemble_eval(net, data, target, samples)
    outputs = ensemble_forward(net, data, samples)
    density = []
    for _ in range(samples):
        g = [l.gamma.rsample().flatten() for l in (net.l1, net.l2, net.l3)]
        density.append(torch.cat(g).mean())
    pred_ens = outputs.mean(0).argmax(1)
    pred_mean = net(data, sample=False).argmax(1)
    res = {"outputs": outputs, "pred_ensemble": pred_ens, "pred_posterior_mean": pred_mean,
           "density": torch.stack(density)}
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


def _base_ensemble_eval(net, data, target, samples):
    r = base_ensemble(net, data, samples)
    outputs = r["outputs"]
    layers = (net.l1, net.l2, net.l3)
    n_w = sum(l.out_features * l.in_features for l in layers)
    density = torch.stack([rw.double().sum(1) for rw in r["gate_rows"]]).sum(0) / n_w
    for l in layers:
        l.alpha = 1 / (1 + torch.exp(-l.lambdal.detach()))                  # :369-374
        l.gamma.alpha = l.alpha
    pred_mean = net(data, None, None, None, sample=False).argmax(1)          # :413 (mode 2: weight = alpha * mu)
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
    if outputs.dim() != 3:
        raise ValueError("bnn_amd: outputs must be (samples, B, classes), got %s" % (tuple(outputs.shape),))
    p = torch.sigmoid(outputs.float())
    p = p / p.sum(-1, keepdim=True)
    m = p.mean(0)
    return -(m * torch.log(m)).sum(-1)
