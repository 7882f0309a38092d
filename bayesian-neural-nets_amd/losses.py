"""The scalar head of a training step as fused HIP launches (include/lbbnn.h: lbbnn_elbo_loss*, lbbnn_elbo_bce_loss*).

``elbo_loss(log_probs, target, kl, num_batches)`` is ``F.nll_loss(log_probs, target, reduction='sum') + kl / num_batches`` --
what the reference's ``train()`` writes out (LBBNN-GP-MF-MNF.py:268-271; ...LRT.py:222-225) -- as ONE forward launch and ONE
backward launch instead of torch's nll_loss / mul / add kernels (13 + 4 + 4 us forward, 6 us + fills backward for a
4096 x 10 batch: the reduce kernel of nll_loss runs on a single workgroup).  The reference's own spelling keeps working; this
is the faster one for callers that want it (``bnn_amd.parallel.DataParallelELBO.loss`` uses it on HIP tensors).

``TrainMonitor`` is training's counterpart of ``evaluate.EvalAccumulator``: ``elbo_loss(..., monitor=mon)`` keeps the running
totals of a training log (loss, nll, accuracy, bad labels, non-finite steps) on the device, in the loss launch itself, and
leaves a per-step "loss is not finite" word there that ``optim.Adam`` / ``optim.SGD`` honour after ``set_guard(mon)``.

``elbo_bce_loss`` (a ``head="sigmoid"`` network) and ``elbo_gaussian_loss`` (a ``head="identity"`` network: regression with a
normal likelihood, lbbnn_elbo_gaussian_loss*) are the same step for the other two heads, with the same monitor.
"""
import torch
import torch.nn.functional as F

import os as _os

from . import _lib

_FUSE_LSM_BWD = _os.environ.get("LBBNN_FUSE_LSM_BWD", "1") != "0"     # A/B knob


class _Handover:
    """Hand-over from a loss's backward to the backward of the head that produced the loss's input.  When the log-probabilities
    came out of a layer's fused log_softmax, or the probabilities out of ``layers._SigmoidHeadFn``, the loss backward forms the
    gradient with respect to the LOGITS in its own launch (lbbnn_elbo_loss_backward_logits, lbbnn_elbo_bce_loss_backward) and
    leaves it here; the head's backward takes it instead of launching lbbnn_log_softmax_backward / lbbnn_sigmoid_backward.

    ``leave(out, g_out, g_logits)``: ``g_logits`` is for the node that produced ``out``, valid only against ``g_out``, the
    gradient the loss returns for ``out``.  ``take(out, g)``: ``g_logits`` if ``g``, the gradient that node received, is that
    very tensor, else None (something stood between the head and the loss: the caller runs its own backward kernel).

    Why the addresses are enough: the entry HOLDS ``out`` and ``g_out``.  While it exists their storage cannot be freed and
    handed to another tensor, so "same address" means "same tensor" (an address alone could be a reused block).  Entries live
    for one backward pass: ``take`` removes the entry whether it matches or not, and the forward of the next fused loss
    clears what no head asked for."""

    def __init__(self):
        self._held = {}

    def __len__(self):
        return len(self._held)

    def clear(self):
        self._held.clear()

    def leave(self, out, g_out, g_logits):
        self._held[out.data_ptr()] = (g_out.data_ptr(), g_logits, out, g_out)

    def take(self, out, g):
        ent = self._held.pop(out.data_ptr(), None)
        return ent[1] if ent is not None and ent[0] == g.data_ptr() else None


_HEAD_GRAD = _Handover()
HANDOVER = {"taken": 0, "sigmoid_backward": 0}     # which way each sigmoid head's backward went


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch_loss(dev, name, head, monitor):
    """The forward launch of a loss: ``name(*head)``, or with a monitor ``name``_monitor with the same head arguments plus the
    monitor's two pointers."""
    if monitor is None:
        _lib.launch(dev, name, *head)
    else:
        _lib.launch(dev, name + "_monitor", *head, monitor._totals.data_ptr(), monitor._guard.data_ptr())


class TrainMonitor:
    """Running totals of a training pass, kept on the device: ``elbo_loss(..., monitor=mon)`` adds a step to them inside its one
    forward launch (lbbnn_elbo_loss_monitor; no host read, capturable as it is), ``result()`` reads them -- the ONLY
    synchronisation, once per epoch in a training loop.  What the reference's ``train()`` prints per batch (LBBNN-GP-MF-MNF.py:
    263-275: ``loss`` and ``nll``) are ``last_loss`` and ``last_nll``; the epoch means and the training accuracy come with them.

    The monitor also holds the guard word: 1 after a step whose loss is not finite, 0 after any other (per step, not sticky).
    ``optimizer.set_guard(mon)`` makes ``bnn_amd.optim.Adam`` / ``SGD`` skip the update of such a step on the device -- no
    parameter, moment or step counter changes -- and count it in ``skipped_steps``; with ``max_grad_norm`` set, a step whose
    gradient norm is NaN or infinite is skipped and counted too (``max_grad_norm=float("inf")``: a pure check, nothing is clipped).

    ``classes`` (1 to 64) is fixed for the monitor's life.  Under ``graphs.make_graphed_train_step`` the factory's eager warm-up
    steps are real steps and add to the totals: ``reset()`` after building the step.  The monitor is a plain holder of two
    buffers (``to`` / ``_apply`` move them, ``copy.deepcopy`` gives a copy its own) and caches no device address; a captured
    graph addresses the buffers it was captured with.  Not a data-parallel guard: the loss flag is local to a rank.

    The binary loss records into the same monitor: ``elbo_bce_loss(..., monitor=mon)`` with ``TrainMonitor(units, device)``
    (lbbnn_elbo_bce_loss_monitor).  Its unit of account is one element (b, o) of the (B, units) block, so ``rows`` grows by
    B * units a step; ``base.BayesianNetwork.sample_elbo(monitor=)`` and ``vd.loss_fn(monitor=)`` pass a monitor on to the loss
    of their family."""

    def __init__(self, classes: int, device):
        C = int(classes)
        if not 1 <= C <= 64:
            raise ValueError("bnn_amd: TrainMonitor takes 1 to 64 classes, got %d" % C)
        self.classes = C
        # one buffer, one read: the counts | the doubles (bit patterns); the guard word has its own (int32)
        self._totals = torch.zeros(_lib.MONITOR_WORDS, dtype=torch.int64, device=torch.device(device))
        self._guard = torch.zeros(1, dtype=torch.int32, device=self._totals.device)

    @property
    def device(self):
        return self._totals.device

    def _apply(self, fn):
        self._totals, self._guard = fn(self._totals), fn(self._guard)
        return self

    def to(self, device):
        return self._apply(lambda t: t.to(device))

    def reset(self):
        """Zero the totals and the guard word (either loss; after building a graphed step, whose warm-up steps count)."""
        self._totals.zero_()
        self._guard.zero_()

    def _skipped_ptr(self):
        return self._totals.data_ptr() + 8 * _lib.MONITOR_SKIPPED_STEPS

    def _read(self):
        """The totals as a host int64 array (the one device-to-host copy)."""
        return self._totals.cpu().numpy()

    def result(self, strict: bool = True):
        """Python numbers.  Counts: ``steps``, ``rows``, ``correct`` (the arg-max of a row with a valid target equals it;
        numpy.argmax's rule), ``bad_targets`` (outside [0, classes)), ``nonfinite_rows`` (rows with an inf or NaN
        log-probability), ``nonfinite_steps`` (steps whose loss is inf or NaN), ``skipped_steps`` (optimizer steps a guard
        skipped), ``nll_rows`` (rows with a valid target of the finite steps).  Sums over the FINITE steps, in fp64: ``nll_sum``,
        ``kl_term_sum`` (kl / num_batches), ``loss_sum``; of the last step, finite or not: ``last_nll``, ``last_loss``.  Derived:
        ``nll_mean`` = nll_sum / nll_rows, ``loss_mean`` = loss_sum / finite steps, ``accuracy`` = correct / rows with a valid
        target -- NaN where the denominator is 0.  ``strict``: targets outside [0, classes) raise IndexError, as ``F.nll_loss``
        would have; with ``strict=False`` they are reported in ``bad_targets``.

        After ``elbo_bce_loss(monitor=)`` the same keys count ELEMENTS: ``rows`` B * units per step, ``correct`` elements with a
        valid target and (p > 0.5) == (y > 0.5), ``bad_targets`` targets outside [0, 1] or NaN (the IndexError of ``strict`` names
        ``[0, classes)``; it means these), ``nonfinite_rows`` probabilities that are inf or NaN (such an element costs the loss
        100, it does not make it non-finite), ``nll_rows`` elements with a valid target of the finite steps; ``nll_mean`` is the
        mean BCE per element and ``accuracy`` the fraction of elements on the right side of 0.5.

        After ``elbo_gaussian_loss(monitor=)`` they count ELEMENTS too: ``correct`` elements with a valid target and
        |y - mean| <= exp(0.5 log_var), so ``accuracy`` reads as the ONE-SIGMA COVERAGE (about 0.683 for a calibrated Gaussian),
        ``bad_targets`` targets that are NaN or infinite, ``nonfinite_rows`` elements whose mean or log-variance is inf or NaN
        (such an element does make the loss non-finite), ``nll_mean`` the mean Gaussian negative log-likelihood per element."""
        import numpy as np
        h = np.ascontiguousarray(self._read(), dtype=np.int64)
        n = _lib.MONITOR_COUNTS
        res = {k: int(h[i]) for i, k in enumerate(_lib.MONITOR_COUNT_NAMES)}
        if strict and res["bad_targets"]:
            raise IndexError("bnn_amd: %d target(s) outside [0, %d) in this training pass" % (res["bad_targets"], self.classes))
        sums = h[n:n + _lib.MONITOR_SUMS].view(np.float64)
        for i, k in enumerate(_lib.MONITOR_SUM_NAMES):
            res[k] = float(sums[i])
        div = lambda x, d: x / d if d else float("nan")
        res["nll_mean"] = div(res["nll_sum"], res["nll_rows"])
        res["loss_mean"] = div(res["loss_sum"], res["steps"] - res["nonfinite_steps"])
        res["accuracy"] = div(res["correct"], res["rows"] - res["bad_targets"])
        return res


class _ElboLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, target, kl, scale, monitor):
        B, C = log_probs.shape
        _HEAD_GRAD.clear()                         # entries live for one backward pass only
        lp = log_probs if log_probs.stride(1) == 1 else log_probs.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=lp.device)
        head = (lp.data_ptr(), lp.stride(0), target.data_ptr(), B, C, _ptr(kl), float(scale), loss.data_ptr())
        _launch_loss(lp.device, "lbbnn_elbo_loss", head, monitor)
        ctx.save_for_backward(target, lp)
        ctx.meta = (B, C, float(scale), kl is not None)
        return loss

    @staticmethod
    def backward(ctx, g):
        target, lp = ctx.saved_tensors
        B, C, scale, has_kl = ctx.meta
        g = g.contiguous()
        g_logp = torch.empty((B, C), dtype=torch.float32, device=g.device)
        g_kl = torch.empty((), dtype=torch.float32, device=g.device) if has_kl else None
        if _FUSE_LSM_BWD and C <= 64:
            g_logits = torch.empty((B, C), dtype=torch.float32, device=g.device)
            _lib.launch(g.device, "lbbnn_elbo_loss_backward_logits", g.data_ptr(), target.data_ptr(), lp.data_ptr(), lp.stride(0),
                        B, C, scale, g_logp.data_ptr(), g_logits.data_ptr(), _ptr(g_kl))
            _HEAD_GRAD.leave(lp, g_logp, g_logits)
        else:
            _lib.launch(g.device, "lbbnn_elbo_loss_backward", g.data_ptr(), target.data_ptr(), B, C, scale, g_logp.data_ptr(),
                        _ptr(g_kl))
        return g_logp, None, g_kl, None, None


def _fused_kl(kl) -> bool:
    return kl is None or (torch.is_tensor(kl) and kl.is_cuda and kl.dtype == torch.float32 and kl.numel() == 1)


_BAD_KL = "kl must be None or a one-element float32 HIP tensor"


def _check_monitored(loss, noun, units, x, kl, monitor, target=None):
    """A monitor rides in the fused forward launch: ValueError naming what keeps this call of ``loss`` off that path.  ``x`` is
    the loss's (B, ``units``) input, called ``noun``.  The order of the refusals is each loss's own and stays: with class-id
    targets (``elbo_loss``) the device comes before the target and ``kl``, the element-wise losses refuse ``kl`` before the
    device."""
    def refuse(msg):
        raise ValueError("bnn_amd: %s(monitor=...): %s" % (loss, msg))

    if not isinstance(monitor, TrainMonitor):
        refuse("monitor must be a bnn_amd.TrainMonitor, got %s" % type(monitor).__name__)
    if x.dtype != torch.float32 or x.dim() != 2:
        refuse("%s must be float32 (B, %s), got %s %s" % (noun, units, x.dtype, tuple(x.shape)))
    if x.shape[1] != monitor.classes:
        refuse("%s has %d %s, the monitor was built for %d" % (noun, x.shape[1], units, monitor.classes))
    if x.shape[0] < 1:
        refuse("an empty batch has no step to record")
    if target is None and not _fused_kl(kl):
        refuse(_BAD_KL)
    if not x.is_cuda:
        refuse("the monitor lives in the fused HIP loss; %s is on %s" % (noun, x.device))
    if x.device != monitor.device:
        refuse("%s is on %s, the monitor on %s" % (noun, x.device, monitor.device))
    if target is not None:
        if target.dtype != torch.int64 or not target.is_contiguous():
            refuse("target must be contiguous int64 class ids, got %s with strides %s" % (target.dtype, tuple(target.stride())))
        if not _fused_kl(kl):
            refuse(_BAD_KL)


def elbo_loss(log_probs, target, kl=None, num_batches=1.0, *, monitor=None):
    """nll_loss(log_probs, target, reduction='sum') + kl / num_batches.  HIP tensors: the fused launches; anything else (the
    CPU host-logic tests of bnn_amd.parallel run on oracle tensors): the same expression in torch ops.

    ``target`` must lie on the device of ``log_probs`` and hold one class id per row: anything else is a ValueError before a
    pointer is handed to the library.  ``monitor``: a ``TrainMonitor`` whose totals and guard word this step is recorded in, by
    the forward launch itself (lbbnn_elbo_loss_monitor); the loss and every gradient are bitwise those of the call without one.
    A monitor needs the fused path -- float32 (B, monitor.classes) log-probabilities on the monitor's HIP device, int64 targets
    -- and anything else is a ValueError naming the mismatch."""
    if torch.is_tensor(target) and log_probs.dim() == 2:
        if target.device != log_probs.device:
            raise ValueError("bnn_amd: elbo_loss: target is on %s, log_probs on %s" % (target.device, log_probs.device))
        if target.numel() != log_probs.shape[0]:
            raise ValueError("bnn_amd: elbo_loss: target has %d element(s), log_probs %d row(s)"
                             % (target.numel(), log_probs.shape[0]))
    if monitor is not None:
        _check_monitored("elbo_loss", "log_probs", "classes", log_probs, kl, monitor, target)
        return _ElboLossFn.apply(log_probs, target, kl if kl is None else kl.reshape(()), 1.0 / float(num_batches), monitor)
    if (log_probs.is_cuda and log_probs.dtype == torch.float32 and log_probs.dim() == 2 and target.dtype == torch.int64
            and target.is_contiguous() and _fused_kl(kl)):
        return _ElboLossFn.apply(log_probs, target, kl if kl is None else kl.reshape(()), 1.0 / float(num_batches), None)
    nll = F.nll_loss(log_probs, target, reduction="sum")
    return nll if kl is None else nll + kl / num_batches


class _ElboBceLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, probs, target, kl, scale, stats, from_head, monitor=None):
        B, O = probs.shape
        _HEAD_GRAD.clear()                         # entries live for one backward pass only
        p = probs if (probs.stride(1) == 1 or O == 1) else probs.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        head = (p.data_ptr(), p.stride(0) if B > 1 else O, target.data_ptr(), O, B, O, _ptr(kl), float(scale), loss.data_ptr(),
                _ptr(stats), 1)
        _launch_loss(p.device, "lbbnn_elbo_bce_loss", head, monitor)
        ctx.save_for_backward(target, p)
        ctx.meta = (B, O, float(scale), kl is not None, bool(from_head) and p is probs)
        return loss

    @staticmethod
    def backward(ctx, g):
        target, p = ctx.saved_tensors
        B, O, scale, has_kl, from_head = ctx.meta
        g = g.contiguous()
        g_probs = torch.empty((B, O), dtype=torch.float32, device=g.device)
        g_logits = torch.empty((B, O), dtype=torch.float32, device=g.device) if from_head else None
        g_kl = torch.empty((), dtype=torch.float32, device=g.device) if has_kl else None
        _lib.launch(g.device, "lbbnn_elbo_bce_loss_backward", g.data_ptr(), p.data_ptr(), p.stride(0) if B > 1 else O,
                    target.data_ptr(), O, B, O, scale, g_probs.data_ptr(), _ptr(g_logits), _ptr(g_kl))
        if from_head:
            _HEAD_GRAD.leave(p, g_probs, g_logits)
        return g_probs, None, g_kl, None, None, None, None


def _bce_target(probs, target):
    """``target`` as the (B, O) float32 block the loss reads, or ValueError naming the mismatch -- checked before any pointer is
    handed to the library."""
    if not torch.is_tensor(target):
        raise ValueError("bnn_amd: elbo_bce_loss: target must be a tensor, got %s" % type(target).__name__)
    if probs.dim() != 2:
        raise ValueError("bnn_amd: elbo_bce_loss: probs must be (B, O), got shape %s" % (tuple(probs.shape),))
    if target.dtype != torch.float32:
        raise ValueError("bnn_amd: elbo_bce_loss: target must be float32 (0 / 1 or probabilities), got %s" % target.dtype)
    if target.device != probs.device:
        raise ValueError("bnn_amd: elbo_bce_loss: target is on %s, probs on %s" % (target.device, probs.device))
    if tuple(target.shape) != tuple(probs.shape) and not (probs.shape[1] == 1 and tuple(target.shape) == (probs.shape[0],)):
        raise ValueError("bnn_amd: elbo_bce_loss: target has shape %s, probs %s" % (tuple(target.shape), tuple(probs.shape)))
    if not target.is_contiguous():
        raise ValueError("bnn_amd: elbo_bce_loss: target must be contiguous (strides %s)" % (tuple(target.stride()),))
    return target.view(probs.shape)


def elbo_bce_loss(probs, target, kl=None, num_batches=1.0, *, stats=None, monitor=None):
    """nn.BCELoss(reduction='sum')(probs, target) + kl / num_batches -- the sim-study scripts' loss for a sigmoid head.

    ``probs`` (B, O) probabilities, ``target`` float32 of the same shape (or (B,) against (B, 1)), contiguous, on the device of
    ``probs``; anything else is a ValueError before any launch.  HIP float32 tensors: ONE forward and ONE backward launch
    (lbbnn_elbo_bce_loss*); when ``probs`` is what a ``head="sigmoid"`` network returned, the backward launch also forms the
    gradient with respect to the logits and the head's backward takes it.  Anything else (CPU tensors): the same expression in
    torch ops.

    ``stats``: an int32[4] device tensor that every call ADDS to -- correct ((p > 0.5) == (y > 0.5)), elements, bad_targets (y
    outside [0, 1] or not finite: no loss, no gradient), nonfinite_probs.  Nothing here reads it: reading it (``stats.tolist()``)
    is the caller's synchronisation, once per epoch in a training loop; zero it with ``stats.zero_()``.

    ``monitor``: a ``TrainMonitor(units, device)`` whose totals and guard word this step is recorded in, by the forward launch
    itself (lbbnn_elbo_bce_loss_monitor); the loss, ``stats`` and every gradient are bitwise those of the call without one.  The
    monitor counts ELEMENTS (b, o), see ``TrainMonitor.result``.  It needs the fused path -- float32 (B, monitor.classes)
    probabilities on the monitor's HIP device, a non-empty batch, ``kl`` None or a one-element float32 HIP tensor -- and anything
    else is a ValueError naming the mismatch."""
    t = _bce_target(probs, target)
    if monitor is not None:
        _check_monitored("elbo_bce_loss", "probs", "units", probs, kl, monitor)
    if stats is not None and not (torch.is_tensor(stats) and stats.dtype == torch.int32 and stats.numel() == 4
                                  and stats.is_contiguous() and stats.device == probs.device):
        raise ValueError("bnn_amd: elbo_bce_loss: stats must be a contiguous int32[4] tensor on %s" % probs.device)
    if not 1 <= probs.shape[1] <= 16 and probs.is_cuda:
        raise ValueError("bnn_amd: elbo_bce_loss: the fused loss takes 1 to 16 output units, got %d" % probs.shape[1])
    if probs.is_cuda and probs.dtype == torch.float32 and _fused_kl(kl):
        from . import layers
        from_head = isinstance(probs.grad_fn, layers._SigmoidHeadFn._backward_cls)
        return _ElboBceLossFn.apply(probs, t, kl if kl is None else kl.reshape(()), 1.0 / float(num_batches), stats, from_head,
                                    monitor)
    ok = (t >= 0) & (t <= 1)
    bce = F.binary_cross_entropy(torch.where(ok, probs, torch.ones_like(probs)), torch.where(ok, t, torch.ones_like(t)),
                                 reduction="sum")
    if stats is not None:
        with torch.no_grad():
            c = ((probs > 0.5) == (t > 0.5)) & ok
            stats += torch.stack([c.sum(), torch.tensor(t.numel(), device=t.device), (~ok).sum(),
                                  (~torch.isfinite(probs)).sum()]).to(torch.int32)
    return bce if kl is None else bce + kl / num_batches


class _ElboGaussianLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, target, log_var, kl, scale, stats, monitor):
        B, O = mean.shape
        m = mean if (mean.stride(1) == 1 or O == 1) else mean.contiguous()
        shared = log_var.dim() == 1
        lv = log_var if (shared or log_var.stride(1) == 1 or O == 1) else log_var.contiguous()
        lv = lv if (not shared or lv.is_contiguous()) else lv.contiguous()
        ldm = m.stride(0) if B > 1 else O
        ldv = 0 if shared else (lv.stride(0) if B > 1 else O)
        if ldm < O:
            m, ldm = m.contiguous(), O                       # (an expanded row: the kernel reads real rows)
        if not shared and ldv < O:
            lv, ldv = lv.contiguous(), O
        loss = torch.empty((), dtype=torch.float32, device=m.device)
        # d loss / d log_var[o] of a shared noise level, up to the factor g: column sums the forward pass leaves as a by-product
        cols = torch.empty(O, dtype=torch.float32, device=m.device) if shared else None
        head = (m.data_ptr(), ldm, target.data_ptr(), O, lv.data_ptr(), ldv, B, O, _ptr(kl), float(scale), loss.data_ptr(),
                _ptr(stats), _ptr(cols))
        _launch_loss(m.device, "lbbnn_elbo_gaussian_loss", head, monitor)
        ctx.save_for_backward(target, m, lv, cols)
        ctx.meta = (B, O, ldm, ldv, float(scale), kl is not None, tuple(log_var.shape))
        return loss

    @staticmethod
    def backward(ctx, g):
        target, m, lv, cols = ctx.saved_tensors
        B, O, ldm, ldv, scale, has_kl, lv_shape = ctx.meta
        g = g.contiguous()
        g_mean = torch.empty((B, O), dtype=torch.float32, device=g.device)
        g_lv = torch.empty(lv_shape, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[2] else None
        g_kl = torch.empty((), dtype=torch.float32, device=g.device) if has_kl else None
        _lib.launch(g.device, "lbbnn_elbo_gaussian_loss_backward", g.data_ptr(), m.data_ptr(), ldm, target.data_ptr(), O,
                    lv.data_ptr(), ldv, B, O, scale, _ptr(cols), g_mean.data_ptr(), _ptr(g_lv), _ptr(g_kl))
        return g_mean, None, g_lv, g_kl, None, None, None


LOG_2PI = 1.8378770664093453


def _gaussian_args(mean, target, log_var):
    """``target`` as the (B, O) float32 block the loss reads and ``log_var`` as given, or ValueError naming the mismatch --
    checked before any pointer is handed to the library."""
    who = "bnn_amd: elbo_gaussian_loss: "
    if not torch.is_tensor(mean) or mean.dim() != 2:
        raise ValueError(who + "mean must be a (B, O) tensor, got %s"
                         % (tuple(mean.shape) if torch.is_tensor(mean) else type(mean).__name__,))
    if mean.dtype != torch.float32:
        raise ValueError(who + "mean must be float32, got %s" % mean.dtype)
    if not torch.is_tensor(target):
        raise ValueError(who + "target must be a tensor, got %s" % type(target).__name__)
    if target.dtype != torch.float32:
        raise ValueError(who + "target must be float32, got %s" % target.dtype)
    if target.device != mean.device:
        raise ValueError(who + "target is on %s, mean on %s" % (target.device, mean.device))
    B, O = mean.shape
    if tuple(target.shape) != (B, O) and not (O == 1 and tuple(target.shape) == (B,)):
        raise ValueError(who + "target has shape %s, mean %s" % (tuple(target.shape), (B, O)))
    if not target.is_contiguous():
        raise ValueError(who + "target must be contiguous (strides %s)" % (tuple(target.stride()),))
    if not torch.is_tensor(log_var):
        raise ValueError(who + "log_var must be a tensor of shape (O,) or (B, O), got %s" % type(log_var).__name__)
    if log_var.dtype != torch.float32:
        raise ValueError(who + "log_var must be float32, got %s" % log_var.dtype)
    if log_var.device != mean.device:
        raise ValueError(who + "log_var is on %s, mean on %s" % (log_var.device, mean.device))
    if tuple(log_var.shape) not in ((O,), (B, O)):
        raise ValueError(who + "log_var has shape %s, expected (%d,) or (%d, %d)" % (tuple(log_var.shape), O, B, O))
    return target.view(B, O)


def elbo_gaussian_loss(mean, target, log_var, kl=None, num_batches=1.0, *, stats=None, monitor=None):
    """sum_{b,o} 0.5 (log(2 pi) + lv + (y - m)^2 exp(-lv)) + kl / num_batches -- ``F.gaussian_nll_loss(mean, target, exp(log_var),
    full=True, reduction="sum") + kl / num_batches``: the ELBO loss of a regression network (``head="identity"``).

    ``mean`` (B, O) float32, possibly a strided view (a column slice of a wider output); ``target`` float32 of the same shape
    (or (B,) against (B, 1)), contiguous, on the device of ``mean``; ``log_var`` float32 on that device, of shape (O,) -- one
    noise level per output unit, typically an ``nn.Parameter`` the optimizer also steps -- or (B, O), one per element and
    possibly a strided view (the other half of a heteroscedastic network's output).  Anything else is a ValueError before any
    launch.  HIP tensors: ONE forward launch and ONE backward launch (lbbnn_elbo_gaussian_loss*); the gradient of a shared
    ``log_var`` is a column sum over the batch that the forward launch leaves as a by-product (fp64, fixed order: the same bits
    from run to run).  CPU tensors: the same expression in torch ops.

    A target that is NaN or infinite is a bad target: no loss term, no gradient, counted.  A non-finite ``mean`` or
    ``log_var`` makes the loss non-finite.

    ``stats``: a float64[4] device tensor that every call ADDS to -- squared-error sum, absolute-error sum, elements with a
    valid target, bad targets.  Nothing here reads it: ``(stats[0] / stats[2]).sqrt()`` is the training RMSE, one read per
    epoch; zero it with ``stats.zero_()``.

    ``monitor``: a ``TrainMonitor(units, device)`` whose totals and guard word this step is recorded in, by the forward launch
    itself (lbbnn_elbo_gaussian_loss_monitor); the loss, ``stats`` and every gradient are bitwise those of the call without one.
    The monitor counts ELEMENTS (b, o), as for ``elbo_bce_loss``.  ``correct`` counts the elements with a valid target and
    |y - m| <= exp(0.5 lv), so ``result()["accuracy"]`` reads as the ONE-SIGMA COVERAGE: about 0.683 for a calibrated Gaussian.
    ``bad_targets`` are the NaN / infinite targets (``result(strict=True)`` raises on them), ``nonfinite_rows`` the elements
    whose mean or log-variance is not finite.  A monitor needs the fused path -- HIP tensors on the monitor's device, a
    non-empty batch, ``kl`` None or a one-element float32 HIP tensor -- and anything else is a ValueError."""
    t = _gaussian_args(mean, target, log_var)
    if monitor is not None:
        _check_monitored("elbo_gaussian_loss", "mean", "units", mean, kl, monitor)     # (_gaussian_args: float32 (B, O) already)
    if stats is not None and not (torch.is_tensor(stats) and stats.dtype == torch.float64 and stats.numel() == 4
                                  and stats.is_contiguous() and stats.device == mean.device):
        raise ValueError("bnn_amd: elbo_gaussian_loss: stats must be a contiguous float64[4] tensor on %s" % mean.device)
    if not 1 <= mean.shape[1] <= 16 and mean.is_cuda:
        raise ValueError("bnn_amd: elbo_gaussian_loss: the fused loss takes 1 to 16 output units, got %d" % mean.shape[1])
    # (an empty batch has no storage to point the kernel at: it takes the torch expression, the kl term alone)
    if mean.is_cuda and _fused_kl(kl) and mean.shape[0] > 0:
        return _ElboGaussianLossFn.apply(mean, t, log_var, kl if kl is None else kl.reshape(()), 1.0 / float(num_batches), stats,
                                         monitor)
    ok = torch.isfinite(t)
    d = torch.where(ok, t, mean.detach()) - mean
    term = 0.5 * ((LOG_2PI + log_var) + (d * d) * torch.exp(-log_var))
    nll = torch.where(ok, term, torch.zeros_like(term)).sum()
    if stats is not None:
        with torch.no_grad():
            dd = torch.where(ok, d, torch.zeros_like(d)).double()
            stats += torch.stack([(dd * dd).sum(), dd.abs().sum(), ok.sum().double(), (~ok).sum().double()])
    return nll if kl is None else nll + kl / num_batches


class _SumKLFn(torch.autograd.Function):
    """kl_total of a network whose layers' KL tails ran in ONE finalize (kl_piggy.h): the total was added on the device in
    layer order by that launch; this node only tells autograd that it is the sum of the per-layer values."""

    @staticmethod
    def forward(ctx, total, slots, *kls):
        ctx.n = len(kls)
        ctx.slots = slots
        return total.detach().view_as(total)

    @staticmethod
    def backward(ctx, g):
        # d loss / d kl is the same number for every layer and is known HERE first: the layers' V1 kernels
        # (lbbnn_mnf_aux_backward: by-products of the forward + this number) run as one launch, each layer's backward
        # picks its result up from its slot (layers._BayesLinearFn)
        slots = [s for s in (ctx.slots or []) if s is not None and "out" not in s and "in" in s]
        if slots and g.is_cuda and g.dtype == torch.float32 and g.numel() == 1:
            from . import ops
            gk = g.contiguous()
            for s, o in zip(slots, ops.mnf_aux_backward_batch([s["in"] for s in slots], gk)):
                s["out"] = o + (gk,)
                s.pop("in")
            g = gk
        ctx.slots = None
        return (None, None) + (g,) * ctx.n
