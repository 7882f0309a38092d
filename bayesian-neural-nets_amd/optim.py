"""``Adam`` with ``torch.optim.Adam``'s constructor and update rule (the optimizer of the reference's training scripts:
``optim.Adam(net.parameters(), lr=...)``, LBBNN-GP-MF-LRT.py:358, LBBNN-GP-MF-MNF.py:421; per-parameter groups in
LBBNN-GP-MF.py:520-554), executed as ONE multi-tensor HIP launch for ALL parameter groups (``lbbnn_adam_step_groups``; one per
``_lib.ADAM_GROUPS_MAX_TENSORS`` tensors) instead of torch's ~115 small kernels for the 66 parameter tensors of the headline net.

Everything a schedule may change lives on the device: one table row ``{lr, beta1, beta2, eps, weight_decay, flags}`` and one
step counter per group, read by the kernel when it runs.  ``step()`` is therefore HIP-graph capturable as it is (no
``capturable=`` switch needed), and a ``torch.optim.lr_scheduler`` or a plain ``group["lr"] = ...`` takes effect on the next
replay of a captured step: ``push_hyperparameters()`` copies the table when a value changed (``step()`` calls it outside a
capture; the graphed steps of ``graphs`` and ``parallel`` call it before every replay).

Beyond torch.optim.Adam's keywords:
  ``decoupled_weight_decay=True``  AdamW's decay, ``p *= 1 - lr * weight_decay`` ahead of the plain update.
  ``max_grad_norm=c``              global L2-norm clipping over all groups (``torch.nn.utils.clip_grad_norm_``'s formula) in one
                                   extra call (two launches).  Unlike ``clip_grad_norm_``, ``.grad`` is NOT rescaled: the
                                   scale is a device scalar applied inside the update; ``optimizer.grad_norm`` is a device
                                   tensor with the norm before clipping of the last step (reading it inside the step needs no
                                   synchronisation).
  ``set_grad_mask(param, mask)``   multiply ``param``'s gradient by ``mask`` inside the update (and inside the norm): the
                                   reference's COND_OPT, ``weight_mu.grad * gammas`` (LBBNN-GP-MF.py:333-336), without a hook.

  ``set_guard(monitor)``           run every step behind a ``bnn_amd.TrainMonitor``'s guard word: a step after a non-finite loss
                                   (or, with ``max_grad_norm``, a non-finite gradient norm) is skipped on the device and counted.

Not supported (raise): ``amsgrad``, ``maximize``, sparse gradients, non-fp32 or CPU parameters, parameters on several devices.

``SGD`` is the same machinery (one base class) with ``torch.optim.SGD``'s constructor and update rule -- the optimizer of the
baseline simulation study: eleven single-tensor groups at two rates, six of them set to 0 at epoch 50
(LBBNN-GP-MFsim_study.py) -- as one ``lbbnn_sgd_step_groups`` launch per list; its table row is ``{lr, momentum, dampening,
weight_decay, flags}``.  One deviation from torch: the ``buf = g`` rule of the first step is per GROUP here (the group's
counter is 0) and per parameter in torch; a parameter that receives its first gradient later than its group differs from torch
only when ``dampening != 0``.
"""
import ctypes

import torch

from . import _lib


def hyper_values(param_groups):
    """The values the device table holds, per group, as plain host numbers: (lr, beta1, beta2, eps, weight_decay, flags).
    flags: _lib.ADAM_F_DECOUPLED from the group's ``decoupled_weight_decay``, _lib.ADAM_F_INACTIVE for a
    group without parameters."""
    rows = []
    for group in param_groups:
        b1, b2 = group["betas"]
        flags = (_lib.ADAM_F_DECOUPLED if group.get("decoupled_weight_decay") else 0) | \
                (0 if group["params"] else _lib.ADAM_F_INACTIVE)
        rows.append((float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), flags))
    return tuple(rows)


def hyper_dirty(pushed, current):
    """True exactly when the table on the device (``pushed``: the hyper_values() it was filled from, None = never) differs
    from ``current`` in some group's lr, betas, eps, weight_decay (or flags), or in the number of groups.  Pure host logic."""
    return pushed is None or tuple(pushed) != tuple(current)


def sgd_hyper_values(param_groups):
    """``SGD``'s table rows as plain host numbers: (lr, momentum, dampening, weight_decay, flags).  flags: _lib.SGD_F_NESTEROV
    from the group's ``nesterov``, _lib.SGD_F_INACTIVE for a group without parameters."""
    rows = []
    for group in param_groups:
        flags = (_lib.SGD_F_NESTEROV if group.get("nesterov") else 0) | (0 if group["params"] else _lib.SGD_F_INACTIVE)
        rows.append((float(group["lr"]), float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]), flags))
    return tuple(rows)


def chunk_entries(entries, limit=None):
    """``entries`` in per-launch lists of at most ``limit`` (default: the kernel's tensor limit); one empty list when there
    is nothing to update (the counters still advance)."""
    limit = limit or _lib.ADAM_GROUPS_MAX_TENSORS
    return [entries[i:i + limit] for i in range(0, len(entries), limit)] or [[]]


class _GroupsOptimizer(torch.optim.Optimizer):
    """What ``Adam`` and ``SGD`` share: the device tables, ``push_hyperparameters``, masks, clipping, and the list launches of
    ``step``.  A subclass names its table (``_NAME``, ``_COLS`` columns, the last one the flags; ``_hyper_values``), its state
    (``_group_state(group, index)``, ``_buffers``: the list's m / v pointers of a parameter, 0 = none) and its entry point (``_ENTRY``)."""
    _NAME = _ENTRY = _hyper_values = None
    _COLS = 0

    def _check_push(self, cur):
        """Host check of the rows about to be copied; raises before anything is copied."""

    # ---- device tables ---------------------------------------------------------------------------------------------------
    # All groups share ONE hyper-parameter table (G rows of lbbnn_adam_hyper_t / lbbnn_sgd_hyper_t) and ONE counter array (G floats);
    # group["step_dev"] is the one-element view of the group's counter.  The tables are (re)built lazily, outside a capture:
    # at the first step, after add_param_group, after load_state_dict.
    def _tables(self):
        tab = self.__dict__.get("_tab")
        groups = self.param_groups
        if tab is not None and tab["n"] == len(groups) and all(g.get("step_dev") is v for g, v in zip(groups, tab["views"])):
            return tab
        dev = next((p.device for g in groups for p in g["params"]), None)
        if dev is None or dev.type != "cuda":
            raise RuntimeError(self._NAME + " needs contiguous float32 parameters on a HIP device")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(self._NAME + ": the parameter groups changed; the device tables cannot be rebuilt inside a "
                               "graph capture (run one eager step, or push_hyperparameters(), first)")
        steps = torch.zeros(len(groups), dtype=torch.float32, device=dev)
        for i, g in enumerate(groups):                                  # counters of the groups that had one carry over
            if g.get("step_dev") is not None:
                steps[i:i + 1].copy_(g["step_dev"].reshape(-1)[:1])
        views = [steps[i:i + 1] for i in range(len(groups))]
        for g, v in zip(groups, views):
            g["step_dev"] = v
        tab = dict(n=len(groups), dev=dev, steps=steps, views=views, hyper=torch.zeros(len(groups), self._COLS, dtype=torch.float32, device=dev),
                   ticket=torch.zeros(4, dtype=torch.int32, device=dev), norm=torch.zeros(1, dtype=torch.float32, device=dev),
                   scale=torch.ones(1, dtype=torch.float32, device=dev), pushed=None, work=None)
        self.__dict__["_tab"] = tab
        self.__dict__.pop("_lists", None)
        return tab

    def push_hyperparameters(self):
        """Copy the groups' lr / betas / eps / weight_decay to the device table if one of them changed since the last push
        (``hyper_dirty``); returns whether it copied.  Call it before replaying a captured ``step()`` (the graphed steps of
        this package do); an eager ``step()`` calls it itself.  Never inside a capture: a host-to-device copy there would be
        replayed with the values of capture time."""
        tab = self._tables()
        cur = self._hyper_values(self.param_groups)
        if not hyper_dirty(tab["pushed"], cur):
            return False
        self._check_push(cur)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(self._NAME + ".push_hyperparameters: called inside a graph capture")
        nf = self._COLS - 1                                         # the float columns; the last one holds the flags
        host = torch.empty(len(cur), self._COLS, dtype=torch.float32)
        host[:, :nf] = torch.tensor([r[:nf] for r in cur], dtype=torch.float64).to(torch.float32)   # rounded as c_float rounds
        host.view(torch.int32)[:, nf] = torch.tensor([r[nf] for r in cur], dtype=torch.int32)
        tab["hyper"].copy_(host)
        tab["pushed"] = cur
        return True

    @property
    def grad_norm(self):
        """Device tensor (1 element): the global L2 norm of the (masked) gradients of the last step, before clipping.  Only
        written when ``max_grad_norm`` is set."""
        return self._tables()["norm"]

    def set_grad_mask(self, param, mask):
        """Multiply ``param``'s gradient elementwise by ``mask`` inside the update: a tensor of ``param``'s shape, or a
        zero-argument callable returning the current one (``lambda: layer.gammas``: the layer rebinds ``gammas`` on every
        forward), resolved at ``step()`` time -- under a capture to the graph's static buffer.  ``None`` removes the mask."""
        if not any(param is p for g in self.param_groups for p in g["params"]):
            raise ValueError(self._NAME + ".set_grad_mask: not a parameter of this optimizer")
        masks = self.__dict__.setdefault("_masks", {})
        if mask is None:
            masks.pop(id(param), None)
        else:
            masks[id(param)] = mask

    def set_guard(self, monitor):
        """``monitor``: a ``bnn_amd.TrainMonitor`` -- every ``step()`` then runs behind its guard word (the ``_guarded`` entry
        point): after a loss that is not finite, or with ``max_grad_norm`` set a gradient norm that is not, the step changes no
        parameter, moment or step counter and adds 1 to the monitor's ``skipped_steps``, all on the device (a replayed graph
        included: set the guard before building the graphed step).  ``None``: the plain step again.  Not part of ``state_dict``."""
        from .losses import TrainMonitor
        if monitor is not None and not isinstance(monitor, TrainMonitor):
            raise TypeError(self._NAME + ".set_guard takes a bnn_amd.TrainMonitor or None, got %s" % type(monitor).__name__)
        self.__dict__["_guard"] = monitor

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self.__dict__.pop("_lists", None)                       # the tables regrow at the next step / push (outside capture)

    def _resolve_mask(self, p, keep):
        m = self.__dict__.get("_masks", {}).get(id(p))
        if m is None:
            return None
        if callable(m) and not isinstance(m, torch.Tensor):
            m = m()
        if not isinstance(m, torch.Tensor) or m.shape != p.shape or m.device != p.device:
            raise RuntimeError(self._NAME + ": a gradient mask must be a tensor of its parameter's shape on its device")
        if m.dtype != torch.float32 or not m.is_contiguous():
            m = m.detach().contiguous().float()
            keep.append(m)
        return m

    @torch.no_grad()
    def step(self, closure=None, grads=None):
        """``grads``: optional (params, tensors) pair -- gradients to use instead of ``p.grad`` (the views of a
        data-parallel flat bucket after its all-reduce, so they are consumed where RCCL left them)."""
        override = {}
        if grads is not None:
            override = {id(p): g for p, g in zip(*grads)}
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not any(g["params"] for g in self.param_groups):
            return loss
        tab = self._tables()
        if not torch.cuda.is_current_stream_capturing():
            self.push_hyperparameters()
        elif hyper_dirty(tab["pushed"], self._hyper_values(self.param_groups)):
            raise RuntimeError(self._NAME + ": hyper-parameters changed since the last push and step() runs inside a graph "
                               "capture; call push_hyperparameters() before the capture")
        dev = tab["dev"]
        keep = []
        entries = []                                                # (group index, parameter, gradient, mask or None)
        for gi, group in enumerate(self.param_groups):
            self._group_state(group, gi)
            for p in group["params"]:
                g = override.get(id(p), p.grad)
                if g is None:
                    continue
                if p.device != dev:
                    raise RuntimeError(self._NAME + ": all parameters must live on one device")
                if g.is_sparse:
                    raise RuntimeError(self._NAME + " does not support sparse gradients")
                if not g.is_contiguous() or g.dtype != torch.float32:
                    g = g.contiguous().float()
                    keep.append(g)
                entries.append((gi, p, g, self._resolve_mask(p, keep)))
        stream = torch.cuda.current_stream(dev).cuda_stream
        chunks = chunk_entries(entries)
        cache = self.__dict__.setdefault("_lists", {})              # not in param_groups: state_dict() stays plain
        lists = []
        for ci, chunk in enumerate(chunks):
            # the kernel-argument list is rebuilt only when a pointer changed (gradients living in a flat bucket, or
            # accumulated in place, keep their addresses: 7 ctypes stores per tensor saved on every step)
            # (the m / v addresses are part of the key: optimizer.state may be replaced or cleared between steps --
            # load_state_dict, a fresh state after a checkpoint restore -- and a stale list would update freed buffers; so is
            # the mask's: a callable may hand out another buffer)
            key = tuple((gi, p.data_ptr(), g.data_ptr(), *self._buffers(p), 0 if m is None else m.data_ptr())
                        for gi, p, g, m in chunk)
            hit = cache.get(ci)
            if hit is None or hit[0] != key:
                lst = _lib.AdamGroupList()
                lst.n = len(chunk)
                for k, (gi, p, g, m) in enumerate(chunk):
                    bm, bv = self._buffers(p)                       # 0: no such buffer (SGD without momentum; SGD has no v)
                    lst.p[k], lst.g[k], lst.mask[k] = p.data_ptr(), g.data_ptr(), (None if m is None else m.data_ptr())
                    lst.m[k], lst.v[k] = bm or None, bv or None
                    lst.numel[k] = p.numel()
                    lst.group[k] = gi
                cache[ci] = (key, lst)
            else:
                lst = hit[1]
            lists.append(lst)
        lib = _lib.lib()
        scale = None
        if self.max_grad_norm is not None and entries:
            # global norm first, over every list: per-workgroup partials, then ONE fixed-order reduction that leaves the norm
            # and min(1, max_norm / (norm + 1e-6)) on the device for the update launches below
            counts = [sum((p.numel() + _lib.ADAM_CHUNK - 1) // _lib.ADAM_CHUNK for _, p, _, _ in chunk) for chunk in chunks]
            need = lib.lbbnn_grad_sumsq_workspace(sum(counts))
            if tab["work"] is None or tab["work"].numel() < need:
                tab["work"] = torch.empty(need, dtype=torch.float32, device=dev)
            off = 0
            for ci, lst in enumerate(lists):
                last = ci == len(lists) - 1
                rc = lib.lbbnn_grad_sumsq(ctypes.byref(lst), tab["work"].data_ptr(), off, off + counts[ci] if last else 0,
                                          self.max_grad_norm, tab["norm"].data_ptr(), tab["scale"].data_ptr(), stream)
                _lib.check(rc, "lbbnn_grad_sumsq")
                off += counts[ci]
            scale = tab["scale"].data_ptr()
        guard = self.__dict__.get("_guard")
        if guard is not None and guard.device != dev:
            raise RuntimeError(self._NAME + ": the guard's monitor is on %s, the parameters on %s" % (guard.device, dev))
        name = self._ENTRY if guard is None else self._ENTRY + "_guarded"
        entry = getattr(lib, name)
        # (every list of a guarded step reads the same guard word and scale; the last one, which advances, counts the skip)
        extra = () if guard is None else (guard._guard.data_ptr(), guard._skipped_ptr())
        for ci, lst in enumerate(lists):
            rc = entry(ctypes.byref(lst), tab["hyper"].data_ptr(), tab["steps"].data_ptr(), tab["n"], scale,
                       tab["ticket"].data_ptr(), 1 if ci == len(lists) - 1 else 0, *extra, stream)
            _lib.check(rc, name)
        del keep
        return loss


class Adam(_GroupsOptimizer):
    _NAME, _ENTRY, _COLS = "bnn_amd.optim.Adam", "lbbnn_adam_step_groups", 6
    _hyper_values = staticmethod(hyper_values)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 maximize=False, capturable=True, decoupled_weight_decay=False, max_grad_norm=None):
        if amsgrad or maximize:
            raise NotImplementedError("bnn_amd.optim.Adam: amsgrad / maximize are not implemented")
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("bnn_amd.optim.Adam: invalid hyper-parameter")
        if max_grad_norm is not None and not (max_grad_norm > 0):
            raise ValueError("bnn_amd.optim.Adam: max_grad_norm must be positive (or None)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # (the extra keys are torch.optim.Adam's own group keys at their defaults: a state_dict of this optimizer then loads
        # into torch.optim.Adam and back)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=bool(decoupled_weight_decay)))

    def _group_state(self, group, gi):
        st = self.state
        for p in group["params"]:
            if p not in st or "exp_avg" not in st[p]:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("bnn_amd.optim.Adam needs contiguous float32 parameters on a HIP device")
                st[p]["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st[p]["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _buffers(self, p):
        st = self.state[p]
        return st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()

    # torch.optim.Adam keeps one ``state[p]["step"]`` per parameter; this optimizer keeps ONE device-side counter per
    # parameter group (``group["step_dev"]``: every parameter of a group is updated in the same launch, so their counts
    # cannot differ).  state_dict() / load_state_dict() translate between the two, so that checkpoints interchange with
    # torch.optim.Adam and bias correction continues where it stopped.
    def state_dict(self):
        sd = super().state_dict()
        for gi, group in enumerate(self.param_groups):
            step = group.get("step_dev")
            sg = sd["param_groups"][gi]
            sg.pop("step_dev", None)
            if step is not None:
                count = float(step.detach().reshape(-1)[0])          # one device -> host read per group (checkpoint time only)
                for idx in sg["params"]:
                    if idx in sd["state"]:
                        # a tensor of its OWN per parameter, on the CPU, as torch.optim.Adam keeps it when capturable=False: its
                        # foreach path adds 1 to every listed step tensor, so a tensor shared by two parameters would count double
                        sd["state"][idx] = dict(sd["state"][idx], step=torch.tensor(count, dtype=torch.float32))
        return sd

    def load_state_dict(self, state_dict):
        steps = {}
        for gi, sg in enumerate(state_dict["param_groups"]):
            for idx in sg["params"]:
                st = state_dict["state"].get(idx)
                if st is not None and "step" in st:
                    steps[gi] = float(torch.as_tensor(st["step"]).reshape(-1)[0])
                    break
        super().load_state_dict(state_dict)
        self.__dict__.pop("_lists", None)                       # kernel-argument lists point at the old m / v buffers
        self.__dict__.pop("_tab", None)
        for gi, group in enumerate(self.param_groups):
            group.pop("step_dev", None)
            for p in group["params"]:
                self.state.get(p, {}).pop("step", None)
        if any(g["params"] for g in self.param_groups):
            tab = self._tables()                                    # fresh counters, all zero
            for gi, count in steps.items():
                tab["steps"][gi] = count


class SGD(_GroupsOptimizer):
    """``torch.optim.SGD``'s constructor (plus ``max_grad_norm``), group keys and update rule; see the module docstring.
    ``state[p]["momentum_buffer"]`` exists only for the groups whose momentum is non-zero at their first step; pushing a non-zero
    momentum to a group that stepped without buffers raises (its first-step rule ``buf = g`` can no longer be applied)."""
    _NAME, _ENTRY, _COLS = "bnn_amd.optim.SGD", "lbbnn_sgd_step_groups", 5
    _hyper_values = staticmethod(sgd_hyper_values)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 max_grad_norm=None):
        if maximize:
            raise NotImplementedError("bnn_amd.optim.SGD: maximize is not implemented")
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("bnn_amd.optim.SGD: invalid hyper-parameter")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("bnn_amd.optim.SGD: Nesterov momentum requires a momentum and zero dampening")
        if max_grad_norm is not None and not (max_grad_norm > 0):
            raise ValueError("bnn_amd.optim.SGD: max_grad_norm must be positive (or None)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # (torch.optim.SGD's own group keys: a state_dict of this optimizer loads into torch.optim.SGD and back)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=bool(nesterov), maximize=False, foreach=None, differentiable=False, fused=None))

    def _has_buffers(self, group):
        return any("momentum_buffer" in self.state.get(p, {}) for p in group["params"])

    def _check_push(self, cur):
        bare = self.__dict__.get("_bare", ())
        for gi, row in enumerate(cur):
            if row[1] != 0 and gi in bare:
                raise RuntimeError("bnn_amd.optim.SGD: group %d stepped without momentum and has no momentum buffers; a non-zero "
                                   "momentum cannot be pushed to it (build the optimizer with the momentum, or load a state "
                                   "with buffers)" % gi)

    def _group_state(self, group, gi):
        # buffers are made at the group's first step (zeros: the kernel's first step overwrites them, and a parameter whose
        # first gradient comes later starts from 0 -- the deviation the module docstring names); a group that steps without
        # momentum is remembered as bare
        checked = self.__dict__.setdefault("_checked", set())       # parameters whose device / dtype / layout were looked at
        for p in group["params"]:
            if id(p) not in checked:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("bnn_amd.optim.SGD needs contiguous float32 parameters on a HIP device")
                checked.add(id(p))
        bare = self.__dict__.setdefault("_bare", set())
        if group["momentum"] == 0:
            if gi not in bare and group["params"] and not self._has_buffers(group):
                bare.add(gi)
            return
        st = self.state
        for p in group["params"]:
            if "momentum_buffer" not in st[p]:
                st[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _buffers(self, p):
        buf = self.state.get(p, {}).get("momentum_buffer")
        return (0 if buf is None else buf.data_ptr()), 0

    # torch.optim.SGD keeps no step count: whether a buffer exists is its "first step".  Here the group's device counter is;
    # state_dict() / load_state_dict() translate, so that checkpoints interchange with torch.optim.SGD.
    def state_dict(self):
        sd = super().state_dict()
        for gi, group in enumerate(self.param_groups):
            step = group.get("step_dev")
            sg = sd["param_groups"][gi]
            sg.pop("step_dev", None)
            count = 0.0 if step is None else float(step.detach().reshape(-1)[0])   # one device -> host read per group
            if count == 0:                                      # not stepped: torch initialises the buffers itself
                for idx in sg["params"]:
                    if idx in sd["state"]:
                        st = {k: v for k, v in sd["state"][idx].items() if k != "momentum_buffer"}
                        if st:
                            sd["state"][idx] = st
                        else:
                            del sd["state"][idx]
        return sd

    def load_state_dict(self, state_dict):
        with_buffer = set()
        for gi, sg in enumerate(state_dict["param_groups"]):
            if any((state_dict["state"].get(idx) or {}).get("momentum_buffer") is not None for idx in sg["params"]):
                with_buffer.add(gi)
        super().load_state_dict(state_dict)
        self.__dict__.pop("_lists", None)                       # kernel-argument lists point at the old buffers
        self.__dict__.pop("_tab", None)
        self.__dict__.pop("_bare", None)
        for group in self.param_groups:
            group.pop("step_dev", None)
            for p in group["params"]:
                if p in self.state and self.state[p].get("momentum_buffer", 0) is None:
                    del self.state[p]["momentum_buffer"]
        if any(g["params"] for g in self.param_groups):
            tab = self._tables()                                    # fresh counters, all zero
            for gi in with_buffer:
                tab["steps"][gi] = 1.0
