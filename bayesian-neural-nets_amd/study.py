"""Replicate studies: R independent one-layer LRT or planar-MNF networks with a sigmoid head trained in one launch.

The simulation study of the latent-binary papers (LBBNN-GP-MF-MNFsim_study.py:305-395) builds k = 100 networks from seeds
0..99, trains each for 500 epochs of 5 batches with the Adam rates switched at epochs 50 / 100 / 450, and reduces the 100 rows of
``sigmoid(lambdal)`` to an RMSE per covariate and a selection table.  One such network is a few hundred floats:
``fit_replicates`` hands every replicate to one workgroup of ``lbbnn_lrt_study_fit`` (csrc/lrt_study.hip), which
keeps the replicate's parameters, Adam state and Philox state on chip and loops over epochs and batches itself.

    nets = study.make_replicates(100, (20, 1), priors=PRIORS, device=DEVICE)
    res = study.fit_replicates(nets, x, y, epochs=500, batch_size=400, lr=RATES, restarts=(50, 100, 450))
    print(study.selection_summary(res.inclusion_probabilities[:, 0], support))

The script's own family, MNF networks, goes through the same kernel's second instantiation (``lbbnn_mnf_study_fit``; DESIGN.md
9.6) with planar flows and three rate groups -- the named tensors, z_flow, r_flow:

    nets = study.make_mnf_replicates(100, (20, 1), num_transforms=2, priors=PRIORS, device=DEVICE)
    res = study.fit_mnf_replicates(nets, x, y, epochs=500, batch_size=400, lr=RATES, lr_z_flow=Z_RATES, lr_r_flow=R_RATES,
                                   restarts=(50, 100, 450))

Not built: baseline replicates, RNVP / MNF-type flows, hidden layers, SGD, shuffled batches, HIP-graph capture of the call,
data parallel.  Train such networks one by one with ``graphs.make_graphed_train_step``.
"""
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib, ops
from ._lib import Priors
from .layers import LRTBayesianNetwork, MNFBayesianNetwork

PARAM_NAMES = ("weight_mu", "weight_rho", "lambdal", "bias_mu", "bias_rho")      # the order of a replicate's packed row
MNF_VECTOR_NAMES = ("q0_mean", "q0_log_var", "r0_c", "r0_b1", "r0_b2")          # ... then z_flow.<t>.u / .w / .b, r_flow likewise
HISTORY_COLUMNS = ("loss_mean", "nll_mean", "accuracy", "last_loss", "last_nll", "skipped_steps")
STEPS_PER_LAUNCH = 2048        # default bound of one launch (epochs_per_launch=None): whole epochs of at most this many steps


class StudyState(NamedTuple):
    """What a fit leaves besides the parameters, all on the device: pass it back as ``state=`` to continue.  ``exp_avg`` /
    ``exp_avg_sq`` are (R, 3 O I + 2 O) rows packed as ``PARAM_NAMES`` (``unpack`` gives the named views; MNF replicates:
    ``mnf_row_width`` wide, ``unpack_mnf``), ``step`` the (R)
    float Adam counters, ``rng`` the (R, 2) int64 Philox states {seed, offset} -- a replicate's offset grows by one per
    step, skipped steps included -- and ``skipped_steps`` the (R) int64 running counts."""
    exp_avg: torch.Tensor
    exp_avg_sq: torch.Tensor
    step: torch.Tensor
    rng: torch.Tensor
    skipped_steps: torch.Tensor


class StudyResult(NamedTuple):
    inclusion_probabilities: torch.Tensor      # (R, O, I): sigmoid(lambdal)
    params: dict                               # name -> (R, O, I) / (R, O) views of the trained parameters
    state: StudyState
    history: torch.Tensor                      # (R, epochs, 6) float64, columns HISTORY_COLUMNS
    skipped_steps: torch.Tensor                # (R) int64: state.skipped_steps


def unpack(packed: torch.Tensor, O: int, I: int) -> dict:
    """Named views of (R, 3 O I + 2 O) packed rows: weights (R, O, I), biases (R, O)."""
    R, OI = packed.shape[0], O * I
    out = {n: packed[:, q * OI:(q + 1) * OI].view(R, O, I) for q, n in enumerate(PARAM_NAMES[:3])}
    out["bias_mu"] = packed[:, 3 * OI:3 * OI + O]
    out["bias_rho"] = packed[:, 3 * OI + O:3 * OI + 2 * O]
    return out


def mnf_row_width(O: int, I: int, Tz: int, Tr: int) -> int:
    """P of an MNF replicate's packed row."""
    return 3 * O * I + 2 * O + 5 * I + (Tz + Tr) * (2 * I + 1)


def unpack_mnf(packed: torch.Tensor, O: int, I: int, Tz: int, Tr: int) -> dict:
    """Named views of (R, P) packed rows of MNF replicates, in the order of ``MNFBayesianLinear._param_list()``: the five names
    of ``unpack``, then q0_mean, q0_log_var, r0_c, r0_b1, r0_b2 (R, I), then ``z_flow.<t>.u`` / ``.w`` (R, I) and ``.b`` (R, 1)
    for t < Tz and ``r_flow.<t>...`` for t < Tr."""
    if packed.shape[1] != mnf_row_width(O, I, Tz, Tr):
        raise ValueError("bnn_amd.study: a packed MNF row of O = %d, I = %d, Tz = %d, Tr = %d is %d wide, got %d"
                         % (O, I, Tz, Tr, mnf_row_width(O, I, Tz, Tr), packed.shape[1]))
    out = unpack(packed, O, I)
    at = 3 * O * I + 2 * O
    for n in MNF_VECTOR_NAMES:
        out[n] = packed[:, at:at + I]
        at += I
    for fl, T in (("z_flow", Tz), ("r_flow", Tr)):
        for t in range(T):
            out["%s.%d.u" % (fl, t)] = packed[:, at:at + I]
            out["%s.%d.w" % (fl, t)] = packed[:, at + I:at + 2 * I]
            out["%s.%d.b" % (fl, t)] = packed[:, at + 2 * I:at + 2 * I + 1]
            at += 2 * I + 1
    return out


def check_shapes(I: int, O: int, batch_size: int, N: int, R: int):
    """The limits of lbbnn_lrt_study_fit (include/lbbnn.h), refused here with their names."""
    if not (1 <= I <= _lib.STUDY_MAX_I and 1 <= O <= _lib.STUDY_MAX_O and O * I <= _lib.STUDY_MAX_WEIGHTS):
        raise ValueError("bnn_amd.study: a replicate takes 1 <= I <= %d inputs, 1 <= O <= %d units and O * I <= %d weights, got "
                         "I = %d, O = %d; train larger networks one by one with graphs.make_graphed_train_step"
                         % (_lib.STUDY_MAX_I, _lib.STUDY_MAX_O, _lib.STUDY_MAX_WEIGHTS, I, O))
    if not 1 <= batch_size <= _lib.STUDY_MAX_BATCH:
        raise ValueError("bnn_amd.study: batch_size must be in [1, %d], got %d" % (_lib.STUDY_MAX_BATCH, batch_size))
    if N < 1:
        raise ValueError("bnn_amd.study: the data set has no rows")
    if not 1 <= R <= 65535:
        raise ValueError("bnn_amd.study: 1 to 65535 replicates per call, got %d" % R)


def _check_net(net):
    if not isinstance(net, LRTBayesianNetwork):
        raise NotImplementedError("bnn_amd.study: replicates are lrt.BayesianNetwork (one LRT layer, sigmoid head), got %s; "
                                  "planar-MNF networks go through fit_mnf_replicates; train other MNF, baseline and VD networks "
                                  "one by one with graphs.make_graphed_train_step" % type(net).__name__)
    if len(net.dims) != 2:
        raise ValueError("bnn_amd.study: a replicate has one layer, got dims=%s; train deeper networks one by one with "
                         "graphs.make_graphed_train_step" % (net.dims,))
    if net.head != "sigmoid":
        raise ValueError('bnn_amd.study: a replicate has head="sigmoid", got %r; use graphs.make_graphed_train_step' % net.head)


def make_replicates(R: int, dims, seeds: Optional[Sequence[int]] = None, priors=None, lambdal_init=(1.5, 2.5), device=None):
    """R networks ``lrt.BayesianNetwork(dims, head="sigmoid", priors=priors[r], lambdal_init=...)``, replicate r built after
    ``torch.manual_seed(seeds[r])`` (default seeds 0 .. R - 1, the script's): its initial values are exactly those of the
    network a user builds by hand from that seed.  ``priors``: one ``Priors`` for all, or a sequence of R."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 2:
        raise ValueError("bnn_amd.study: a replicate has one layer (dims = (I, O)), got dims=%s; train deeper networks one by "
                         "one with graphs.make_graphed_train_step" % (dims,))
    seeds = list(range(R)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != R:
        raise ValueError("bnn_amd.study: %d seeds for %d replicates" % (len(seeds), R))
    plist = list(priors) if isinstance(priors, (list, tuple)) else [priors] * R
    if len(plist) != R:
        raise ValueError("bnn_amd.study: %d priors for %d replicates" % (len(plist), R))
    nets = []
    for r in range(R):
        torch.manual_seed(seeds[r])
        net = LRTBayesianNetwork(dims, head="sigmoid", priors=plist[r], lambdal_init=lambdal_init)
        nets.append(net.to(device) if device is not None else net)
    return nets


def _priors_table(nets, priors, dev):
    R = len(nets)
    if priors is None:
        plist = [n.l1.priors for n in nets]
    else:
        plist = list(priors) if isinstance(priors, (list, tuple)) else [priors] * R
    if len(plist) != R:
        raise ValueError("bnn_amd.study: %d priors for %d replicates" % (len(plist), R))
    rows = [(p.mu_prior, p.sigma_prior, p.alpha_prior, p.bias_mu_prior, p.bias_sigma_prior) for p in plist]
    if all(row == rows[0] for row in rows):
        rows = rows[:1]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(dev)       # rounded as c_float rounds


def _lr_table(lr, R, epochs, dev):
    if torch.is_tensor(lr):
        if not lr.is_cuda:
            raise RuntimeError("bnn_amd.study: an lr tensor must be on the HIP device (no CPU path); pass a sequence otherwise")
        if tuple(lr.shape) not in ((epochs,), (R, epochs)):
            raise ValueError("bnn_amd.study: an lr tensor is (epochs,) or (R, epochs), got %s" % (tuple(lr.shape),))
        return lr.to(device=dev, dtype=torch.float32).contiguous()
    if isinstance(lr, (int, float)):
        return torch.full((epochs,), float(lr), dtype=torch.float64).to(torch.float32).to(dev)
    vals = [float(v) for v in lr]
    if len(vals) != epochs:
        raise ValueError("bnn_amd.study: %d rates for %d epochs" % (len(vals), epochs))
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32).to(dev)


def _named_tensors(net):
    """[(name, tensor)] of a replicate's layer in the order of its packed row."""
    l1 = net.l1
    out = [(n, getattr(l1, n)) for n in PARAM_NAMES]
    if isinstance(net, MNFBayesianNetwork):
        out += [(n, getattr(l1, n)) for n in MNF_VECTOR_NAMES]
        for fl in ("z_flow", "r_flow"):
            for t, tr in enumerate(getattr(l1, fl).transforms):
                out += [("%s.%d.u" % (fl, t), tr.u), ("%s.%d.w" % (fl, t), tr.w), ("%s.%d.b" % (fl, t), tr.bias)]
    return out


def _fit(nets, check_net, x, y, epochs, batch_size, lr_table, restarts, betas, eps, weight_decay, seeds, offset, priors,
         epochs_per_launch, state, row_width, launch, unpack_rows) -> StudyResult:
    """What fit_replicates and fit_mnf_replicates share: the checks, the tables, the launches and the copy back.
    ``check_net(net)`` refuses and returns what must agree between replicates; ``lr_table(R, epochs, dev)``,
    ``row_width(key)``, ``launch(key, **tensors)`` and ``unpack_rows(key, packed)`` are the family's."""
    nets = list(nets)
    if not nets:
        raise ValueError("bnn_amd.study: no replicates")
    keys = [check_net(n) for n in nets]
    if any(n.dims != nets[0].dims for n in nets):
        raise ValueError("bnn_amd.study: the replicates differ in dims: %s" % sorted({n.dims for n in nets}))
    if any(k != keys[0] for k in keys):
        raise ValueError("bnn_amd.study: the replicates differ in their transform counts (z_flow, r_flow): %s" % sorted(set(keys)))
    key = keys[0]
    I, O = nets[0].dims
    R = len(nets)
    dev = nets[0].l1.weight_mu.device
    for name, t in (("x", x), ("y", y), ("parameters", nets[0].l1.weight_mu)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("bnn_amd.study: %s must be on a HIP device (there is no CPU path)" % name)
    if any(p.device != dev for n in nets for p in n.parameters()):
        raise RuntimeError("bnn_amd.study: the replicates must all be on %s" % dev)
    if x.dim() not in (2, 3) or y.dim() not in (2, 3):
        raise ValueError("bnn_amd.study: x is (N, I) or (R, N, I) and y (N, O) or (R, N, O)")
    N = x.shape[-2]
    epochs, batch_size = int(epochs), int(batch_size)
    check_shapes(I, O, batch_size, N, R)
    if tuple(x.shape) not in ((N, I), (R, N, I)) or tuple(y.shape) not in ((N, O), (R, N, O)):
        raise ValueError("bnn_amd.study: x is (N, %d) or (%d, N, %d) and y (N, %d) or (%d, N, %d), got %s and %s"
                         % (I, R, I, O, R, O, tuple(x.shape), tuple(y.shape)))
    if epochs < 1:
        raise ValueError("bnn_amd.study: epochs must be at least 1")
    x = x.to(torch.float32).contiguous()
    y = y.to(torch.float32).contiguous()
    nb = -(-N // batch_size)
    if epochs_per_launch is None:
        epochs_per_launch = max(1, STEPS_PER_LAUNCH // nb)
    epochs_per_launch = int(epochs_per_launch)
    if epochs_per_launch < 1:
        raise ValueError("bnn_amd.study: epochs_per_launch must be at least 1")
    rs = sorted({int(e) for e in restarts})
    if rs and not (0 <= rs[0] and rs[-1] < epochs):
        raise ValueError("bnn_amd.study: restarts are epoch indices in [0, epochs)")

    def per_replicate(v, name):
        vals = [float(q) for q in v] if isinstance(v, (list, tuple)) else [float(v)] * R
        if len(vals) != R:
            raise ValueError("bnn_amd.study: %d values of %s for %d replicates" % (len(vals), name, R))
        return vals
    pairs = list(betas) if isinstance(betas, (list, tuple)) and isinstance(betas[0], (list, tuple)) else [tuple(betas)] * R
    if len(pairs) != R:
        raise ValueError("bnn_amd.study: %d beta pairs for %d replicates" % (len(pairs), R))
    eps_r, wd_r = per_replicate(eps, "eps"), per_replicate(weight_decay, "weight_decay")
    for (b1, b2), e, w in zip(pairs, eps_r, wd_r):
        if not (0 <= b1 < 1 and 0 <= b2 < 1) or e < 0 or w < 0:
            raise ValueError("bnn_amd.study: invalid Adam hyper-parameter")
    hyper = torch.zeros(R, 6, dtype=torch.float64)
    hyper[:, 1] = torch.tensor([p[0] for p in pairs], dtype=torch.float64)
    hyper[:, 2] = torch.tensor([p[1] for p in pairs], dtype=torch.float64)
    hyper[:, 3] = torch.tensor(eps_r, dtype=torch.float64)
    hyper[:, 4] = torch.tensor(wd_r, dtype=torch.float64)
    hyper = hyper.to(torch.float32).to(dev)                             # (column 5, the flags word, is zero)

    with torch.no_grad():
        packed = torch.stack([torch.cat([t.detach().reshape(-1) for _, t in _named_tensors(n)]) for n in nets])
    packed = packed.to(torch.float32).contiguous()
    P = row_width(key, O, I)
    if state is None:
        if seeds is None:
            base = ops.RngState.get(dev).seed
            seeds = [base + r for r in range(R)]
        seeds = [int(s) for s in seeds]
        if len(seeds) != R:
            raise ValueError("bnn_amd.study: %d seeds for %d replicates" % (len(seeds), R))
        rows = []
        for s in seeds:
            s &= 0xFFFFFFFFFFFFFFFF
            rows.append([s - (1 << 64) if s >= 1 << 63 else s, int(offset)])
        st = StudyState(torch.zeros(R, P, dtype=torch.float32, device=dev), torch.zeros(R, P, dtype=torch.float32, device=dev),
                        torch.zeros(R, dtype=torch.float32, device=dev), torch.tensor(rows, dtype=torch.int64).to(dev),
                        torch.zeros(R, dtype=torch.int64, device=dev))
    else:
        for name, t, shape in (("exp_avg", state.exp_avg, (R, P)), ("exp_avg_sq", state.exp_avg_sq, (R, P)),
                               ("step", state.step, (R,)), ("rng", state.rng, (R, 2)), ("skipped_steps", state.skipped_steps, (R,))):
            if not t.is_cuda or tuple(t.shape) != shape:
                raise ValueError("bnn_amd.study: state.%s must be a device tensor of shape %s" % (name, shape))
        st = StudyState(*(t.clone().contiguous() for t in state))       # the caller's state is left as it is
    prior_tab = _priors_table(nets, priors, dev)
    lr_tab = lr_table(R, epochs, dev)
    restart_tab = torch.tensor(rs, dtype=torch.int32).to(dev) if rs else None
    history = torch.zeros(R, epochs, len(HISTORY_COLUMNS), dtype=torch.float64, device=dev)
    for first in range(0, epochs, epochs_per_launch):
        launch(key, params=packed, exp_avg=st.exp_avg, exp_avg_sq=st.exp_avg_sq, step=st.step, rng=st.rng,
               skipped=st.skipped_steps, x=x, y=y, priors=prior_tab, hyper=hyper, lr=lr_tab, restarts=restart_tab,
               history=history, I=I, O=O, batch=batch_size, first_epoch=first, n_epochs=min(epochs_per_launch, epochs - first))
    named = unpack_rows(key, packed, O, I)
    with torch.no_grad():
        for r, n in enumerate(nets):
            for name, t in _named_tensors(n):
                t.copy_(named[name][r].view_as(t))
    return StudyResult(torch.sigmoid(named["lambdal"]), named, st, history, st.skipped_steps)


def fit_replicates(nets, x, y, epochs: int, batch_size: int, lr=0.01, restarts=(), betas=(0.9, 0.999), eps: float = 1e-8,
                   weight_decay: float = 0.0, seeds=None, offset: int = 0, priors=None, epochs_per_launch: Optional[int] = None,
                   state: Optional[StudyState] = None) -> StudyResult:
    """Train the R networks of ``nets`` (``make_replicates``, or hand-built ``lrt.BayesianNetwork((I, O), head="sigmoid")`` of
    equal dims) independently on BCELoss(sum) + kl * batch_size / N with Adam, unshuffled batches in order, the last one of an
    epoch possibly short -- the loop of the sim-study scripts -- in ceil(epochs / epochs_per_launch) launches, and copy every
    replicate's trained parameters back into ``nets[r]``.

    x: (N, I) shared or (R, N, I); y: (N, O) or (R, N, O) float targets in [0, 1].  lr: one rate, a sequence of ``epochs``
    rates (shared), or a device tensor (epochs,) / (R, epochs).  restarts: epochs at whose start the moments and the step
    counter start afresh (the scripts re-create ``optim.Adam`` at 50 / 100 / 450).  betas / eps / weight_decay: one value or a
    sequence of R.  seeds / offset: replicate r draws its step t from Philox state {seeds[r], offset + t} as layer l1 of a
    network does; seeds defaults to the device RNG state's seed + r.  priors: default each net's own.  state: the ``state`` of
    an earlier result continues it (its Philox states replace seeds / offset; epochs, lr and restarts count from this call's
    first epoch).  A step whose loss or one of whose probabilities is not finite changes nothing and is counted.

    Everything returned is on the device; the call reads nothing back to the host."""
    def check(net):
        _check_net(net)
        return ()
    return _fit(nets, check, x, y, epochs, batch_size, lambda R, E, dev: _lr_table(lr, R, E, dev), restarts, betas, eps,
                weight_decay, seeds, offset, priors, epochs_per_launch, state,
                row_width=lambda key, O, I: 3 * O * I + 2 * O,
                launch=lambda key, **kw: ops.lrt_study_fit(**kw),
                unpack_rows=lambda key, packed, O, I: unpack(packed, O, I))


def _check_mnf_net(net):
    if not isinstance(net, MNFBayesianNetwork):
        raise NotImplementedError("bnn_amd.study: fit_mnf_replicates takes mnf.BayesianNetwork (one planar-MNF layer, sigmoid "
                                  "head), got %s; LRT networks go through fit_replicates, baseline and VD networks are trained "
                                  "one by one with graphs.make_graphed_train_step" % type(net).__name__)
    if len(net.dims) != 2:
        raise ValueError("bnn_amd.study: a replicate has one layer, got dims=%s; train deeper networks one by one with "
                         "graphs.make_graphed_train_step" % (net.dims,))
    if net.head != "sigmoid":
        raise ValueError('bnn_amd.study: a replicate has head="sigmoid", got %r; use graphs.make_graphed_train_step' % net.head)
    kinds = (net.l1.z_flow.kind, net.l1.r_flow.kind)
    if kinds != ("Planar", "Planar"):
        raise NotImplementedError("bnn_amd.study: MNF replicates have planar flows (z_flow_type = r_flow_type = \"Planar\"), got "
                                  "%s / %s; train networks with other flows one by one with graphs.make_graphed_train_step" % kinds)
    Tz, Tr = len(net.l1.z_flow.transforms), len(net.l1.r_flow.transforms)
    if Tz > _lib.STUDY_MAX_TRANSFORMS or Tr > _lib.STUDY_MAX_TRANSFORMS:
        raise ValueError("bnn_amd.study: a replicate's flows have at most %d transforms each, got %d and %d; train longer flows "
                         "one by one with graphs.make_graphed_train_step" % (_lib.STUDY_MAX_TRANSFORMS, Tz, Tr))
    return (Tz, Tr)


def make_mnf_replicates(R: int, dims, num_transforms: int = 2, seeds: Optional[Sequence[int]] = None, priors=None,
                        lambdal_init=(1.5, 2.5), device=None):
    """R networks ``mnf.BayesianNetwork(dims, num_transforms, z_flow_type="Planar", r_flow_type="Planar", head="sigmoid",
    priors=priors[r], lambdal_init=...)``, replicate r built after ``torch.manual_seed(seeds[r])`` (default seeds 0 .. R - 1):
    the values of the network a user builds by hand from that seed."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 2:
        raise ValueError("bnn_amd.study: a replicate has one layer (dims = (I, O)), got dims=%s; train deeper networks one by "
                         "one with graphs.make_graphed_train_step" % (dims,))
    num_transforms = int(num_transforms)
    if not 0 <= num_transforms <= _lib.STUDY_MAX_TRANSFORMS:
        raise ValueError("bnn_amd.study: a replicate's flows have 0 to %d transforms, got %d; train longer flows one by one "
                         "with graphs.make_graphed_train_step" % (_lib.STUDY_MAX_TRANSFORMS, num_transforms))
    seeds = list(range(R)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != R:
        raise ValueError("bnn_amd.study: %d seeds for %d replicates" % (len(seeds), R))
    plist = list(priors) if isinstance(priors, (list, tuple)) else [priors] * R
    if len(plist) != R:
        raise ValueError("bnn_amd.study: %d priors for %d replicates" % (len(plist), R))
    nets = []
    for r in range(R):
        torch.manual_seed(seeds[r])
        net = MNFBayesianNetwork(dims, num_transforms, z_flow_type="Planar", r_flow_type="Planar", head="sigmoid",
                                 priors=plist[r], lambdal_init=lambdal_init)
        nets.append(net.to(device) if device is not None else net)
    return nets


def fit_mnf_replicates(nets, x, y, epochs: int, batch_size: int, lr=0.01, lr_z_flow=None, lr_r_flow=None, restarts=(),
                       betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, seeds=None, offset: int = 0, priors=None,
                       epochs_per_launch: Optional[int] = None, state: Optional[StudyState] = None) -> StudyResult:
    """``fit_replicates`` for R planar-MNF networks (``make_mnf_replicates``, or hand-built ``mnf.BayesianNetwork((I, O), T,
    z_flow_type="Planar", r_flow_type="Planar", head="sigmoid")`` of equal dims and transform counts, at most 4 per flow): the
    loop of LBBNN-GP-MF-MNFsim_study.py:305-395 in one launch per ``epochs_per_launch`` epochs.

    lr / lr_z_flow / lr_r_flow: the rates of the ten named tensors, of the z_flow and of the r_flow parameters (the script's
    three Adam groups); each one rate, a sequence of ``epochs`` rates, or a device tensor (epochs,) / (R, epochs); None: ``lr``.
    Every other argument is ``fit_replicates``'.  Replicate r draws eps_z, eps_z2, eps_act and eps_out of its step t from
    Philox state {seeds[r], offset + t} as layer l1 of the network does.  ``params`` of the result carries every name, the flow
    parameters as ``z_flow.<t>.u`` / ``.w`` / ``.b`` and ``r_flow.<t>...``; the rows of ``state.exp_avg`` / ``exp_avg_sq`` are as
    wide as a packed row (``unpack_mnf`` gives the named views).  The trained values, flows included, are copied back into
    ``nets[r]``: ``freeze``, ``evaluate_batches``, ``structure_posterior`` and ``explain`` go on from there."""
    def table(R, E, dev):
        cols = [_lr_table(lr if v is None else v, R, E, dev) for v in (lr, lr_z_flow, lr_r_flow)]
        if any(c.dim() == 2 for c in cols):
            cols = [c if c.dim() == 2 else c.unsqueeze(0).expand(R, E) for c in cols]
        return torch.stack(cols, dim=-1).contiguous()                   # (epochs, 3) or (R, epochs, 3)
    return _fit(nets, _check_mnf_net, x, y, epochs, batch_size, table, restarts, betas, eps, weight_decay, seeds, offset, priors,
                epochs_per_launch, state,
                row_width=lambda key, O, I: mnf_row_width(O, I, *key),
                launch=lambda key, **kw: ops.mnf_study_fit(Tz=key[0], Tr=key[1], **kw),
                unpack_rows=lambda key, packed, O, I: unpack_mnf(packed, O, I, *key))


def selection_summary(alpha, true_support, true_alpha=None) -> dict:
    """The closing numbers of the sim-study scripts (LBBNN-GP-MF-MNFsim_study.py:397-403) in torch, on ``alpha``'s device:
    ``alpha`` (R, p) inclusion probabilities, ``true_support`` (p) booleans (the non-zero true weights), ``true_alpha`` (p)
    or (R, p) the probabilities the RMSE is taken against (default: the support as 0 / 1).
      rmse                   (p)  sqrt(mean_r (alpha - true_alpha)^2) * 100
      rmse_mean              ()   its mean over the covariates
      selected               (R, p) alpha > 0.5
      agreement_covariate    (p)  share of the replicates whose selection of the covariate agrees with the support
      agreement_replicate    (R)  share of the covariates on which the replicate agrees
      true_positive_rate     ()   selected among the supported (replicate, covariate) pairs (NaN without one)
      false_positive_rate    ()   selected among the unsupported pairs (NaN without one)"""
    alpha = torch.as_tensor(alpha)
    if alpha.dim() != 2:
        raise ValueError("bnn_amd.study: alpha is (R, p), got %s" % (tuple(alpha.shape),))
    a = alpha.to(torch.float64)
    sup = torch.as_tensor(true_support, device=a.device).to(torch.bool).reshape(-1)
    if sup.numel() != a.shape[1]:
        raise ValueError("bnn_amd.study: %d covariates in alpha, %d in true_support" % (a.shape[1], sup.numel()))
    ta = sup.to(torch.float64) if true_alpha is None else torch.as_tensor(true_alpha, device=a.device).to(torch.float64)
    rmse = torch.sqrt(((a - ta) ** 2).mean(dim=0)) * 100
    sel = a > 0.5
    agree = (sel == sup).to(torch.float64)
    supf = sup.to(torch.float64).expand_as(agree)
    self64 = sel.to(torch.float64)
    return {"rmse": rmse, "rmse_mean": rmse.mean(), "selected": sel,
            "agreement_covariate": agree.mean(dim=0), "agreement_replicate": agree.mean(dim=1),
            "true_positive_rate": (self64 * supf).sum() / supf.sum(),
            "false_positive_rate": (self64 * (1 - supf)).sum() / (1 - supf).sum()}
