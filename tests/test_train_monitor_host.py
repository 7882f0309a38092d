"""CPU tier of the training monitor: the three new entry points are exported, bound and check their arguments
before launching; the host-side refusals of TrainMonitor, elbo_loss(monitor=...) and set_guard; the numpy reference on a case
worked out by hand."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import train_monitor_ref as ref

NEW = ("lbbnn_elbo_loss_monitor", "lbbnn_adam_step_groups_guarded", "lbbnn_sgd_step_groups_guarded")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_new_symbols_are_exported_and_bound(lib):
    from bnn_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.argtypes[-1] is ctypes.c_void_p
    assert lib.lbbnn_abi_version() == 1
    # the layout the header names, mirrored by the Python side
    assert _lib.MONITOR_COUNT_NAMES.index("skipped_steps") == _lib.MONITOR_SKIPPED_STEPS == 6
    assert len(_lib.MONITOR_COUNT_NAMES) == _lib.MONITOR_COUNTS and len(_lib.MONITOR_SUM_NAMES) == _lib.MONITOR_SUMS
    assert _lib.MONITOR_COUNT_NAMES == ref.COUNT_NAMES


def test_loss_monitor_argument_checks_return_codes_without_launching(lib):
    fake = ctypes.c_void_p(4096)     # never dereferenced: every call fails before launching
    s = ctypes.c_float(0.1)
    f = lib.lbbnn_elbo_loss_monitor
    assert f(None, 10, fake, 4, 10, None, s, fake, fake, None, None) == -1
    assert f(fake, 10, None, 4, 10, None, s, fake, fake, None, None) == -1
    assert f(fake, 10, fake, 4, 10, None, s, None, fake, None, None) == -1
    assert f(fake, 10, fake, 4, 10, None, s, fake, None, fake, None) == -1          # totals are not optional
    assert f(fake, 10, fake, 0, 10, None, s, fake, fake, None, None) == -2
    assert f(fake, 10, fake, 4, 0, None, s, fake, fake, None, None) == -2
    assert f(fake, 65, fake, 4, 65, None, s, fake, fake, None, None) == -2           # more than 64 classes
    assert f(fake, 9, fake, 4, 10, None, s, fake, fake, None, None) == -2            # ldp < C


@pytest.mark.parametrize("name", NEW[1:])
def test_guarded_step_argument_checks_return_codes_without_launching(lib, name):
    from bnn_amd import _lib
    fake = ctypes.c_void_p(4096)
    f = getattr(lib, name)
    lst = _lib.AdamGroupList()
    lst.n = 0
    assert f(ctypes.byref(lst), fake, fake, 1, None, fake, 1, None, None, None) == -1      # no guard: the unguarded entry's case
    assert f(ctypes.byref(lst), fake, fake, 1, None, fake, 1, None, fake, None) == -1
    assert f(None, fake, fake, 1, None, fake, 1, fake, None, None) == -1
    assert f(ctypes.byref(lst), None, fake, 1, None, fake, 1, fake, None, None) == -1
    assert f(ctypes.byref(lst), fake, None, 1, None, fake, 1, fake, None, None) == -1
    assert f(ctypes.byref(lst), fake, fake, 1, None, None, 1, fake, None, None) == -1      # advance without a ticket
    assert f(ctypes.byref(lst), fake, fake, 0, None, fake, 1, fake, None, None) == -2
    assert f(ctypes.byref(lst), fake, fake, 65537, None, fake, 1, fake, None, None) == -2
    lst.n = _lib.ADAM_GROUPS_MAX_TENSORS + 1
    assert f(ctypes.byref(lst), fake, fake, 1, None, fake, 1, fake, None, None) == -2
    lst.n = 1
    assert f(ctypes.byref(lst), fake, fake, 1, None, fake, 1, fake, None, None) == -1      # the tensor's pointers are NULL
    lst.p[0] = lst.g[0] = lst.m[0] = lst.v[0] = 4096
    lst.numel[0] = 0
    assert f(ctypes.byref(lst), fake, fake, 1, None, fake, 1, fake, None, None) == -2
    lst.numel[0], lst.group[0] = 8, 1
    assert f(ctypes.byref(lst), fake, fake, 1, None, fake, 1, fake, None, None) == -2      # group outside [0, n_groups)
    lst.n = 0
    assert f(ctypes.byref(lst), fake, fake, 1, None, None, 0, fake, None, None) == 0       # nothing to update, nothing to advance


def test_train_monitor_constructor_and_holder_behaviour():
    import copy
    import bnn_amd
    for bad in (0, -1, 65, 1000):
        with pytest.raises(ValueError, match="1 to 64 classes"):
            bnn_amd.TrainMonitor(bad, "cpu")
    for ok in (1, 10, 64):
        assert bnn_amd.TrainMonitor(ok, "cpu").classes == ok
    mon = bnn_amd.TrainMonitor(10, "cpu")
    assert mon.device == torch.device("cpu")
    r = mon.result()
    assert all(r[k] == 0 for k in ref.COUNT_NAMES) and r["loss_sum"] == 0.0
    assert all(math.isnan(r[k]) for k in ("nll_mean", "loss_mean", "accuracy"))
    mon._totals[3] = 2                                        # bad_targets
    with pytest.raises(IndexError):
        mon.result()
    assert mon.result(strict=False)["bad_targets"] == 2
    twin = copy.deepcopy(mon)                                 # a copy owns its buffers
    assert twin._totals.data_ptr() != mon._totals.data_ptr() and twin._guard.data_ptr() != mon._guard.data_ptr()
    assert torch.equal(twin._totals, mon._totals)
    mon.reset()
    assert int(mon._totals.abs().sum()) == 0 and int(twin._totals[3]) == 2
    assert mon._apply(lambda t: t.clone()) is mon and mon.to("cpu") is mon


def test_elbo_loss_with_a_monitor_refuses_what_the_fused_path_cannot_take():
    import bnn_amd
    mon = bnn_amd.TrainMonitor(10, "cpu")
    lp = torch.log_softmax(torch.randn(4, 10), dim=1)
    t = torch.tensor([0, 1, 2, 3])
    with pytest.raises(ValueError, match="log_probs is on cpu"):
        bnn_amd.elbo_loss(lp, t, monitor=mon)
    with pytest.raises(ValueError, match="7 classes, the monitor was built for 10"):
        bnn_amd.elbo_loss(lp[:, :7], t, monitor=mon)
    with pytest.raises(ValueError, match="must be a bnn_amd.TrainMonitor"):
        bnn_amd.elbo_loss(lp, t, monitor=object())
    with pytest.raises(ValueError, match="float32"):
        bnn_amd.elbo_loss(lp.double(), t, monitor=mon)
    # the target guard holds without a monitor too, and the plain CPU expression is unchanged
    with pytest.raises(ValueError, match="3 element"):
        bnn_amd.elbo_loss(lp, t[:3])
    assert torch.equal(bnn_amd.elbo_loss(lp, t), torch.nn.functional.nll_loss(lp, t, reduction="sum"))


@pytest.mark.parametrize("cls", ["Adam", "SGD"])
def test_set_guard_takes_a_monitor_or_none(cls):
    import bnn_amd
    opt = getattr(bnn_amd.optim, cls)([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    mon = bnn_amd.TrainMonitor(10, "cpu")
    before = opt.state_dict()
    opt.set_guard(mon)
    assert opt.__dict__["_guard"] is mon
    assert opt.state_dict() == before                         # not part of the checkpoint
    opt.set_guard(None)
    assert opt.__dict__["_guard"] is None
    for bad in (1, "monitor", torch.zeros(1, dtype=torch.int32), object()):
        with pytest.raises(TypeError):
            opt.set_guard(bad)
    assert opt.__dict__["_guard"] is None


def test_reference_agrees_with_a_hand_computed_case():
    """3 rows, 3 classes.  Row 0: target 1, arg-max 1 (correct), term 0.5.  Row 1: a tie at the maximum -> index 0, target 2
    (wrong), term 2.0.  Row 2: target 7 is outside [0, 3): no term, not in `correct`; its NaN makes the row non-finite."""
    lp = np.array([[-1.0, -0.5, -3.0], [-0.25, -0.25, -2.0], [-1.0, np.nan, -1.0]], dtype=np.float32)
    s = ref.step(lp, [1, 2, 7], kl=3.0, kl_scale=0.5)
    assert (s["rows"], s["valid"], s["bad_targets"], s["correct"], s["nonfinite_rows"]) == (3, 2, 1, 1, 1)
    assert s["nll"] == 2.5 and s["kl_term"] == 1.5 and s["loss"] == 4.0 and s["finite"] and s["abs_terms"] == 2.5
    bad = ref.step(lp, [1, 2, 1])                             # the NaN is now a term: the loss is not finite
    assert not bad["finite"] and bad["correct"] == 2 and bad["bad_targets"] == 0      # (a NaN is row 2's arg-max)
    tot = ref.totals([s, bad, s], skipped_steps=1)
    assert [tot[k] for k in ref.COUNT_NAMES] == [3, 9, 4, 2, 3, 1, 1, 4]
    assert (tot["nll_sum"], tot["kl_term_sum"], tot["loss_sum"]) == (5.0, 3.0, 8.0)
    assert (tot["last_nll"], tot["last_loss"]) == (2.5, 4.0)
    assert tot["nll_mean"] == 1.25 and tot["loss_mean"] == 4.0 and tot["accuracy"] == 4 / 7
    assert tot["loss_sum_abs"] == 8.0
