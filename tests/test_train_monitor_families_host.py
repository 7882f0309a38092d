"""CPU tier of the training monitor for the BCE loss, the baseline family and variational dropout:
lbbnn_elbo_bce_loss_monitor is exported, bound and checks its arguments before launching; the host-side refusals of
elbo_bce_loss(monitor=...), base.sample_elbo(monitor=...) and vd.loss_fn(monitor=...); vd.kl; the numpy reference on a case
worked out by hand."""
import ctypes
import os

import numpy as np
import pytest
import torch

import train_monitor_bce_ref as ref

NAME = "lbbnn_elbo_bce_loss_monitor"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_symbol_is_exported_and_bound(lib):
    from bnn_amd import _lib
    assert NAME in _lib.SIGNATURES
    fn = getattr(lib, NAME)
    assert fn.argtypes == _lib.SIGNATURES[NAME][1] and fn.argtypes[-1] is ctypes.c_void_p
    # lbbnn_elbo_bce_loss's arguments, then totals and guard ahead of the stream
    assert fn.argtypes[:11] == _lib.SIGNATURES["lbbnn_elbo_bce_loss"][1][:11] and len(fn.argtypes) == 14
    assert ref.COUNT_NAMES == _lib.MONITOR_COUNT_NAMES


def test_argument_checks_return_codes_without_launching(lib):
    fake = ctypes.c_void_p(4096)     # never dereferenced: every call fails before launching
    s = ctypes.c_float(0.1)
    f = getattr(lib, NAME)
    #        probs ldp target ldt B  O  kl    scale loss stats acc totals guard stream
    assert f(None, 1, fake, 1, 4, 1, None, s, fake, None, 1, fake, None, None) == -1
    assert f(fake, 1, None, 1, 4, 1, None, s, fake, None, 1, fake, None, None) == -1
    assert f(fake, 1, fake, 1, 4, 1, None, s, None, None, 1, fake, None, None) == -1
    assert f(fake, 1, fake, 1, 4, 1, None, s, fake, fake, 1, None, fake, None) == -1     # totals are not optional
    assert f(fake, 1, fake, 1, 0, 1, None, s, fake, None, 1, fake, None, None) == -2     # an empty batch has no step
    assert f(fake, 1, fake, 1, -1, 1, None, s, fake, None, 1, fake, None, None) == -2
    assert f(fake, 1, fake, 1, 4, 0, None, s, fake, None, 1, fake, None, None) == -2
    assert f(fake, 17, fake, 17, 4, 17, None, s, fake, None, 1, fake, None, None) == -2  # more than 16 units
    assert f(fake, 2, fake, 3, 4, 3, None, s, fake, None, 1, fake, None, None) == -2     # ldp < O
    assert f(fake, 3, fake, 2, 4, 3, None, s, fake, None, 1, fake, None, None) == -2     # ldt < O


def test_elbo_bce_loss_with_a_monitor_refuses_what_the_fused_path_cannot_take():
    import bnn_amd
    mon = bnn_amd.TrainMonitor(3, "cpu")
    p = torch.rand(4, 3) * 0.9 + 0.05
    y = (torch.rand(4, 3) > 0.5).float()
    with pytest.raises(ValueError, match="must be a bnn_amd.TrainMonitor"):
        bnn_amd.elbo_bce_loss(p, y, monitor=object())
    with pytest.raises(ValueError, match="probs must be float32"):
        bnn_amd.elbo_bce_loss(p.double(), y, monitor=mon)
    with pytest.raises(ValueError, match="probs is on cpu"):
        bnn_amd.elbo_bce_loss(p, y, monitor=mon)
    with pytest.raises(ValueError, match="2 units, the monitor was built for 3"):
        bnn_amd.elbo_bce_loss(p[:, :2].contiguous(), y[:, :2].contiguous(), monitor=mon)
    with pytest.raises(ValueError, match="empty batch"):
        bnn_amd.elbo_bce_loss(p[:0], y[:0], monitor=mon)
    for bad_kl in (torch.tensor(1.0), torch.ones(2), 1.0):
        with pytest.raises(ValueError, match="kl must be None or a one-element float32 HIP tensor"):
            bnn_amd.elbo_bce_loss(p, y, bad_kl, monitor=mon)
    assert mon.result()["steps"] == 0
    # without a monitor the CPU expression is what it was
    want = torch.nn.functional.binary_cross_entropy(p, y, reduction="sum") + torch.tensor(3.0) / 5
    assert torch.equal(bnn_amd.elbo_bce_loss(p, y, torch.tensor(3.0), 5), want)


@pytest.mark.parametrize("head", ["log_softmax", "sigmoid"])
def test_sample_elbo_with_a_monitor_refuses_before_any_forward(head):
    import bnn_amd
    from bnn_amd import base
    torch.manual_seed(0)
    sig = head == "sigmoid"
    net = base.BayesianNetwork((8, 1), head="sigmoid") if sig else base.BayesianNetwork((12, 16, 3))
    x = torch.rand(5, net.dims[0])
    t = torch.zeros(5, 1) if sig else torch.zeros(5, dtype=torch.int64)
    mon = bnn_amd.TrainMonitor(net.dims[-1], "cpu")
    for draws in ("torch", "hip"):
        with pytest.raises(ValueError, match="samples must be 1, got 2"):
            net.sample_elbo(x, t, 2, draws=draws, monitor=mon)
        with pytest.raises(ValueError, match="must be a bnn_amd.TrainMonitor"):
            net.sample_elbo(x, t, 1, draws=draws, monitor="mon")
    with pytest.raises(ValueError, match="input is on cpu"):
        net.sample_elbo(x, t, 1, draws="torch", monitor=mon)
    with pytest.raises(TypeError):
        net.sample_elbo(x, t, 1, 600.0, "torch", None, mon)                      # keyword-only
    assert mon.result()["steps"] == 0


class _Net(torch.nn.Module):
    """A VD-shaped model on the CPU (the layers' forward needs the GPU, their parameters and alpha do not) with a child that
    is not a BayesianLayer."""

    def __init__(self):
        super().__init__()
        from bnn_amd import vd
        self.l1, self.act, self.l2 = vd.BayesianLayer(8, 6), torch.nn.ReLU(), vd.BayesianLayer(6, 3)
        with torch.no_grad():
            self.l1.alpha.copy_(torch.linspace(0.05, 0.9, 6))
            self.l2.alpha.copy_(torch.tensor([0.2, 1.7, 0.01]))


def _reference_kl(model):
    """The KL of variational_dropout.py:97-102, written out as loss_fn wrote it before vd.kl existed."""
    from bnn_amd import vd
    KL = 0
    c1, c2, c3 = 1.16145124, -1.50204118, 0.58629921
    for layer in model.children():
        if isinstance(layer, vd.BayesianLayer):
            a = layer.alpha
            KL = KL + (0.5 * torch.log(a) + c1 * a + c2 * a ** 2 + c3 * a ** 3).sum()
    return KL


def test_vd_kl_is_the_kl_of_loss_fn_and_loss_fn_is_unchanged():
    import bnn_amd
    from bnn_amd import vd
    model = _Net().eval()
    want = _reference_kl(model)
    got = vd.kl(model)
    assert got.dtype == torch.float32 and got.dim() == 0 and got.device == model.l1.alpha.device
    assert torch.equal(got, want)
    lp = torch.log_softmax(torch.randn(5, 3, generator=torch.Generator().manual_seed(1)), dim=1)
    t = torch.tensor([0, 2, 1, 1, 0])
    for nb in (None, 7.0):
        model.eval()
        loss = vd.loss_fn(lp, t, model) if nb is None else vd.loss_fn(lp, t, model, num_batches=nb)
        assert model.training                                                    # the side effect of :91 is kept
        old = want / (vd.NUM_BATCHES if nb is None else nb) + torch.nn.functional.nll_loss(lp, t, reduction="sum")
        assert torch.equal(loss, old)
    # a model without a BayesianLayer child: KL is the number 0, as a tensor
    z = vd.kl(torch.nn.Sequential(torch.nn.Linear(2, 2)))
    assert z.dtype == torch.float32 and z.dim() == 0 and float(z) == 0.0
    # a monitor needs the fused loss: CPU tensors are refused with elbo_loss's words, after the side effect
    mon = bnn_amd.TrainMonitor(3, "cpu")
    model.eval()
    with pytest.raises(ValueError, match="log_probs is on cpu"):
        vd.loss_fn(lp, t, model, monitor=mon)
    assert model.training
    with pytest.raises(ValueError, match="must be a bnn_amd.TrainMonitor"):
        vd.loss_fn(lp, t, model, monitor=3)
    assert bnn_amd.vd.kl is vd.kl


def test_reference_agrees_with_a_hand_computed_case():
    """2 rows, 2 units, probabilities whose logarithms are exact in every arithmetic (1, 0, and 0.5 against a term that is 0
    times the logarithm).  (0, 0): p = 1, y = 1 -> term 0, correct.  (0, 1): p = 0, y = 1 -> -max(log 0, -100) = 100, wrong.
    (1, 0): a target of 1.5 -> no term, not in `correct`.  (1, 1): p = NaN, y = 0 -> (0 - 1) fmax(NaN, -100) - 0 = 100: finite,
    counted as a non-finite "row", and (NaN > 0.5) == (0 > 0.5) makes it `correct`."""
    p = np.array([[1.0, 0.0], [0.5, np.nan]], dtype=np.float32)
    y = np.array([[1.0, 1.0], [1.5, 0.0]], dtype=np.float32)
    s = ref.step(p, y, kl=3.0, kl_scale=0.5)
    assert (s["rows"], s["valid"], s["bad_targets"], s["correct"], s["nonfinite_rows"]) == (4, 3, 1, 2, 1)
    assert s["nll"] == 200.0 and s["kl_term"] == 1.5 and s["loss"] == 201.5 and s["finite"] and s["abs_terms"] == 200.0
    assert s["n_terms"] == 3
    bad = ref.step(p, y, kl=float("inf"), kl_scale=0.5)
    assert not bad["finite"] and bad["nll"] == 200.0 and bad["loss"] == float("inf")
    given = ref.step(p, y, terms=np.array([[1.0, 2.0], [64.0, 4.0]], dtype=np.float32))      # the bad target's term is dropped
    assert given["nll"] == 7.0 and given["loss"] == 7.0
    tot = ref.totals([s, bad, s], skipped_steps=1)
    assert [tot[k] for k in ref.COUNT_NAMES] == [3, 12, 6, 3, 3, 1, 1, 6]
    assert (tot["nll_sum"], tot["kl_term_sum"], tot["loss_sum"]) == (400.0, 3.0, 403.0)
    assert (tot["last_nll"], tot["last_loss"]) == (200.0, 201.5)
    assert tot["nll_mean"] == 400.0 / 6 and tot["loss_mean"] == 201.5 and tot["accuracy"] == 6 / 9
