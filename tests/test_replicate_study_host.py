"""CPU tier of the replicate study (bnn_amd.study, lbbnn_lrt_study_fit): the analytic gradients of the float64 restatement
tests/replicate_study_ref.py against torch.autograd on the same expressions, ``selection_summary`` against a table computed by
hand, ``make_replicates`` against hand-built networks, every refusal, and the C entry's argument codes (nothing is launched)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import replicate_study_ref as ref


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def _case(I, O, B, seed, bad_target=False):
    g = torch.Generator().manual_seed(seed)
    P = {"weight_mu": torch.empty(O, I).uniform_(-0.2, 0.2, generator=g), "weight_rho": torch.empty(O, I).uniform_(-5, -4, generator=g),
         "lambdal": torch.empty(O, I).uniform_(1.5, 2.5, generator=g), "bias_mu": torch.empty(O).uniform_(-0.2, 0.2, generator=g),
         "bias_rho": torch.empty(O).uniform_(-5, -4, generator=g)}
    x = torch.randn(B, I, generator=g, dtype=torch.float64)
    y = (torch.rand(B, O, generator=g) < 0.5).to(torch.float64)
    if bad_target:
        y[0, 0] = 1.5
    eps = torch.randn(B, O, generator=g, dtype=torch.float64)
    return ref.f64(P), x, y, eps


@pytest.mark.parametrize("I,O,B,bad", [(1, 1, 1, False), (20, 1, 400, False), (33, 3, 7, True), (64, 16, 65, False)])
def test_analytic_gradients_equal_autograd_on_the_same_expressions(I, O, B, bad):
    """Pins the hand-written backward before any GPU is involved: float64 against float64, so the bar is rounding alone."""
    P, x, y, eps = _case(I, O, B, 7 + I, bad)
    pri = ref.priors_dict(dict(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_mu_prior=-0.05, bias_sigma_prior=1.7))
    kl_scale = 0.2
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    nll, kl, _, _ = ref.loss_terms(Pg, x, y, eps, pri, kl_scale)
    (nll + kl * kl_scale).backward()
    got = ref.analytic_grads(P, x, y, eps, pri, kl_scale)
    for name in ref.NAMES:
        want = Pg[name].grad
        err = float((got[name] - want).abs().max() / want.abs().max())
        assert err < 1e-11, (name, err)


def test_restatement_guard_restart_and_history():
    """The restatement's own bookkeeping on a case small enough to follow: a NaN row makes its batch's steps skipped and
    counted, a restart zeroes moments and counter, the offset advances on every step."""
    P, x, y, _ = _case(5, 1, 7, 3)
    x = x.to(torch.float32)
    x[4, 2] = float("nan")                                      # rows 3..5 are batch 1 of 3 (batch = 3, N = 7)
    out = ref.fit({k: v.to(torch.float32) for k, v in P.items()}, x, y, epochs=2, batch=3, lr=[0.01, 0.02], restarts=(1,), seed=5, offset=9)
    assert out["finite"] == [True, False, True, True, False, True]
    assert out["skipped"] == 2 and out["step"] == 2 and out["offset"] == 9 + 6          # the counter restarted at epoch 1
    assert list(out["history"][:, 5]) == [1.0, 1.0]
    assert all(torch.isfinite(v).all() for v in out["params"].values())
    assert out["grads"][1] is None and out["grads"][0] is not None


def test_selection_summary_against_a_hand_computed_table(bnn):
    alpha = torch.tensor([[0.9, 0.2, 0.6], [0.7, 0.6, 0.4]])
    s = bnn.study.selection_summary(alpha, [True, False, True], true_alpha=[1.0, 0.3, 0.5])
    # per covariate sqrt(mean((alpha - true)^2)) * 100: (0.1, 0.3) -> sqrt(0.05); (-0.1, 0.3) -> sqrt(0.05); (0.1, -0.1) -> 0.1
    want = torch.tensor([np.sqrt(0.05) * 100, np.sqrt(0.05) * 100, 10.0], dtype=torch.float64)
    assert torch.allclose(s["rmse"], want, rtol=1e-6)
    assert abs(float(s["rmse_mean"]) - float(want.mean())) < 1e-5
    assert s["selected"].tolist() == [[True, False, True], [True, True, False]]
    assert s["agreement_covariate"].tolist() == [1.0, 0.5, 0.5]
    assert torch.allclose(s["agreement_replicate"], torch.tensor([1.0, 1 / 3], dtype=torch.float64))
    assert float(s["true_positive_rate"]) == 0.75 and float(s["false_positive_rate"]) == 0.5
    s0 = bnn.study.selection_summary(alpha, [True, False, True])            # default: the support as 0 / 1
    want0 = torch.sqrt(((alpha.double() - torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)) ** 2).mean(0)) * 100
    assert torch.allclose(s0["rmse"], want0)
    with pytest.raises(ValueError):
        bnn.study.selection_summary(alpha, [True, False])


def test_make_replicates_reproduces_hand_built_networks(bnn):
    pri = bnn.Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
    nets = bnn.study.make_replicates(3, (20, 1), seeds=[4, 0, 11], priors=pri)
    for net, seed in zip(nets, [4, 0, 11]):
        torch.manual_seed(seed)
        twin = bnn.lrt.BayesianNetwork((20, 1), head="sigmoid", priors=pri, lambdal_init=(1.5, 2.5))
        for (n1, p1), (n2, p2) in zip(net.named_parameters(), twin.named_parameters()):
            assert n1 == n2 and torch.equal(p1, p2), n1
        assert net.head == "sigmoid" and net.l1.priors is pri
    assert float(nets[0].l1.lambdal.detach().min()) >= 1.5
    default = bnn.study.make_replicates(2, (4, 2))                   # seeds 0, 1
    torch.manual_seed(1)
    twin = bnn.lrt.BayesianNetwork((4, 2), head="sigmoid", lambdal_init=(1.5, 2.5))
    assert torch.equal(default[1].l1.weight_mu, twin.l1.weight_mu)
    with pytest.raises(ValueError):
        bnn.study.make_replicates(2, (4, 3, 1))
    with pytest.raises(ValueError):
        bnn.study.make_replicates(2, (4, 1), seeds=[1])


def test_refusals_name_what_to_use(bnn):
    study = bnn.study
    x, y = torch.zeros(10, 4), torch.zeros(10, 1)
    ok = study.make_replicates(2, (4, 1))
    for net in (bnn.mnf.BayesianNetwork((4, 1), 2, z_flow_type="Planar", r_flow_type="Planar", head="sigmoid"),
                bnn.base.BayesianNetwork((4, 1), head="sigmoid"), bnn.vd.BNN((4, 1))):
        with pytest.raises(NotImplementedError, match="make_graphed_train_step"):
            study.fit_replicates([net], x, y, 1, 5)
    with pytest.raises(ValueError, match="one layer"):
        study.fit_replicates([bnn.lrt.BayesianNetwork((4, 3, 1), head="sigmoid")], x, y, 1, 5)
    with pytest.raises(ValueError, match="sigmoid"):
        study.fit_replicates([bnn.lrt.BayesianNetwork((4, 1))], x, y, 1, 5)
    with pytest.raises(ValueError, match="differ in dims"):
        study.fit_replicates([ok[0], bnn.lrt.BayesianNetwork((5, 1), head="sigmoid")], x, y, 1, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        study.fit_replicates(ok, x, y, 1, 5)                          # CPU tensors
    with pytest.raises(ValueError):
        study.fit_replicates([], x, y, 1, 5)
    # shapes outside the kernel's limits, by name
    for I, O, B, N, R in ((257, 1, 8, 8, 1), (128, 16, 8, 8, 1), (4, 17, 8, 8, 1), (4, 1, 4097, 8, 1), (4, 1, 0, 8, 1), (4, 1, 8, 0, 1),
                          (4, 1, 8, 8, 65536), (0, 1, 8, 8, 1)):
        with pytest.raises(ValueError):
            study.check_shapes(I, O, B, N, R)
    study.check_shapes(256, 4, 4096, 1, 65535)
    study.check_shapes(64, 16, 1, 1, 1)


_PTRS = ("params", "exp_avg", "exp_avg_sq", "step", "rng", "skipped", "x", "y", "priors", "hyper", "lr", "history")


def _args(_lib, **change):
    a = _lib.StudyArgs()
    for n in _PTRS:
        setattr(a, n, 4096)
    a.R, a.I, a.O, a.N, a.batch, a.epochs, a.first_epoch, a.n_epochs = 3, 20, 1, 100, 40, 4, 0, 0     # n_epochs = 0: no launch
    for k, v in change.items():
        setattr(a, k, v)
    return a


def test_c_entry_argument_codes_without_a_launch(lib):
    from bnn_amd import _lib
    call = lambda **ch: lib.lbbnn_lrt_study_fit(ctypes.byref(_args(_lib, **ch)), None)
    assert lib.lbbnn_lrt_study_fit(None, None) == -1
    assert call() == 0                                                   # valid, zero epochs: a successful no-op
    for n in _PTRS:
        assert call(**{n: None}) == -1, n
    assert call(n_restarts=2) == -1 and call(n_restarts=2, restarts=4096) == 0
    for ch in (dict(I=0), dict(I=257), dict(O=0), dict(O=17), dict(I=128, O=16), dict(batch=0), dict(batch=4097), dict(N=0),
               dict(R=0), dict(R=65536), dict(n_epochs=-1), dict(first_epoch=-1), dict(first_epoch=3, n_epochs=2), dict(epochs=0),
               dict(n_restarts=-1), dict(x_rstride=100), dict(y_rstride=99), dict(priors_rstride=2), dict(lr_rstride=3)):
        assert call(**ch) == -2, ch
    assert call(I=256, O=4, batch=4096, R=65535, x_rstride=100 * 256, y_rstride=400, priors_rstride=1, lr_rstride=4) == 0
    for n in _PTRS:
        assert call(**{n: 4098}) == -3, n
    assert call(rng=4100) == -3 and call(history=4100) == -3 and call(skipped=4100) == -3      # 8-byte words
    assert call(params=None, I=0) == -1                                  # NULL comes before the shapes
    assert call(I=0, x=4098) == -2                                       # ... and the shapes before the alignment


def test_study_args_layout_matches_the_header(tmp_path):
    """lbbnn_study_args_t as gcc lays it out from the header against its ctypes mirror: size and the offset of every member."""
    import subprocess
    from bnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [n for n, _ in _lib.StudyArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\nprintf("%%zu\\n", sizeof(lbbnn_study_args_t));\n%s\nreturn 0; }\n'
                   % (os.path.join(root, "include", "lbbnn.h"),
                      "\n".join('printf("%%zu\\n", offsetof(lbbnn_study_args_t, %s));' % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.StudyArgs)
    assert out[1:] == [getattr(_lib.StudyArgs, n).offset for n in names]
