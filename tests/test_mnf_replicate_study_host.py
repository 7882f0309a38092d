"""CPU tier of the MNF replicate study (bnn_amd.study.fit_mnf_replicates, lbbnn_mnf_study_fit): the float64 restatement
tests/mnf_replicate_study_ref.py against oracle.mnf_forward + BCE on the same noise, ``make_mnf_replicates`` against hand-built
networks, the packed row against ``_param_list``, every refusal, the C entry's argument codes (nothing is launched) and the
ctypes mirror of the argument struct against the header."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mnf_replicate_study_ref as ref
from oracle import lbbnn_oracle as orc


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


PRI = dict(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_mu_prior=-0.05, bias_sigma_prior=1.7)


def _case(bnn, I, O, B, T, seed, acting):
    net = bnn.study.make_mnf_replicates(1, (I, O), num_transforms=T, seeds=[seed])[0]
    P = ref.net_params(net)
    if acting:
        P = ref.acting(P, seed, 3)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, I, generator=g, dtype=torch.float64)
    y = (torch.rand(B, O, generator=g) < 0.5).to(torch.float64)
    return ref.f64(P), x, y, ref.draws(seed, 3, B, I, O)


@pytest.mark.parametrize("I,O,B,T,acting", [(1, 1, 1, 1, True), (20, 1, 40, 2, False), (20, 1, 40, 2, True), (33, 3, 7, 3, True)])
def test_restatement_loss_is_the_oracle_forward_plus_bce(bnn, I, O, B, T, acting):
    P, x, y, noise = _case(bnn, I, O, B, T, 5 + I, acting)
    pri = ref.priors_dict(PRI)
    nll, kl, p = ref.loss_terms(P, x, y, noise, pri)
    sd = {k: P[k] for k in ref.BASE_NAMES}
    for fl in ("z_flow", "r_flow"):
        for t in range(T):
            for short, attr in (("u", "u"), ("w", "w"), ("b", "bias")):
                sd["%s.transforms.%d.%s" % (fl, t, attr)] = P["%s.%d.%s" % (fl, t, short)]
    act, kl_o, inter = orc.mnf_forward(x, sd, orc.flow_from_state("z_flow", "Planar", sd, T), orc.flow_from_state("r_flow", "Planar", sd, T),
                                       noise, priors=orc.Priors(**pri))
    want_nll = torch.nn.functional.binary_cross_entropy(torch.sigmoid(act), y, reduction="sum")
    assert abs(float(nll) - float(want_nll)) <= 1e-12 * abs(float(want_nll))
    assert abs(float(kl) - float(kl_o)) <= 1e-12 * abs(float(kl_o))
    assert torch.allclose(p, torch.sigmoid(act), rtol=1e-13, atol=0)
    if acting:                                                           # the flows act: their log-dets are a visible share of the KL
        assert abs(float(inter["log_det_q"])) > 1e-2 and abs(float(inter["log_det_r"])) > 1e-2
    g = ref.gradients(P, x, y, noise, pri, 0.2)
    assert set(g) == set(ref.names(T, T)) and all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in g.values())


def test_restatement_guard_restart_groups_and_history(bnn):
    P, x, y, _ = _case(bnn, 5, 1, 7, 2, 3, True)
    x = x.to(torch.float32)
    x[4, 2] = float("nan")                                      # rows 3..5 are batch 1 of 3 (batch = 3, N = 7)
    P32 = {k: v.to(torch.float32) for k, v in P.items()}
    lr = [[0.01, 0.0, 0.02], [0.02, 0.0, 0.01]]
    out = ref.fit(P32, x, y, epochs=2, batch=3, lr=lr, restarts=(1,), seed=5, offset=9)
    assert out["finite"] == [True, False, True, True, False, True]
    assert out["skipped"] == 2 and out["step"] == 2 and out["offset"] == 9 + 6
    assert list(out["history"][:, 5]) == [1.0, 1.0]
    assert all(torch.isfinite(v).all() for v in out["params"].values())
    for n in ref.names(2, 2):                                   # the rate of group 1 is zero: z_flow stays, the others move
        moved = not torch.equal(out["params"][n], P32[n].double())
        assert moved == (ref.group_of(n) != 1), n


def test_make_mnf_replicates_reproduces_hand_built_networks(bnn):
    pri = bnn.Priors(mu_prior=0.1, sigma_prior=1.3, alpha_prior=0.3, bias_sigma_prior=1.3)
    nets = bnn.study.make_mnf_replicates(3, (20, 1), num_transforms=3, seeds=[4, 0, 11], priors=pri)
    for net, seed in zip(nets, [4, 0, 11]):
        torch.manual_seed(seed)
        twin = bnn.mnf.BayesianNetwork((20, 1), 3, z_flow_type="Planar", r_flow_type="Planar", head="sigmoid", priors=pri,
                                       lambdal_init=(1.5, 2.5))
        pairs = list(zip(net.named_parameters(), twin.named_parameters()))
        assert len(pairs) == 10 + 2 * 3 * 3
        for (n1, p1), (n2, p2) in pairs:
            assert n1 == n2 and torch.equal(p1, p2), n1
        assert net.head == "sigmoid" and net.l1.priors is pri and net.l1.z_flow.kind == net.l1.r_flow.kind == "Planar"
    default = bnn.study.make_mnf_replicates(2, (4, 2))               # seeds 0, 1; two transforms
    torch.manual_seed(1)
    twin = bnn.mnf.BayesianNetwork((4, 2), 2, z_flow_type="Planar", r_flow_type="Planar", head="sigmoid", lambdal_init=(1.5, 2.5))
    assert torch.equal(default[1].l1.r_flow.transforms[1].w, twin.l1.r_flow.transforms[1].w)
    assert len(bnn.study.make_mnf_replicates(1, (4, 1), num_transforms=0)[0].l1.z_flow.transforms) == 0
    for bad in (dict(dims=(4, 3, 1)), dict(dims=(4, 1), seeds=[1]), dict(dims=(4, 1), num_transforms=5)):
        with pytest.raises(ValueError):
            bnn.study.make_mnf_replicates(2, **bad)


def test_packed_row_is_in_param_list_order(bnn):
    study = bnn.study
    I, O, T = 7, 3, 2
    nets = study.make_mnf_replicates(2, (I, O), num_transforms=T)
    rows = torch.stack([torch.cat([t.detach().reshape(-1) for _, t in study._named_tensors(n)]) for n in nets])
    want = torch.stack([torch.cat([p.detach().reshape(-1) for p in n.l1._param_list()]) for n in nets])
    assert torch.equal(rows, want) and rows.shape[1] == study.mnf_row_width(O, I, T, T) == 3 * O * I + 2 * O + 5 * I + 2 * T * (2 * I + 1)
    named = study.unpack_mnf(rows, O, I, T, T)
    assert list(named) == ref.names(T, T)
    for r, n in enumerate(nets):
        got = ref.net_params(n)
        for name in ref.names(T, T):
            assert torch.equal(named[name][r].reshape(-1), got[name].reshape(-1)), name
        assert torch.equal(ref.pack(got), rows[r])
    assert named["weight_mu"].shape == (2, O, I) and named["z_flow.1.b"].shape == (2, 1) and named["r0_b2"].shape == (2, I)
    named["r_flow.1.w"][1, 3] = 7.0                                   # views, not copies
    assert float(rows[1, -2 - (I - 1 - 3)]) == 7.0
    with pytest.raises(ValueError):
        study.unpack_mnf(rows, O, I, T, T + 1)


def test_refusals_name_what_to_use(bnn):
    study = bnn.study
    x, y = torch.zeros(10, 4), torch.zeros(10, 1)
    mk = lambda dims=(4, 1), T=2, **kw: bnn.mnf.BayesianNetwork(dims, T, **dict(dict(z_flow_type="Planar", r_flow_type="Planar",
                                                                                     head="sigmoid"), **kw))
    ok = study.make_mnf_replicates(2, (4, 1))
    for net in (bnn.lrt.BayesianNetwork((4, 1), head="sigmoid"), bnn.base.BayesianNetwork((4, 1), head="sigmoid"), bnn.vd.BNN((4, 1))):
        with pytest.raises(NotImplementedError, match="make_graphed_train_step"):
            study.fit_mnf_replicates([net], x, y, 1, 5)
    with pytest.raises(NotImplementedError, match="fit_replicates"):
        study.fit_mnf_replicates([bnn.lrt.BayesianNetwork((4, 1), head="sigmoid")], x, y, 1, 5)
    for kw in (dict(z_flow_type="RNVP"), dict(r_flow_type="RNVP"), dict(z_flow_type="RNVP", r_flow_type="RNVP")):
        with pytest.raises(NotImplementedError, match="Planar.*make_graphed_train_step"):
            study.fit_mnf_replicates([mk(**kw)], x, y, 1, 5)
    with pytest.raises(ValueError, match="at most 4 transforms.*make_graphed_train_step"):
        study.fit_mnf_replicates([mk(T=5)], x, y, 1, 5)
    with pytest.raises(ValueError, match="one layer"):
        study.fit_mnf_replicates([mk(dims=(4, 3, 1))], x, y, 1, 5)
    with pytest.raises(ValueError, match="sigmoid"):
        study.fit_mnf_replicates([mk(head="log_softmax")], x, y, 1, 5)
    with pytest.raises(ValueError, match="differ in dims"):
        study.fit_mnf_replicates([ok[0], mk(dims=(5, 1))], x, y, 1, 5)
    with pytest.raises(ValueError, match="transform counts"):
        study.fit_mnf_replicates([ok[0], mk(T=3)], x, y, 1, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        study.fit_mnf_replicates(ok, x, y, 1, 5)                      # CPU tensors
    with pytest.raises(ValueError):
        study.fit_mnf_replicates([], x, y, 1, 5)
    # fit_replicates still refuses an MNF network, and now names the call that takes it
    with pytest.raises(NotImplementedError, match="fit_mnf_replicates.*make_graphed_train_step"):
        study.fit_replicates([ok[0]], x, y, 1, 5)


_PTRS = ("params", "exp_avg", "exp_avg_sq", "step", "rng", "skipped", "x", "y", "priors", "hyper", "lr", "history")


def _args(_lib, **change):
    a = _lib.MnfStudyArgs()
    for n in _PTRS:
        setattr(a, n, 4096)
    a.R, a.I, a.O, a.N, a.batch, a.epochs, a.first_epoch, a.n_epochs = 3, 20, 1, 100, 40, 4, 0, 0     # n_epochs = 0: no launch
    a.Tz, a.Tr = 2, 2
    for k, v in change.items():
        setattr(a, k, v)
    return a


def test_c_entry_argument_codes_without_a_launch(lib):
    from bnn_amd import _lib
    call = lambda **ch: lib.lbbnn_mnf_study_fit(ctypes.byref(_args(_lib, **ch)), None)
    assert lib.lbbnn_mnf_study_fit(None, None) == -1
    assert call() == 0                                                   # valid, zero epochs: a successful no-op
    for n in _PTRS:
        assert call(**{n: None}) == -1, n
    assert call(n_restarts=2) == -1 and call(n_restarts=2, restarts=4096) == 0
    for ch in (dict(I=0), dict(I=257), dict(O=0), dict(O=17), dict(I=128, O=16), dict(batch=0), dict(batch=4097), dict(N=0),
               dict(R=0), dict(R=65536), dict(n_epochs=-1), dict(first_epoch=-1), dict(first_epoch=3, n_epochs=2), dict(epochs=0),
               dict(n_restarts=-1), dict(x_rstride=100), dict(y_rstride=99), dict(priors_rstride=2), dict(lr_rstride=3),
               dict(Tz=5), dict(Tr=5), dict(Tz=-1), dict(Tr=-1)):
        assert call(**ch) == -2, ch
    assert call(I=256, O=4, batch=4096, R=65535, x_rstride=100 * 256, y_rstride=400, priors_rstride=1, lr_rstride=4, Tz=4, Tr=0) == 0
    assert call(Tz=0, Tr=0) == 0 and call(Tz=0, Tr=4) == 0
    for n in _PTRS:
        assert call(**{n: 4098}) == -3, n
    assert call(rng=4100) == -3 and call(history=4100) == -3 and call(skipped=4100) == -3      # 8-byte words
    assert call(params=None, I=0) == -1 and call(params=None, Tz=5) == -1   # NULL comes before the shapes
    assert call(I=0, x=4098) == -2 and call(Tz=5, x=4098) == -2          # ... and the shapes before the alignment


def test_mnf_study_args_layout_matches_the_header(tmp_path):
    """lbbnn_mnf_study_args_t as gcc lays it out from the header against its ctypes mirror: size and the offset of every member."""
    import subprocess
    from bnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [n for n, _ in _lib.MnfStudyArgs._fields_]
    assert names[-2:] == ["Tz", "Tr"] and _lib.STUDY_MAX_TRANSFORMS == 4
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\nprintf("%%zu\\n", sizeof(lbbnn_mnf_study_args_t));\n'
                   'printf("%%d\\n", LBBNN_STUDY_MAX_TRANSFORMS);\n%s\nreturn 0; }\n'
                   % (os.path.join(root, "include", "lbbnn.h"),
                      "\n".join('printf("%%zu\\n", offsetof(lbbnn_mnf_study_args_t, %s));' % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.MnfStudyArgs) and out[1] == _lib.STUDY_MAX_TRANSFORMS
    assert out[2:] == [getattr(_lib.MnfStudyArgs, n).offset for n in names]


def _ops_tensors(R=2, I=4, O=1, T=2, N=6, E=3, device="cpu"):
    from bnn_amd import study
    P = study.mnf_row_width(O, I, T, T)
    f = dict(dtype=torch.float32, device=device)
    return dict(params=torch.zeros(R, P, **f), exp_avg=torch.zeros(R, P, **f), exp_avg_sq=torch.zeros(R, P, **f), step=torch.zeros(R, **f),
                rng=torch.zeros(R, 2, dtype=torch.int64, device=device), skipped=torch.zeros(R, dtype=torch.int64, device=device),
                x=torch.zeros(N, I, **f), y=torch.zeros(N, O, **f), priors=torch.ones(1, 5, **f), hyper=torch.zeros(R, 6, **f),
                lr=torch.zeros(E, 3, **f), restarts=None, history=torch.zeros(R, E, 6, dtype=torch.float64, device=device),
                I=I, O=O, Tz=T, Tr=T, batch=3, first_epoch=0, n_epochs=0)


def test_ops_wrapper_refuses_cpu_tensors_by_name(bnn):
    """ops.mnf_study_fit checks its tensors before it touches the library: there is no CPU path.  (Its shape, dtype and
    contiguity refusals need device tensors: tests/test_mnf_replicate_study_gpu.py.)"""
    with pytest.raises(RuntimeError, match="params must be a contiguous torch.float32 tensor of shape .* on a HIP device"):
        bnn.ops.mnf_study_fit(**_ops_tensors())
    with pytest.raises(TypeError):
        bnn.ops.mnf_study_fit(**{k: v for k, v in _ops_tensors().items() if k != "Tz"})
