"""CPU tier for the baseline layer's in-kernel draws (sample_elbo(draws="hip")): the new C structs match the header, the new
entry points are exported and bound, their argument checks return the documented codes without launching, and the Python
interface rejects what it cannot run."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lbbnn_gate_sample_draw", "lbbnn_gate_backward_draw", "lbbnn_philox_uniform", "lbbnn_philox_std_gamma", "lbbnn_gamma_grad")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_draw_struct_layouts_match_the_header(tmp_path):
    from bnn_amd import _lib
    pairs = [("lbbnn_gate_draw_args_t", _lib.GateDrawArgs, ("g", "lambdal", "tau_b", "temperature")),
             ("lbbnn_gate_bwd_draw_args_t", _lib.GateBwdDrawArgs, ("g", "lambdal", "d_lambdal", "temperature")),
             ("lbbnn_gate_args_t", _lib.GateArgs, ("mu", "log_q", "flags", "layer_id")),
             ("lbbnn_gate_bwd_args_t", _lib.GateBwdArgs, ("mu", "rows", "exact", "layer_id"))]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"),
             "int main(void) {"]
    for cname, _, fields in pairs:
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in fields:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["return 0; }"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = {}
    for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        c, f, v = l.split()
        got[(c, f)] = int(v)
    for cname, cls, fields in pairs:
        assert ctypes.sizeof(cls) == got[(cname, "size")], cname
        for f in fields:
            assert getattr(cls, f).offset == got[(cname, f)], (cname, f)


def test_new_symbols_exported_and_bound(lib):
    from bnn_amd import _lib
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n


def test_stream_ids_match_the_header():
    from bnn_amd import ops
    src = open(os.path.join(ROOT, "include", "lbbnn.h")).read()
    for name, val in (("GATE", ops.STREAM_GATE), ("GAMMA_W", ops.STREAM_GAMMA_W), ("GAMMA_B", ops.STREAM_GAMMA_B)):
        assert "#define LBBNN_STREAM_%s %d" % (name, val) in src, name
    # distinct from every other kind of draw
    assert len({ops.STREAM_EPS_OUT, ops.STREAM_EPS_Z, ops.STREAM_EPS_ACT, ops.STREAM_EPS_W, ops.STREAM_EPS_B, ops.STREAM_MASK,
                ops.STREAM_ROW_MASK, ops.STREAM_GATE, ops.STREAM_GAMMA_W, ops.STREAM_GAMMA_B}) == 10


def _filled_draw_args(_lib, fake):
    a = _lib.GateDrawArgs()
    g = a.g
    for n in ("mu", "rho", "bias_mu", "bias_rho", "bias_a", "bias_b", "weight_a", "weight_b", "pa", "pb", "w_out", "bias_out",
              "rows", "log_prior", "log_q"):
        setattr(g, n, fake)
    a.lambdal = a.gammas = a.alpha = a.tau_w = a.tau_b = fake
    g.O, g.I, g.ld, g.mode, g.want_lp = 4, 4, 32, 0, 1
    a.temperature = 0.5
    return a


def _filled_bwd_draw_args(_lib, fake):
    a = _lib.GateBwdDrawArgs()
    g = a.g
    for n in ("mu", "rho", "bias_mu", "bias_rho", "bias_a", "bias_b", "tau_b", "weight_a", "weight_b", "tau_w", "pa", "pb",
              "d_mu", "d_rho", "d_bias_mu", "d_bias_rho", "d_bias_a", "d_bias_b", "d_scalars", "rows"):
        setattr(g, n, fake)
    a.lambdal = a.d_lambdal = fake
    g.O, g.I = 4, 4
    a.temperature = 0.5
    return a


def test_draw_entry_points_argument_checks(lib):
    """Every case fails before a launch (the fake pointers are never dereferenced)."""
    from bnn_amd import _lib
    fake = 4096
    rng = ctypes.c_void_p(fake)
    assert lib.lbbnn_gate_sample_draw(None, rng, None) == -1
    a = _filled_draw_args(_lib, fake)
    a.lambdal = None
    assert lib.lbbnn_gate_sample_draw(ctypes.byref(a), rng, None) == -1
    a = _filled_draw_args(_lib, fake)
    a.tau_b = None
    assert lib.lbbnn_gate_sample_draw(ctypes.byref(a), rng, None) == -1
    for O, I in ((0, 4), (4, 0), (-1, 4)):
        a = _filled_draw_args(_lib, fake)
        a.g.O, a.g.I = O, I
        assert lib.lbbnn_gate_sample_draw(ctypes.byref(a), rng, None) == -2, (O, I)
    a = _filled_draw_args(_lib, fake)
    a.g.mode = 1                                   # only the sampled training forward draws
    assert lib.lbbnn_gate_sample_draw(ctypes.byref(a), rng, None) == -4
    a = _filled_draw_args(_lib, fake)
    a.temperature = 0.0
    assert lib.lbbnn_gate_sample_draw(ctypes.byref(a), rng, None) == -4
    a = _filled_draw_args(_lib, fake)
    a.g.ld = 30
    assert lib.lbbnn_gate_sample_draw(ctypes.byref(a), rng, None) == -3
    a = _filled_draw_args(_lib, fake)
    assert lib.lbbnn_gate_sample_draw(ctypes.byref(a), None, None) == -5     # the draws need the Philox state

    assert lib.lbbnn_gate_backward_draw(None, rng, None) == -1
    b = _filled_bwd_draw_args(_lib, fake)
    b.d_lambdal = None
    assert lib.lbbnn_gate_backward_draw(ctypes.byref(b), rng, None) == -1
    b = _filled_bwd_draw_args(_lib, fake)
    b.g.tau_w = None
    assert lib.lbbnn_gate_backward_draw(ctypes.byref(b), rng, None) == -1
    for O, I in ((0, 4), (4, 0)):
        b = _filled_bwd_draw_args(_lib, fake)
        b.g.O, b.g.I = O, I
        assert lib.lbbnn_gate_backward_draw(ctypes.byref(b), rng, None) == -2, (O, I)
    b = _filled_bwd_draw_args(_lib, fake)
    assert lib.lbbnn_gate_backward_draw(ctypes.byref(b), None, None) == -5

    f = ctypes.c_void_p(fake)
    assert lib.lbbnn_philox_uniform(None, 0, 0, 4, 4, f, None) == -1
    assert lib.lbbnn_philox_uniform(f, 0, 0, 4, 4, None, None) == -1
    assert lib.lbbnn_philox_uniform(f, 0, 0, 0, 4, f, None) == -2
    assert lib.lbbnn_philox_uniform(f, 0, 0, 4, 0, f, None) == -2
    assert lib.lbbnn_philox_std_gamma(None, 0, f, None, 4, f, None) == -1
    assert lib.lbbnn_philox_std_gamma(f, 0, None, None, 4, f, None) == -1
    assert lib.lbbnn_philox_std_gamma(f, 0, f, None, 0, f, None) == -2
    assert lib.lbbnn_gamma_grad(None, f, 4, f, None) == -1
    assert lib.lbbnn_gamma_grad(f, f, 4, None, None) == -1
    assert lib.lbbnn_gamma_grad(f, f, 0, f, None) == -2


def test_sample_elbo_rejects_unknown_draws():
    import bnn_amd
    net = bnn_amd.base.BayesianNetwork((784, 8, 6, 10))
    x, y = torch.rand(2, 1, 28, 28), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError):
        net.sample_elbo(x, y, draws="bogus")
    with pytest.raises(ValueError):
        net.sample_elbo(x, y, 1, num_batches=600, draws=None)


def test_hip_draws_need_a_device_tensor():
    import bnn_amd
    net = bnn_amd.base.BayesianNetwork((784, 8, 6, 10))
    x, y = torch.rand(2, 1, 28, 28), torch.zeros(2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="HIP device"):
        net.sample_elbo(x, y, draws="hip")
    with pytest.raises(RuntimeError, match="HIP device"):
        net.l1.sample_forward(x.view(2, -1))


@pytest.mark.parametrize("T", [0.5, 0.001])
def test_relaxed_reference_is_torch_relaxed_bernoulli(T):
    """tests/base_draw_ref._relaxed, the gate reference of every GPU draw test, against torch's own
    RelaxedBernoulli(probs, T).rsample() on the same torch.rand uniforms (reseeded): the values in fp32 (the same operations:
    equal), and in fp64 the values and the autograd gradient with respect to lambdal wherever the fp32 clamp constants of the
    reference do not bite (fp64 torch clamps at the fp64 constants)."""
    from base_draw_ref import _relaxed, gate_clamp_classes
    lam = torch.empty(20000, dtype=torch.float64).uniform_(-8, 8, generator=torch.Generator().manual_seed(1))
    RB = torch.distributions.RelaxedBernoulli
    # fp32
    p32 = torch.sigmoid(lam.float())
    torch.manual_seed(5)
    u32 = torch.rand(p32.shape, dtype=torch.float32)
    torch.manual_seed(5)
    ref32 = RB(probs=p32, temperature=torch.tensor(T)).rsample()
    assert torch.equal(_relaxed(p32, u32, T), ref32)
    # fp64 with autograd through alpha = sigmoid(lambdal)
    l1 = lam.clone().requires_grad_(True)
    l2 = lam.clone().requires_grad_(True)
    torch.manual_seed(6)
    u64 = torch.rand(lam.shape, dtype=torch.float64)
    mine = _relaxed(torch.sigmoid(l1), u64, T)
    torch.manual_seed(6)
    theirs = RB(probs=torch.sigmoid(l2), temperature=torch.tensor(T, dtype=torch.float64)).rsample()
    w = torch.randn(lam.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    (mine * w).sum().backward()
    (theirs * w).sum().backward()
    inside, outside = gate_clamp_classes(torch.sigmoid(lam), u64, T)
    assert int(inside.sum()) > 100
    assert torch.allclose(mine[inside], theirs[inside], rtol=1e-12, atol=0)
    assert torch.allclose(l1.grad[inside], l2.grad[inside], rtol=1e-9, atol=0)
    # outside the fp32 clamps the reference's gate is a clamp constant with no gradient
    assert (l1.grad[outside] == 0).all()
    assert ((mine[outside] == torch.finfo(torch.float32).tiny) | (mine[outside] == 1 - torch.finfo(torch.float32).eps)).all()
