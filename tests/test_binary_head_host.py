"""CPU tier of the binary (sigmoid) head: the restatement tests/binary_head_ref.py against torch on the saturation vector,
``elbo_bce_loss`` on CPU tensors, its guards, the argument checks of the four entry points (nothing is launched) and the
construction keywords ``head=`` / ``lambdal_init=``."""
import ctypes
import os

import pytest
import torch

import binary_head_ref as ref


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


def _bits(t):
    return t.detach().to(torch.float32).contiguous().view(torch.int32)


def _torch_autograd():
    """torch.sigmoid + nn.BCELoss(reduction='sum') autograd in fp32 on the saturation vector: p, terms, g_probs, g_logits."""
    x = ref.SATURATION.clone().requires_grad_(True)
    y = ref.SATURATION_TARGETS
    p = torch.sigmoid(x)
    p.retain_grad()
    torch.nn.BCELoss(reduction="sum")(p, y).backward()
    terms = torch.nn.BCELoss(reduction="none")(p.detach(), y)
    return p.detach(), terms, p.grad, x.grad


# ------------------------------------------------------------------------------------------- the formulas are torch's
def test_reference_equals_torch_on_the_saturation_vector():
    p, terms, g_probs, g_logits = _torch_autograd()
    y = ref.SATURATION_TARGETS
    f32 = torch.float32
    # the sigmoid of the header, 1 / (1 + exp(-x)), against torch.sigmoid: the same value to one float32 rounding
    ps = ref.sigmoid(ref.SATURATION, f32)
    assert float((ps - p).abs().max()) <= 2.0 ** -24 and float(ps[0]) == 0.0 and float(ps[-1]) == 1.0
    assert torch.equal(_bits(ref.bce_terms(p, y, f32)), _bits(terms))                      # bitwise
    gp, gl, gk = ref.backward(1.0, p, y, 0.2, f32)
    assert torch.equal(_bits(gp), _bits(g_probs))                                          # bitwise
    assert float((gl - g_logits).abs().max()) <= 1e-8
    assert float(gk) == float(torch.tensor(0.2, dtype=f32))
    # the clamps: p == 1.0f from x = 17 on, a term of exactly 100 against y = 0, a g_probs of 1e12, a logit gradient of exactly 0
    sat = (ref.SATURATION >= 17) & (y == 0)
    assert bool(sat.any()) and bool((p[ref.SATURATION >= 17] == 1).all())
    assert bool((terms[sat] == 100).all()) and bool((gl[sat] == 0).all())
    assert float(gp[sat].max()) == float(torch.tensor(1.0, dtype=f32) / torch.tensor(1e-12, dtype=f32))
    # sigmoid_backward of g_probs is the g_logits of the fused backward, bit for bit
    assert torch.equal(_bits(ref.sigmoid_backward(gp, p, f32)), _bits(gl))


def test_float32_reference_stays_inside_the_gpu_bars_of_its_float64_form():
    """The bars of tests/test_binary_head_gpu.py are stated against the float64 form: the float32 form of the SAME restatement
    (CPU libm) stays inside each of them on the inputs those tests use, so the bars are not asking for more than fp32 gives."""
    g = torch.Generator().manual_seed(0)
    x = torch.cat([ref.SATURATION.repeat(69)[:1031] + 3.0 * torch.randn(1031, generator=g), ref.SATURATION])
    p64, p32 = ref.sigmoid(x), ref.sigmoid(x, torch.float32)
    assert bool(((p32.double() - p64).abs() <= 1e-6 * p64 + 1e-37).all())
    l64, l32 = ref.logp2(x), ref.logp2(x, torch.float32)
    assert bool(torch.isfinite(l32).all()) and bool(((l32.double() - l64).abs() <= 1e-6 * l64.abs() + 1e-37).all())
    y = (torch.arange(x.numel()) % 2).float()
    t64, t32 = ref.bce_terms(p32, y), ref.bce_terms(p32, y, torch.float32)
    assert abs(float(t32.double().sum()) - float(t64.sum())) <= 2e-6 * float(t64.abs().sum())
    for a, b in zip(ref.backward(1.0, p32, y, 0.2, torch.float32)[:2], ref.backward(1.0, p32, y, 0.2)[:2]):
        assert bool(((a.double() - b).abs() <= 1e-6 * b.abs() + 1e-30).all())


# ------------------------------------------------------------------------------------------- elbo_bce_loss on CPU tensors
@pytest.mark.parametrize("with_kl", (False, True))
@pytest.mark.parametrize("shape", ((15, 1), (5, 3)))
def test_elbo_bce_loss_on_cpu_tensors_is_the_torch_expression(bnn, with_kl, shape):
    g = torch.Generator().manual_seed(1)
    x = ref.SATURATION.repeat(2)[:shape[0] * shape[1]].reshape(shape) * 0.2 + torch.randn(shape, generator=g)
    y = (torch.rand(shape, generator=g) > 0.5).float()
    grads = []
    for fn in ("ours", "torch"):
        xv = x.clone().requires_grad_(True)
        kl = torch.tensor(3.5, requires_grad=True) if with_kl else None
        p = torch.sigmoid(xv)
        if fn == "ours":
            loss = bnn.elbo_bce_loss(p, y, kl, 5)
        else:
            loss = torch.nn.BCELoss(reduction="sum")(p, y)
            loss = loss + kl / 5 if with_kl else loss
        loss.backward()
        grads.append((loss.detach(), xv.grad, kl.grad if with_kl else None))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    if with_kl:
        assert torch.equal(grads[0][2], grads[1][2])
    if shape[1] == 1:                                           # (B,) targets against (B, 1) probabilities
        assert torch.equal(bnn.elbo_bce_loss(torch.sigmoid(x), y.reshape(-1)), torch.nn.BCELoss(reduction="sum")(torch.sigmoid(x), y))
    st = torch.zeros(4, dtype=torch.int32)
    bnn.elbo_bce_loss(torch.sigmoid(x), y, stats=st)
    bnn.elbo_bce_loss(torch.sigmoid(x), y, stats=st)
    assert st.tolist() == [2 * v for v in ref.stats(torch.sigmoid(x), y)]


def test_elbo_bce_loss_guards_raise_before_the_library_is_reached(bnn, monkeypatch):
    from bnn_amd import _lib

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.full((4, 1), 0.5)
    with pytest.raises(ValueError, match="shape"):
        bnn.elbo_bce_loss(p, torch.zeros(3, 1))
    with pytest.raises(ValueError, match="shape"):
        bnn.elbo_bce_loss(torch.full((4, 2), 0.5), torch.zeros(4))             # (B,) stands for (B, 1) only
    with pytest.raises(ValueError, match="float32"):
        bnn.elbo_bce_loss(p, torch.zeros(4, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="meta"):
        bnn.elbo_bce_loss(p, torch.zeros(4, 1, device="meta"))                  # a target on another device
    with pytest.raises(ValueError, match="contiguous"):
        bnn.elbo_bce_loss(p, torch.zeros(4, 2)[:, :1])
    with pytest.raises(ValueError, match="stats"):
        bnn.elbo_bce_loss(p, torch.zeros(4, 1), stats=torch.zeros(4))


# ------------------------------------------------------------------------------------------- the C entry points
def test_argument_checks_return_codes_without_launching(lib):
    fake, f = ctypes.c_void_p(4096), ctypes.c_float(0.2)
    odd = ctypes.c_void_p(4098)
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    head = lib.lbbnn_binary_head
    assert head(None, 1, 4, 1, fake, 1, None, 2, None) == E_NULL
    assert head(fake, 1, 4, 1, None, 1, None, 2, None) == E_NULL                 # neither output
    assert head(fake, 1, -1, 1, fake, 1, None, 2, None) == E_SHAPE
    assert head(fake, 1, 4, 0, fake, 1, None, 2, None) == E_SHAPE
    assert head(fake, 17, 4, 17, fake, 17, None, 2, None) == E_SHAPE
    assert head(fake, 2, 4, 3, fake, 3, None, 2, None) == E_SHAPE                # ldi < O
    assert head(fake, 3, 4, 3, fake, 2, None, 2, None) == E_SHAPE                # ldp < O
    assert head(fake, 3, 4, 3, fake, 3, fake, 2, None) == E_SHAPE                # logp2 with O != 1
    assert head(fake, 1, 4, 1, None, 0, fake, 1, None) == E_SHAPE                # ld2 < 2
    assert head(fake, 1, 4, 1, odd, 1, None, 2, None) == E_ALIGN
    assert head(fake, 1, 0, 1, fake, 1, fake, 2, None) == 0                      # an empty batch: a successful no-op
    loss = lib.lbbnn_elbo_bce_loss
    assert loss(None, 1, fake, 1, 4, 1, None, f, fake, None, 0, None) == E_NULL
    assert loss(fake, 1, None, 1, 4, 1, None, f, fake, None, 0, None) == E_NULL
    assert loss(fake, 1, fake, 1, 4, 1, None, f, None, None, 0, None) == E_NULL
    assert loss(fake, 1, fake, 1, -1, 1, None, f, fake, None, 0, None) == E_SHAPE
    assert loss(fake, 1, fake, 1, 4, 0, None, f, fake, None, 0, None) == E_SHAPE
    assert loss(fake, 17, fake, 17, 4, 17, None, f, fake, None, 0, None) == E_SHAPE
    assert loss(fake, 3, fake, 2, 4, 3, None, f, fake, None, 0, None) == E_SHAPE  # ldt < O
    assert loss(fake, 1, fake, 1, 4, 1, None, f, fake, odd, 0, None) == E_ALIGN
    bwd = lib.lbbnn_elbo_bce_loss_backward
    assert bwd(None, fake, 1, fake, 1, 4, 1, f, fake, None, None, None) == E_NULL
    assert bwd(fake, None, 1, fake, 1, 4, 1, f, fake, None, None, None) == E_NULL
    assert bwd(fake, fake, 1, None, 1, 4, 1, f, fake, None, None, None) == E_NULL
    assert bwd(fake, fake, 1, fake, 1, 4, 1, f, None, fake, None, None) == E_NULL
    assert bwd(fake, fake, 1, fake, 1, -1, 1, f, fake, None, None, None) == E_SHAPE
    assert bwd(fake, fake, 1, fake, 1, 4, 0, f, fake, None, None, None) == E_SHAPE
    assert bwd(fake, fake, 17, fake, 17, 4, 17, f, fake, None, None, None) == E_SHAPE
    assert bwd(fake, fake, 2, fake, 3, 4, 3, f, fake, None, None, None) == E_SHAPE
    sb = lib.lbbnn_sigmoid_backward
    assert sb(None, 1, fake, 1, fake, 1, 4, 1, None) == E_NULL
    assert sb(fake, 1, None, 1, fake, 1, 4, 1, None) == E_NULL
    assert sb(fake, 1, fake, 1, None, 1, 4, 1, None) == E_NULL
    assert sb(fake, 1, fake, 1, fake, 1, -1, 1, None) == E_SHAPE
    assert sb(fake, 1, fake, 1, fake, 1, 4, 0, None) == E_SHAPE
    assert sb(fake, 17, fake, 17, fake, 17, 4, 17, None) == E_SHAPE
    assert sb(fake, 3, fake, 3, fake, 2, 4, 3, None) == E_SHAPE
    assert sb(fake, 1, fake, 1, fake, 1, 0, 1, None) == 0


# ------------------------------------------------------------------------------------------- construction
def _nets(bnn, seed, **kw):
    torch.manual_seed(seed)
    a = bnn.lrt.BayesianNetwork((20, 8, 1), **kw)
    torch.manual_seed(seed)
    b = bnn.mnf.BayesianNetwork((20, 8, 1), 2, z_flow_type="Planar", r_flow_type="Planar", **kw)
    return a, b


def test_head_keyword_changes_neither_the_state_dict_nor_the_seeded_values(bnn):
    for plain, sig in zip(_nets(bnn, 3), _nets(bnn, 3, head="sigmoid")):
        assert plain.head == "log_softmax" and sig.head == "sigmoid"
        a, b = plain.state_dict(), sig.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_lambdal_init_draws_inside_its_range_and_moves_nothing_else(bnn):
    for plain, wide in zip(_nets(bnn, 4), _nets(bnn, 4, lambdal_init=(1.5, 2.5))):
        a, b = plain.state_dict(), wide.state_dict()
        assert list(a) == list(b)
        for k in a:
            if k.endswith("lambdal"):
                assert float(b[k].min()) >= 1.5 and float(b[k].max()) <= 2.5 and not torch.equal(a[k], b[k])
                assert float(a[k].min()) >= 0.0 and float(a[k].max()) <= 1.0
            else:
                assert torch.equal(a[k], b[k]), k
    torch.manual_seed(4)
    l = bnn.lrt.BayesianLinear(20, 1, lambdal_init=(1.5, 2.5))
    assert 1.5 <= float(l.lambdal.detach().min()) and float(l.lambdal.detach().max()) <= 2.5
    alphas = wide.inclusion_probabilities()
    assert [tuple(a.shape) for a in alphas] == [(8, 20), (1, 8)] and not alphas[0].requires_grad
    assert torch.equal(alphas[0], torch.sigmoid(wide.l1.lambdal.detach()))


def test_head_keyword_refusals(bnn):
    with pytest.raises(ValueError, match="16"):
        bnn.lrt.BayesianNetwork((20, 17), head="sigmoid")
    with pytest.raises(ValueError, match="16"):
        bnn.mnf.BayesianNetwork((20, 17), 2, head="sigmoid")
    with pytest.raises(ValueError, match="softmax"):
        bnn.lrt.BayesianNetwork((20, 1), head="softmax")
    with pytest.raises(ValueError, match="softmax"):
        bnn.mnf.BayesianNetwork((20, 1), 2, head="softmax")
    assert bnn.lrt.BayesianNetwork((20, 17)).head == "log_softmax"            # the default head takes any width, as before
    with pytest.raises(NotImplementedError, match="sigmoid"):
        bnn.parallel.DataParallelELBO(bnn.lrt.BayesianNetwork((20, 1), head="sigmoid"))
    with pytest.raises(ValueError, match="sigmoid"):
        bnn.evaluate.FrozenNetwork((20, 17), "lrt", head="sigmoid")
    assert bnn.evaluate.FrozenNetwork((20, 1), "lrt", head="sigmoid").head == "sigmoid"
