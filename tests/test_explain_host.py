"""CPU tier of evaluate.explain: the numpy restatement (tests/explain_ref.py) against torch autograd on an fp64 ReLU chain, the
argument checks of the new entry points (nothing is launched), the accumulator's arithmetic on hand-made totals, every refusal,
and the seeds of the GPU tier's networks (few hidden units near 0 in fp64)."""
import ctypes

import numpy as np
import pytest
import torch

import explain_ref as er


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


@pytest.fixture(scope="module")
def lib():
    from bnn_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dims,B,seed", [((5, 1), 4, 0), ((6, 7, 3), 5, 1), ((4, 9, 5, 6, 2), 3, 2)],
                         ids=["5-1", "6-7-3", "4-9-5-6-2"])
def test_restatement_equals_autograd_jacobian(dims, B, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(dims) - 1
    Ws = [torch.randn(dims[i + 1], dims[i], generator=g, dtype=torch.float64) * (torch.rand(dims[i + 1], dims[i], generator=g) < 0.6)
          for i in range(n)]
    bs = [torch.randn(dims[i + 1], generator=g, dtype=torch.float64) for i in range(n)]
    x = torch.randn(B, dims[0], generator=g, dtype=torch.float64)

    def chain(v):
        h = v
        for i in range(n):
            h = h @ Ws[i].T + bs[i]
            if i < n - 1:
                h = torch.relu(h)
        return h

    masks, pre = er.relu_masks([w.numpy() for w in Ws], [b.numpy() for b in bs], x.numpy())
    assert len(masks) == n - 1 and all(m.shape == (B, dims[i + 1]) for i, m in enumerate(masks))
    ref = er.explain_ref([w.numpy() for w in Ws], [b.numpy() for b in bs], x.numpy(), masks)
    logits = chain(x).numpy()
    for b in range(B):
        J = torch.autograd.functional.jacobian(chain, x[b]).numpy()               # (C, I)
        np.testing.assert_allclose(ref["J"][b], J, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(ref["contributions"][b], J * x[b].numpy()[None, :], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(ref["intercept"][b], logits[b] - J @ x[b].numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref["logits"], logits, rtol=1e-12, atol=1e-13)
    resid = ref["logits"] - (ref["contributions"].sum(-1) + ref["intercept"])
    assert np.abs(resid).max() < 1e-12 * max(1.0, np.abs(ref["contributions"]).max())


def test_depth_one_is_the_weights_and_the_bias():
    W, b = np.array([[1.0, -2.0, 0.0]]), np.array([0.5])
    x = np.array([[1.0, 1.0, 7.0], [2.0, 0.0, -1.0]])
    ref = er.explain_ref([W], [b], x, [])
    assert np.array_equal(ref["contributions"], (W * x)[:, None, :]) and np.array_equal(ref["intercept"], [[0.5], [0.5]])


@pytest.mark.parametrize("name", [k for k, v in er.CASES.items() if v[2] == "lrt" and len(v[0]) > 2])
def test_gpu_tier_seeds_keep_the_fp64_masks_decided(bnn, name):
    """The GPU tier leaves units with |a| < 1e-4 max|a| out of its mask comparison and allows 1 % of them: the fp64 reference
    alone must stay inside that cap (the median probability model of the case's network, built here from its seed)."""
    net, x = er.build_net(bnn, name)
    Ws, bs = er.mpm_operands(net)
    _, pre = er.relu_masks(Ws, bs, x.numpy())
    assert er.near_zero_share(pre) <= er.NEAR_ZERO_CAP / 2, er.near_zero_share(pre)


# ------------------------------------------------------------------------------------------------ the C entry points
_F = 4096            # never dereferenced
_ODD = 4098


def _step(bnn, **kw):
    from bnn_amd import _lib
    base = dict(mode=_lib.EXPLAIN_MASK, B=4, C=2, width=8, g=_F, ldg=8, w=None, ldw=0, w_rows=0, targets=None, h=_F, ldh=8,
                bias=_F, bias_out=None, intercept=_F, active=_F, ld_active=1, mask_out=None, ldm=0, logits=None, ldl=0, map=None,
                full_width=0, contributions=None, ldc=0, residual=None)
    base.update(kw)
    a = _lib.ExplainStepArgs()
    for k, v in base.items():
        setattr(a, k, v)
    return a


def test_explain_step_argument_checks(bnn, lib):
    from bnn_amd import _lib
    call = lambda **kw: lib.lbbnn_explain_step(ctypes.byref(_step(bnn, **kw)), None)
    seed = dict(mode=_lib.EXPLAIN_SEED, w=_F, ldw=32, w_rows=2, bias_out=_F)
    fin = dict(mode=_lib.EXPLAIN_FINISH, bias=None, active=None, logits=_F, ldl=2, w_rows=2, contributions=_F, ldc=8, full_width=8,
               residual=_F)
    assert lib.lbbnn_explain_step(None, None) == -1
    # NULL: what every mode reads, then what the mode needs
    assert call(h=None) == -1 and call(intercept=None) == -1
    assert call(g=None) == -1 and call(bias=None) == -1 and call(active=None) == -1
    assert call(**dict(seed, w=None)) == -1 and call(**dict(seed, bias_out=None)) == -1
    for k in ("logits", "contributions", "residual"):
        assert call(**dict(fin, **{k: None})) == -1, k
    assert call(**dict(fin, g=None)) == -1                                     # one layer: needs w and bias_out
    # shapes (a NULL comes first)
    assert call(mode=3) == -2 and call(mode=-1) == -2
    assert call(width=0) == -2 and call(C=0) == -2 and call(C=17) == -2 and call(B=-1) == -2
    assert call(B=(1 << 24) // 2 + 1) == -2                                    # B * C > 2^24
    assert call(ldh=7) == -2 and call(ldg=7) == -2 and call(ld_active=0) == -2
    assert call(mask_out=_F, ldm=7) == -2
    assert call(**dict(seed, ldw=7)) == -2 and call(**dict(seed, w_rows=0)) == -2
    assert call(**dict(seed, w_rows=1)) == -2                                  # C = 2 rows of a 1-row operand
    assert call(**dict(seed, targets=_F)) == -2                                # targets explain ONE output per row
    assert call(**dict(fin, ldl=1)) == -2 and call(**dict(fin, ldc=7)) == -2 and call(**dict(fin, full_width=9)) == -2
    assert call(**dict(fin, map=_F, full_width=7)) == -2
    # alignment (after the shapes)
    assert call(g=_ODD) == -3 and call(h=_ODD) == -3 and call(bias=_ODD) == -3 and call(active=_ODD) == -3
    assert call(**dict(seed, C=1, targets=4100)) == -3                         # int64 targets off 8 B
    assert call(g=_ODD, ldg=7) == -2
    # an empty batch is valid and launches nothing
    assert call(B=0) == 0 and call(**dict(fin, B=0)) == 0 and call(**dict(seed, B=0)) == 0


def test_explain_totals_and_operand_argument_checks(lib):
    f = ctypes.c_void_p(_F)
    tot = lambda **kw: lib.lbbnn_explain_totals(*dict(dict(c=f, ldc=8, t=None, B=4, C=2, I=8, s=f, a=f, r=f, w=f), **kw).values(), None)
    for k in ("c", "s", "a", "r", "w"):
        assert tot(**{k: None}) == -1, k
    assert tot(B=-1) == -2 and tot(C=0) == -2 and tot(C=17) == -2 and tot(I=0) == -2 and tot(ldc=7) == -2
    assert tot(B=(1 << 24) // 2 + 1) == -2
    assert tot(t=f, B=(1 << 24) // 2 + 1, c=None) == -1                        # with targets B alone counts; NULL comes first
    assert tot(c=ctypes.c_void_p(_ODD)) == -3 and tot(s=ctypes.c_void_p(4100)) == -3 and tot(t=ctypes.c_void_p(4100)) == -3
    assert tot(B=0) == 0
    # work: [blocks][2][C][I] doubles + [blocks][C] counts; 64 rows per block until 256 blocks, then more rows per block
    wb = lib.lbbnn_explain_work_bytes
    assert wb(1, 1, 1) == 16 + 8 and wb(64, 2, 8) == 2 * 2 * 8 * 8 + 2 * 8 and wb(65, 2, 8) == 2 * (2 * 2 * 8 * 8 + 2 * 8)
    assert wb(64 * 256, 3, 5) == 256 * (2 * 3 * 5 * 8 + 3 * 8) and wb(64 * 256 + 1, 3, 5) == 253 * (2 * 3 * 5 * 8 + 3 * 8)
    assert wb(0, 2, 8) == 0 and wb(4, 17, 8) == 0 and wb(4, 2, 0) == 0 and wb((1 << 24) + 1, 1, 1) == 0
    assert all(wb(b, 4, 20) <= wb(b + 1, 4, 20) for b in range(1, 200))
    op = lambda **kw: lib.lbbnn_explain_operand(*dict(dict(op=f, O=4, I=8, ld=32, out=f), **kw).values(), None)
    assert op(op=None) == -1 and op(out=None) == -1
    assert op(O=0) == -2 and op(I=0) == -2 and op(ld=4) == -2
    assert op(ld=40) == -3 and op(op=ctypes.c_void_p(4100)) == -3 and op(out=ctypes.c_void_p(4100)) == -3


def test_step_args_layout_matches_the_header(tmp_path):
    import os
    import subprocess
    from bnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%zu\\n", '
                   'sizeof(lbbnn_explain_step_args_t), offsetof(lbbnn_explain_step_args_t, residual), '
                   'offsetof(lbbnn_explain_step_args_t, full_width)); return 0; }\n' % os.path.join(root, "include", "lbbnn.h"))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, last, fw = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(_lib.ExplainStepArgs) == size
    assert _lib.ExplainStepArgs.residual.offset == last and _lib.ExplainStepArgs.full_width.offset == fw


# ------------------------------------------------------------------------------------------------ the accumulator
def test_accumulator_result_arithmetic(bnn):
    ev = bnn.evaluate
    acc = ev.ExplanationAccumulator(3, 2, "cpu")
    assert acc.result()["rows"].tolist() == [0, 0, 0] and np.isnan(acc.result()["mean_contribution"]).all()
    total = np.array([[1.0, -2.0], [0.5, 0.25], [0.0, 0.0]])
    abs_total = np.array([[3.0, 2.0], [0.5, 0.75], [0.0, 0.0]])
    rows = np.array([4, 1, 0], dtype=np.int64)
    acc._read = lambda: np.concatenate([rows, total.reshape(-1).view(np.int64), abs_total.reshape(-1).view(np.int64)])
    res = acc.result()
    assert res["rows"].dtype == np.int64 and res["rows"].tolist() == [4, 1, 0]
    assert res["mean_contribution"].dtype == res["mean_abs_contribution"].dtype == np.float64
    assert res["mean_contribution"].shape == res["mean_abs_contribution"].shape == (3, 2)
    assert np.array_equal(res["mean_contribution"][:2], [[0.25, -0.5], [0.5, 0.25]])
    assert np.array_equal(res["mean_abs_contribution"][:2], [[0.75, 0.5], [0.5, 0.75]])
    assert np.isnan(res["mean_contribution"][2]).all() and np.isnan(res["mean_abs_contribution"][2]).all()
    assert np.array_equal(res["sum_contribution"], total) and np.array_equal(res["sum_abs_contribution"], abs_total)
    for bad in ((0, 2), (17, 2), (3, 0)):
        with pytest.raises(ValueError):
            ev.ExplanationAccumulator(bad[0], bad[1], "cpu")
    # a result of another shape is refused before anything is launched
    fake = dict(contributions=torch.zeros(2, 3, 5), logits=torch.zeros(2, 3), targets=None)
    with pytest.raises(ValueError, match="3 outputs and 2 features"):
        acc.update(fake)
    with pytest.raises(ValueError, match="accumulator on"):
        acc.update(dict(contributions=torch.zeros(2, 3, 2), logits=torch.zeros(2, 3), targets=None))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(bnn):
    ev = bnn.evaluate
    x = torch.zeros(2, 6)
    with pytest.raises(TypeError, match="freeze"):
        ev.explain(bnn.lrt.BayesianNetwork((6, 4, 2)), x)                      # an unfrozen network
    with pytest.raises(TypeError, match="freeze"):
        ev.explain(bnn.mnf.BayesianNetwork((8, 4, 2), 2, z_flow_type="Planar", r_flow_type="Planar"), x)
    with pytest.raises(TypeError, match="variational-dropout"):
        ev.explain(bnn.vd.BNN(), x)
    with pytest.raises(TypeError, match="baseline"):
        ev.explain(bnn.base.BayesianNetwork((6, 4, 2)), x)
    with pytest.raises(TypeError, match="baseline"):
        ev.explain(ev.FrozenBaseNetwork((6, 4, 2), device="cpu"), x)
    with pytest.raises(TypeError, match="FrozenNetwork"):
        ev.explain(torch.nn.Linear(6, 2), x)
    with pytest.raises(ValueError, match="dense=True"):
        ev.explain(ev.FrozenNetwork((8, 4, 2), "mnf", flows="dense", device="cpu"), x)
    fz = ev.FrozenNetwork((6, 4, 2), "lrt", device="cpu")
    with pytest.raises(ValueError, match=r"data.to\(device\)"):
        ev.explain(fz, x)                                                      # a CPU tensor
    with pytest.raises(TypeError, match="device tensor"):
        ev.explain(fz, x.numpy())
    with pytest.raises(ValueError, match="split the batch"):
        ev._check_explain_rows((1 << 24) // 10 + 1, 10)
    ev._check_explain_rows((1 << 24) // 16, 16)
    with pytest.raises(ValueError, match="\"all\" or \"pred\""):
        ev.explain_batches(fz, [], targets="true")
    with pytest.raises(TypeError, match="freeze"):
        ev.explain_batches(bnn.lrt.BayesianNetwork((6, 4, 2)), [])
