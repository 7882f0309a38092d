"""GPU tier: the kernels that finish a training step, called directly at the shapes and option branches where they can go
wrong, against float64 (tests/backward_tail_ref.py; the host tier is tests/test_backward_tail_host.py).

  1. lbbnn_head_dx            both kernels (registers: C == 10 with G_v; LDS: everything else), rows / columns around a
                              16 x 256 workgroup, strided 4-byte-aligned gradients, padded operands and x
  2. lbbnn_weight_pass_backward   O < 8, I around a 256-column workgroup, every NULL-pointer branch, the slab loop (fp64 and
                              bitwise the promised order), the W = 1 fall-back on unaligned pointers, trained-parameter ranges
  3. column sums              lbbnn_output_grad + the second level past 16 row tiles, through all three routes, and the bias
                              gradients made from them
  4. lbbnn_output_grad        gv_scale, want_g=False, row strides, the scalar path at O % 4 == 0, the ReLU boundary, in-kernel eps
  5. lbbnn_dx_combine         around the 1024 columns of one workgroup, strided x
  6. csrc/loss_head.hip       ldp > C, targets outside [0, C), C = 64, the second trips of the forward and backward loops

Every strided or padded buffer is NaN outside its logical view: a read past a bound shows in the result.  Bars are the
repository's existing ones (TIGHT 5e-6 for short fp32 sums, 2e-5 for K1b, 1e-6 / 2e-6 for the loss head) or derived bounds
(column sums: depth * 2^-24 * Sum|term|); none was set from a kernel's output.

Found by section 6 and fixed in csrc/loss_head.hip: lbbnn_elbo_loss_backward_logits took the row sum of g_logp to be -g for
every row, so a row whose target lies outside [0, C) got g_logits = g exp(logp) instead of zeros whenever the head's backward
took the handed-over gradient; the two-launch route (lbbnn_elbo_loss_backward + lbbnn_log_softmax_backward) was right.

Measured on an MI355X when this was written, one run (each test prints its figures next to its bar: pytest -s):
  section                                   cases   worst figure                                   bar
  1  head_dx (+ 2 ldo calls, 1 refusal)     80      2.5e-6 (C = 16, (1, 1), one output); 1.5e-7    5e-6
  2  K1b shapes and options / slabs /       26 / 10 4.8e-7 / 2.7e-7 (all ten bitwise the ordered   2e-5
     unaligned / wide ranges                1 / 2   sum) / 2.2e-7 / 2.7e-7
  3  sums past 16 tiles, bias gradients     8       G_v 6.5e-8; sums 0.009, d_bias_mu 0.005,       1e-6; 1 (x the
                                                    d_bias_rho 0.105 of their bounds; 1.9e-7       bound); 2e-5
  4  output_grad options                    19      G_v 7.6e-8; sums 0.020 of their bounds         1e-6; 1
  5  dx_combine                             3       3.2e-8; 777 of 3069 elements one contracted    5e-6
                                                    rounding away from the torch float32 expression
  6  loss head (+ 2 log_softmax_backward,   32      loss 6.0e-8, gradients 8.1e-8 (both routes,    1e-6
     1 network)                                     bitwise each other); C = 64: 1.3e-7            2e-6
With the library from before the fix, the 8 cases of section 6 with out-of-range targets and the network test fail."""

import pytest
import torch

import backward_tail_ref as bt
from conftest import rel_err

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL = -1234.5625


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bnn():
    import bnn_amd
    return bnn_amd


def _cols(t, off, pad, dev):
    """``t`` (B, n) as the columns [off, off + n) of a NaN-filled (B, n + pad) GPU buffer."""
    B, n = t.shape
    buf = torch.full((B, n + pad), NAN, device=dev)
    buf[:, off:off + n] = t.to(dev)
    return buf[:, off:off + n]


def _from_element_1(t, dev):
    """``t`` contiguous, but starting at element 1 of a flat NaN-headed buffer: 4-byte aligned only."""
    buf = torch.full((t.numel() + 1,), NAN, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t.to(dev))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _bits(t):
    return t.contiguous().view(torch.int32)


# =========================================================================== 1. lbbnn_head_dx
def _head_dx_tensors(ops, dev, C, B, I, layout):
    d = bt.head_dx_inputs(C, B, I)
    ld = ops.operand_ld(C)
    wmT, wvT = torch.full((I, ld), NAN, device=dev), torch.full((I, ld), NAN, device=dev)
    wmT[:, :C], wvT[:, :C] = d["wmT"].to(dev), d["wvT"].to(dev)
    if layout == "dense":
        gm, gv, x = d["gm"].to(dev), d["gv"].to(dev), d["x"].to(dev)
    else:
        pad = bt.HEAD_DX_G_LD - C
        gm, gv = _cols(d["gm"], bt.HEAD_DX_G_OFF, pad, dev), _cols(d["gv"], bt.HEAD_DX_G_OFF, pad, dev)
        x = _cols(d["x"], bt.HEAD_DX_X_OFF, bt.HEAD_DX_X_PAD, dev)
        assert gm.stride(0) == gv.stride(0) == bt.HEAD_DX_G_LD and gm.data_ptr() % 16 != 0
    return d, gm, gv, wmT, wvT, x


@pytest.mark.parametrize("C,stoch,B,I,layout", bt.HEAD_DX_CASES)
def test_head_dx_vs_fp64(bnn, dev, C, stoch, B, I, layout):
    ops = bnn.ops
    d, gm, gv, wmT, wvT, x = _head_dx_tensors(ops, dev, C, B, I, layout)
    got = ops.head_dx(gm, gv if stoch else None, wmT, wvT if stoch else None, x, C=C, I=I)
    ref = bt.head_dx_ref(d["gm"], d["gv"] if stoch else None, d["wmT"], d["wvT"], d["x"], C)
    e = rel_err(got, ref)
    print("head_dx C=%d stoch=%s (%d,%d) %s: %.2e (bar %.0e)" % (C, stoch, B, I, layout, e, bt.TIGHT))
    assert got.shape == (B, I) and torch.isfinite(got).all() and e < bt.TIGHT


@pytest.mark.parametrize("C", [10, 3])
def test_head_dx_row_stride_of_the_output_keeps_the_pad(bnn, dev, C):
    """The C entry with ldo = I + 3, once per kernel (C = 10: registers, C = 3: LDS): the pad columns keep their bits."""
    from bnn_amd import _lib
    ops = bnn.ops
    B, I = 17, 257
    d, gm, gv, wmT, wvT, x = _head_dx_tensors(ops, dev, C, B, I, "strided")
    ldo = I + bt.HEAD_DX_PAD_OUT
    out = torch.full((B, ldo), SENTINEL, device=dev)
    want = _bits(out[:, I:]).clone()
    rc = _lib.lib().lbbnn_head_dx(gm.data_ptr(), gv.data_ptr(), gm.stride(0), wmT.data_ptr(), wvT.data_ptr(), wmT.stride(0),
                                  x.data_ptr(), x.stride(0), out.data_ptr(), ldo, B, C, I, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "lbbnn_head_dx")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:, I:]), want)
    e = rel_err(out[:, :I], bt.head_dx_ref(d["gm"], d["gv"], d["wmT"], d["wvT"], d["x"], C))
    print("head_dx ldo=I+3 C=%d: %.2e (bar %.0e)" % (C, e, bt.TIGHT))
    assert e < bt.TIGHT


def test_head_dx_refuses_gradients_with_different_row_strides(bnn, dev):
    """lbbnn_head_dx has ONE row stride for G_m and G_v: the wrapper must not pass G_m's for both."""
    ops = bnn.ops
    C, B, I = 3, 5, 9
    d, gm, gv, wmT, wvT, x = _head_dx_tensors(ops, dev, C, B, I, "strided")
    gv_other = _cols(d["gv"], 0, 5, dev)
    assert gv_other.stride(0) != gm.stride(0)
    with pytest.raises(ValueError, match="row stride"):
        ops.head_dx(gm, gv_other, wmT, wvT, x, C=C, I=I)
    ops.head_dx(gm, None, wmT, None, x, C=C, I=I)                        # mean-only: nothing to compare


# =========================================================================== 2. lbbnn_weight_pass_backward
def _run_wpb(bnn, dev, d, opt):
    ops = bnn.ops
    put = (lambda t: _from_element_1(t, dev)) if opt["unaligned"] else (lambda t: t.to(dev))
    dv = lambda t: None if t is None else t.to(dev)
    return ops.weight_pass_backward(put(d["mu"]), put(d["rho"]), put(d["lam"]), put(d["dWm"]),
                                    None if d["dWv"] is None else put(d["dWv"]), z_fwd=dv(d["zf"]), z_kl=dv(d["zk"]),
                                    r0_c=dv(d["rc"]), da_mu=dv(d["dam"]), da_var=dv(d["dav"]), g_kl=dv(d["gk"]), priors=bnn.Priors())


def _check_wpb(cid, got, ref):
    worst = 0.0
    for name, a, b in zip(bt.WPB_NAMES, got, (ref[n] for n in bt.WPB_NAMES)):
        if b is None:
            assert a is None, (cid, name)                                # no such input vector
        elif float(b.abs().max()) == 0:
            assert a is None or float(a.abs().max()) == 0, (cid, name)   # the objective does not depend on it: exact zeros
        else:
            assert a is not None and torch.isfinite(a).all(), (cid, name)
            e = rel_err(a, b)
            worst = max(worst, e)
            assert e < bt.WPB_BAR, (cid, name, e)
    print("K1b %s: worst output %.2e (bar %.0e)" % (cid, worst, bt.WPB_BAR))


_WPB_PLAIN = bt.WPB_CASES + bt.WPB_UNALIGNED_CASES + bt.WPB_WIDE_CASES


@pytest.mark.parametrize("case", _WPB_PLAIN, ids=[c[0] for c in _WPB_PLAIN])
def test_weight_pass_backward_edges_vs_fp64(bnn, dev, case):
    cid, O, I, opt = case
    d = bt.wpb_inputs(O, I, opt)
    _check_wpb(cid, _run_wpb(bnn, dev, d, opt), bt.wpb_reference(d, opt, bnn.Priors()))


@pytest.mark.parametrize("case", bt.WPB_SLAB_CASES, ids=[c[0] for c in bt.WPB_SLAB_CASES])
def test_weight_pass_backward_slabs_vs_fp64_and_in_the_promised_order(bnn, dev, case):
    """(S, O, I) gradients: against fp64 of the slab sum, and bitwise the one-slab call on ((s0 + s1) + s2) + ... formed with
    float32 adds -- the fixed order of additions the kernel's comments promise (4 slabs per trip, absent slabs add +0)."""
    cid, O, I, opt = case
    d = bt.wpb_inputs(O, I, opt)
    got = _run_wpb(bnn, dev, d, opt)
    _check_wpb(cid, got, bt.wpb_reference(d, opt, bnn.Priors()))
    one = dict(d)
    for k in ("dWm", "dWv"):
        acc = d[k][0].clone()
        for s in range(1, opt["S"]):
            acc = acc + d[k][s]
        one[k] = acc
    ordered = _run_wpb(bnn, dev, one, dict(opt, S=0))
    for name, a, b in zip(bt.WPB_NAMES, got, ordered):
        assert torch.equal(_bits(a), _bits(b)), (cid, name)


# =========================================================================== 3. column sums past 16 row tiles
def _og_dev(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _check_og(tag, B, got, ref, stoch):
    gm, gv, gmT, gvT, gs, gvs = got
    assert torch.equal(gm.cpu().double(), ref["gm"]) and torch.equal(gmT, gm.t()), tag
    err = (gs.cpu().double() - gm.cpu().double().sum(0)).abs()
    bound = bt.column_sum_bound(gm.cpu(), B)
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert (err <= bound).all(), (tag, "g_sum", worst)
    if not stoch:
        assert gv is None and gvT is None and gvs is None, tag
        print("output_grad %s: g_sum at most %.3f of its bound" % (tag, worst))
        return
    e = rel_err(gv, ref["gv"])
    assert e < bt.GV_BAR and torch.equal(gvT, gv.t()), (tag, e)
    err = (gvs.cpu().double() - gv.cpu().double().sum(0)).abs()
    bound = bt.column_sum_bound(gv.cpu(), B)
    worst_v = float((err / bound.clamp_min(1e-300)).max())
    assert (err <= bound).all(), (tag, "gv_sum", worst_v)
    print("output_grad %s: gv %.2e (bar %.0e), sums at most %.3f / %.3f of their bounds" % (tag, e, bt.GV_BAR, worst, worst_v))


@pytest.mark.parametrize("B,O", bt.OG_SUM_SHAPES)
@pytest.mark.parametrize("stoch", [True, False])
def test_column_sums_past_16_row_tiles_and_the_bias_gradients(bnn, dev, B, O, stoch):
    ops = bnn.ops
    pr = bnn.Priors()
    h = bt.og_inputs(B, O)
    d = _og_dev(h, dev)
    kw = dict(out=d["out"], std=d["std"] if stoch else None, eps=d["eps"] if stoch else None, relu=True)
    got = ops.output_grad(d["g_out"], **kw)
    ref = bt.output_grad_ref(h["g_out"], h["out"], h["std"] if stoch else None, h["eps"] if stoch else None)
    _check_og("(%d,%d) stoch=%s" % (B, O, stoch), B, got, ref, stoch)
    gm, gv, _, _, gs, gvs = got
    g = torch.Generator().manual_seed(O)
    bias_mu = (0.3 + 0.1 * torch.randn(O, generator=g)).to(dev)
    bias_rho = (-3 + torch.randn(O, generator=g)).to(dev)
    # the same partials through the three routes
    jobs = []
    deferred = ops.output_grad(d["g_out"], defer_sums=jobs, **kw)
    job = dict(jobs[0])
    assert job["nblk"] == bt.og_row_tiles(B)
    for gk in (torch.full((), 0.37, device=dev), None):
        a = ops.bias_backward_partials(job, B, bias_mu, bias_rho, gk, pr)
        b = ops.bias_backward(bias_mu, bias_rho, gs, gvs, gk, pr)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
        # ... and against float64, with the sums' own bound carried through the formula
        s_m = gm.cpu().double().sum(0)
        s_v = gv.cpu().double().sum(0) if stoch else None
        r_mu, r_rho = bt.bias_ref(bias_mu.cpu(), bias_rho.cpu(), s_m, s_v, None if gk is None else gk.cpu(), pr)
        rho64 = bias_rho.cpu().double()
        sb, dsig = torch.nn.functional.softplus(rho64), torch.sigmoid(rho64)
        kl_mu = r_mu - s_m
        bound_mu = bt.column_sum_bound(gm.cpu(), B) + 16 * bt.U32 * (s_m.abs() + kl_mu.abs())
        err_mu = (a[0].cpu().double() - r_mu).abs()
        assert (err_mu <= bound_mu).all(), float((err_mu / bound_mu).max())
        if stoch:
            v_part = s_v * 2 * sb * dsig
            bound_rho = (bt.column_sum_bound(gv.cpu(), B) * 2 * sb * dsig + 16 * bt.U32 * (v_part.abs() + (r_rho - v_part).abs()))
            err_rho = (a[1].cpu().double() - r_rho).abs()
            assert (err_rho <= bound_rho).all(), float((err_rho / bound_rho).max())
            print("bias (%d,%d) kl=%s: d_mu %.3f, d_rho %.3f of their bounds" % (B, O, gk is not None, float((err_mu / bound_mu).max()),
                                                                                  float((err_rho / bound_rho).max())))
        elif gk is not None:
            e = rel_err(a[1], r_rho)
            print("bias (%d,%d) mean-only kl: d_mu %.3f of its bound, d_rho %.2e (bar %.0e)" % (B, O, float((err_mu / bound_mu).max()), e, bt.WPB_BAR))
            assert e < bt.WPB_BAR
        else:
            assert float(a[1].abs().max()) == 0                          # no variance term, no KL: bias_rho gets no gradient
    ops.reduce_partials_flush(jobs)
    assert not jobs
    torch.cuda.synchronize()
    assert torch.equal(_bits(deferred[4]), _bits(gs)) and (not stoch or torch.equal(_bits(deferred[5]), _bits(gvs)))


# =========================================================================== 4. lbbnn_output_grad: options
def _same_bits(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("B,O", bt.OG_OPTION_SHAPES)
def test_output_grad_gv_scale_and_want_g(bnn, dev, B, O):
    ops = bnn.ops
    h = bt.og_inputs(B, O)
    d = _og_dev(h, dev)
    kw = dict(out=d["out"], std=d["std"], eps=d["eps"], relu=True, gv_scale=d["gv_scale"])
    got = ops.output_grad(d["g_out"], **kw)
    _check_og("(%d,%d) gv_scale" % (B, O), B, got, bt.output_grad_ref(h["g_out"], h["out"], h["std"], h["eps"], h["gv_scale"]), True)
    for stoch in (True, False):
        kw2 = dict(kw) if stoch else dict(out=d["out"], relu=True)
        full = ops.output_grad(d["g_out"], **kw2)
        lean = ops.output_grad(d["g_out"], want_g=False, **kw2)
        assert lean[0] is None and lean[1] is None
        _same_bits(lean[2:], full[2:])


@pytest.mark.parametrize("B,O", bt.OG_OPTION_SHAPES)
@pytest.mark.parametrize("off", bt.OG_STRIDED_OFFSETS)
@pytest.mark.parametrize("stoch", [True, False])
def test_output_grad_row_strides(bnn, dev, B, O, off, stoch):
    """g_out, out and std as column views of wider NaN-filled buffers: offset 1 is a 4-byte-aligned base (the scalar path, also
    at O % 4 == 0), offset 4 an aligned base with ld != O (the vector path at O = 64).  Same bits as the dense call."""
    ops = bnn.ops
    h = bt.og_inputs(B, O)
    d = _og_dev(h, dev)
    g_out, out, std = (_cols(h[k], off, bt.OG_PAD, dev) for k in ("g_out", "out", "std"))
    assert g_out.stride(0) == O + bt.OG_PAD and (g_out.data_ptr() % 16 == 0) == (off == 4)
    got = ops.output_grad(g_out, out=out, std=std if stoch else None, eps=d["eps"] if stoch else None, relu=True)
    ref = bt.output_grad_ref(h["g_out"], h["out"], h["std"] if stoch else None, h["eps"] if stoch else None)
    _check_og("(%d,%d) off=%d stoch=%s" % (B, O, off, stoch), B, got, ref, stoch)
    dense = ops.output_grad(d["g_out"], out=d["out"], std=d["std"] if stoch else None, eps=d["eps"] if stoch else None, relu=True)
    _same_bits(got, dense)


@pytest.mark.parametrize("B,O", bt.OG_OPTION_SHAPES)
def test_output_grad_relu_boundary(bnn, dev, B, O):
    """The mask is !(out > 0): +0, -0 and NaN pass no gradient, the smallest positive denormal passes it."""
    ops = bnn.ops
    h = bt.og_inputs(B, O)
    flat = h["out"].view(-1)
    flat[0], flat[1], flat[2] = 0.0, -0.0, NAN
    _bits(flat)[3] = 1                                                   # 2^-149
    assert float(flat[3]) > 0 and h["out"].view(-1)[3] == flat[3]
    h["g_out"].view(-1)[:4] = torch.tensor([1.5, -2.5, 3.5, -4.5])
    d = _og_dev(h, dev)
    got = ops.output_grad(d["g_out"], out=d["out"], std=d["std"], eps=d["eps"], relu=True)
    assert got[0].view(-1)[:4].tolist() == [0.0, 0.0, 0.0, -4.5]
    _check_og("(%d,%d) relu boundary" % (B, O), B, got, bt.output_grad_ref(h["g_out"], h["out"], h["std"], h["eps"]), True)


def test_output_grad_in_kernel_eps_with_a_row_offset(bnn, dev):
    ops = bnn.ops
    B, O, row_offset = bt.OG_PHILOX
    d = _og_dev(bt.og_inputs(B, O), dev)
    rng = ops.RngState.get(dev).t.clone()
    stream = ops.STREAM_EPS_OUT * 64 + 5
    eps = ops.philox_normal(rng, stream, B, O, row_offset)
    assert torch.isfinite(eps).all() and float(eps.std()) > 0.5
    kw = dict(out=d["out"], std=d["std"], relu=True, gv_scale=d["gv_scale"])
    drawn = ops.output_grad(d["g_out"], rng=rng, rng_stream=stream, row_offset=row_offset, **kw)
    given = ops.output_grad(d["g_out"], eps=eps, **kw)
    _same_bits(drawn, given)
    other = ops.output_grad(d["g_out"], rng=rng, rng_stream=stream, row_offset=row_offset + 1, **kw)
    assert not torch.equal(other[1], drawn[1])                           # the offset is honoured


# =========================================================================== 5. lbbnn_dx_combine
@pytest.mark.parametrize("B,I", bt.DX_COMBINE_SHAPES)
def test_dx_combine_strided_x(bnn, dev, B, I):
    """gx += 2 x gxv: against fp64, and against the same expression in torch float32 ops -- bitwise, or apart by no more than the
    one rounding a contracted multiply-add leaves out.  With p = 2 x gxv exact, torch gives rnd(gx + rnd(p)) and a contracted
    kernel rnd(gx + p): the arguments differ by |p - rnd(p)| <= ulp(p) / 2 and each result is within half an ulp of its
    argument, so  |got - ref32| <= ulp(p) / 2 + ulp(got) / 2 + ulp(ref32) / 2  (one ulp of the result where nothing cancels)."""
    ops = bnn.ops
    g = torch.Generator().manual_seed(B * 7 + I)
    gx, gxv, x = (torch.randn(B, I, generator=g) for _ in range(3))
    xs = _cols(x, 2, 5, dev)
    got = ops.dx_combine(gx.to(dev).clone(), gxv.to(dev), xs).cpu()
    ref32 = gx + 2 * x * gxv
    ulp_of = lambda v: torch.ldexp(torch.ones((), dtype=torch.float64), torch.frexp(v.double())[1] - 24)     # |v| in [2^(e-1), 2^e)
    ulp = 0.5 * (ulp_of(2 * x * gxv) + ulp_of(got) + ulp_of(ref32))
    off = (got.double() - ref32.double()).abs()
    assert (off <= ulp).all(), float((off / ulp).max())
    e = rel_err(got, gx.double() + 2 * x.double() * gxv.double())
    print("dx_combine (%d,%d): %.2e (bar %.0e); %d of %d elements differ from the torch float32 expression"
          % (B, I, e, bt.TIGHT, int((off > 0).sum()), B * I))
    assert e < bt.TIGHT


# =========================================================================== 6. csrc/loss_head.hip
class _Head(torch.autograd.Function):
    """Stands where a layer with a fused log_softmax stands (layers._BayesLinearFn.backward): returns log-probabilities, and its
    backward takes the logits gradient the loss's backward left for it, or launches lbbnn_log_softmax_backward itself."""

    @staticmethod
    def forward(ctx, logits, lp, record):
        out = lp.detach()
        ctx.save_for_backward(out)
        ctx.record = record
        return out.view_as(out)

    @staticmethod
    def backward(ctx, g):
        from bnn_amd import losses, ops
        out, = ctx.saved_tensors
        left = losses._HEAD_GRAD.take(out, g)
        ctx.record["taken"] = left is not None
        ctx.record["g_logp"] = g
        return (left if left is not None else ops.log_softmax_backward(g, out)), None, None


def _loss_tensors(dev, B, C, layout, bad):
    d = bt.loss_inputs(B, C, bad)
    lp = d["logp"].to(dev) if layout == "dense" else _cols(d["logp"], bt.LOSS_OFF, bt.LOSS_PAD, dev)
    return d, lp, d["target"].to(dev)


@pytest.mark.parametrize("B,C", bt.LOSS_SHAPES)
@pytest.mark.parametrize("layout", ["dense", "strided"])
@pytest.mark.parametrize("bad", [False, True])
def test_elbo_loss_forward_and_backward_edges(bnn, dev, monkeypatch, B, C, layout, bad):
    from bnn_amd import losses
    d, lp, y = _loss_tensors(dev, B, C, layout, bad)
    scale = 1.0 / bt.LOSS_BATCHES
    ref = bt.loss_ref(d["logp"], d["target"], bt.LOSS_KL, scale, d["g"])
    valid = ref["valid"]
    # forward, with and without the KL term
    kl = torch.tensor(bt.LOSS_KL, device=dev, requires_grad=True)
    e_loss = rel_err(bnn.elbo_loss(lp, y, kl, bt.LOSS_BATCHES), ref["loss"])
    nll = bnn.elbo_loss(lp, y)
    ref_nll = bt.loss_ref(d["logp"], d["target"])["loss"]
    assert e_loss < bt.LOSS_BAR and (rel_err(nll, ref_nll) < bt.LOSS_BAR if valid.any() else float(nll) == 0)
    worst = {}
    for fused in (False, True):
        monkeypatch.setattr(losses, "_FUSE_LSM_BWD", fused)
        # (a) the log-probabilities are a leaf: lbbnn_elbo_loss_backward / the g_logp half of ..._backward_logits
        leaf = lp.detach().requires_grad_(True)
        kl.grad = None
        bnn.elbo_loss(leaf, y, kl, bt.LOSS_BATCHES).backward(d["g"].to(dev))
        g_logp = leaf.grad.cpu()
        assert (g_logp[~valid] == 0).all()
        e_a, e_k = rel_err(g_logp, ref["g_logp"]), rel_err(kl.grad, ref["g_kl"])
        assert e_a < bt.LOSS_BAR and e_k < bt.LOSS_BAR, (fused, e_a, e_k)
        # (b) they come from a head with a fused log_softmax: the gradient of the logits, handed over or by
        # lbbnn_log_softmax_backward on the (strided) log-probabilities
        logits = d["logits"].to(dev).requires_grad_(True)
        record = {}
        bnn.elbo_loss(_Head.apply(logits, lp, record), y, kl, bt.LOSS_BATCHES).backward(d["g"].to(dev))
        assert record["taken"] == fused
        g_logits = logits.grad.cpu()
        e_b = rel_err(g_logits, ref["g_logits"])
        worst[fused] = max(e_a, e_k, e_b)
        assert (record["g_logp"].cpu()[~valid] == 0).all()
        assert (g_logits[~valid] == 0).all(), "rows with a target outside [0, C) must get no gradient (fused=%s)" % fused
        assert e_b < bt.LOSS_BAR, (fused, e_b)
        if fused:
            assert torch.equal(_bits(logits.grad), _bits(two_launch))    # same expression, same order: the same bits
        else:
            two_launch = logits.grad.clone()
    print("loss (%d,%d) %s bad=%s: loss %.2e, gradients %.2e two launches / %.2e handed over (bar %.0e)"
          % (B, C, layout, bad, e_loss, worst[False], worst[True], bt.LOSS_BAR))


@pytest.mark.parametrize("C", bt.LSM_CLASSES)
def test_log_softmax_backward_at_the_class_limits(bnn, dev, C):
    ops = bnn.ops
    B = 300
    d = bt.loss_inputs(B, C, False)
    g, lp = _cols(d["gout"], 3, 5, dev), _cols(d["logp"], bt.LOSS_OFF, bt.LOSS_PAD, dev)
    got = ops.log_softmax_backward(g, lp)
    ref = bt.lsm_backward_ref(d["gout"], d["logp"])
    if C == 1:
        assert float(ref.abs().max()) == 0 and float(got.abs().max()) == 0
        return
    e = rel_err(got, ref)
    print("log_softmax_backward C=%d: %.2e (bar %.0e)" % (C, e, bt.LSM_BAR))
    assert got.shape == (B, C) and e < bt.LSM_BAR
    with pytest.raises(RuntimeError, match="lbbnn_log_softmax_backward"):
        ops.log_softmax_backward(torch.zeros(2, 65, device=dev), torch.zeros(2, 65, device=dev))


def test_network_gradients_with_ignored_targets_same_through_both_loss_backwards(bnn, dev, monkeypatch):
    """A small planar MNF net whose head fuses its log_softmax, ~1 in 5 targets at -100 or at C: every parameter gradient is
    bitwise the same whether the loss's backward hands the logits gradient over or the head launches
    lbbnn_log_softmax_backward -- as test_loss_backward_hands_the_logits_gradient_to_the_head asserts for valid targets."""
    from bnn_amd import losses
    grads = {}
    for fused in (True, False):
        monkeypatch.setattr(losses, "_FUSE_LSM_BWD", fused)
        bnn.manual_seed(5, 0)
        torch.manual_seed(5)
        net = bnn.mnf.BayesianNetwork((20, 12, 5), 2, z_flow_type="Planar", r_flow_type="Planar").to(dev).train()
        xg = torch.Generator().manual_seed(1)
        x = torch.rand(33, 20, generator=xg).to(dev)
        y = torch.randint(0, 5, (33,), generator=xg)
        y[::5] = -100
        y[3::11] = 5
        loss = bnn.elbo_loss(net(x, sample=True), y.to(dev), net.kl(), 10)
        loss.backward()
        grads[fused] = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    for n in grads[True]:
        assert torch.isfinite(grads[True][n]).all(), n
        assert torch.equal(grads[True][n], grads[False][n]), n
