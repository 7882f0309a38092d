"""GPU tier of the frozen operand kernels (csrc/frozen.hip) at edges the networks of tests/test_frozen_gpu.py and
tests/test_frozen_compact_gpu.py do not reach, through direct C calls of lbbnn_frozen_operands,
lbbnn_frozen_operands_compact, lbbnn_frozen_members and lbbnn_frozen_members_compact.

Every operand call has two layers of O = 5 rows each, so a workgroup of either layer runs (both branches of the
workgroup-to-layer rule) and the second workgroup of a layer has three idle waves:

* full, fp32: I = 1028 in rows of ld = 1056 -- 264 column groups, a lane's fifth group lies in the second batch of four and
  that batch is partial (784, the widest network elsewhere, stays inside the first); I = 7, ld = 32 -- the scalar load
  path with a partial last group;
* full, bf16 hi | lo: the same first layer and I = 8, ld = 32;
* compact, fp32: 5 of 9 rows and I' = 1028 of I_full = 1300 columns (every fifth column taken out): the third batch of two
  groups is partial; I' = 7 of 13;
* compact, bf16 hi | lo: I' = 1032 and I' = 8.

Both gate modes for the full calls, cut in {0, -0.25} everywhere: with a negative cut a zero-filled tail element would count
as kept if the tail were not masked.  lambdal is seeded U(-3, 3), moved at least 2e-3 away from the cut.  Every output buffer
is filled with NaN first and has one row more than the call writes.

Bars (tests/test_frozen_gpu.py): exact for e0 / e_w (fp32) / kept_rows / the zero tails in MPM mode, 5e-6 as rel_err and the
element-wise form for var_w, 5e-6 for bias_var and the alpha-mode means; a split operand is bit for bit lbbnn_format_operand
of the fp32 operand and decodes to it within 2e-5; a compact result is bit for bit the full result gathered."""
import ctypes

import pytest
import torch

from conftest import elementwise_violation, rel_err
from oracle import lbbnn_oracle as orc

pytestmark = pytest.mark.gpu

TIGHT = 5e-6
SPLIT_BAR = 2e-5
F_SPLIT16 = 0x4
O = 5
ROWS9 = [0, 2, 3, 6, 8]                       # the compact rows of a 9-row layer
ROWS7 = [1, 2, 4, 5, 6]                       # ... of a 7-row layer
CUTS = [0.0, -0.25]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def env():
    import bnn_amd
    from bnn_amd import _lib
    return bnn_amd, _lib, _lib.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _params(dev, Of, If, cut, seed):
    """mu / rho / lambdal (Of, If) and bias_rho (Of) of one layer, on the host and on the device."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(Of, If, generator=g) * 0.3
    rho = torch.empty(Of, If).uniform_(-5.0, -1.0, generator=g)
    lam = torch.empty(Of, If).uniform_(-3.0, 3.0, generator=g)
    d = lam - cut
    lam = torch.where(d.abs() < 2e-3, cut + torch.where(d < 0, -2e-3, 2e-3), lam)
    assert float((lam - cut).abs().min()) >= 1e-3
    kept = int((lam > cut).sum())
    assert 0 < kept < Of * If
    bias_rho = torch.empty(Of).uniform_(-4.0, 0.0, generator=g)
    host = dict(mu=mu, rho=rho, lam=lam, bias_rho=bias_rho)
    return host, {k: v.to(dev) for k, v in host.items()}


def _nan(dev, *shape, dtype=torch.float32):
    t = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    return t.view(dtype) if dtype != torch.float32 else t


def _outputs(dev, ld):
    """NaN-filled outputs of one layer with one guard row / element more than the call writes."""
    return dict(e0=_nan(dev, O + 1, ld), e_w=_nan(dev, O + 1, ld), var_w=_nan(dev, O + 1, ld), bias_var=_nan(dev, O + 1),
                kept_rows=_nan(dev, O + 1, dtype=torch.int32))


def _fill(d, p, out, I, ld, split, mode, cut, layer_id):
    d.weight_mu, d.weight_rho, d.lambdal, d.bias_rho = (p[k].data_ptr() for k in ("mu", "rho", "lam", "bias_rho"))
    d.e0, d.e_w, d.var_w = out["e0"].data_ptr(), out["e_w"].data_ptr(), out["var_w"].data_ptr()
    d.bias_var, d.kept_rows = out["bias_var"].data_ptr(), out["kept_rows"].data_ptr()
    d.O, d.I, d.ld, d.flags, d.mode, d.cut, d.layer_id = O, I, ld, F_SPLIT16 if split else 0, mode, cut, layer_id


def _index(dev, idx):
    return torch.tensor(idx, dtype=torch.int32, device=dev)


def _decode_split(buf, ld):
    """(rows, ld) fp32 view of a bf16 hi | lo operand (csrc/lbbnn_device.h: per 32 k one 128-B line of eight 16-B units,
    unit 2g = hi of k in [8g, 8g + 8), unit 2g + 1 = lo of the same k) -> (hi + lo in float64, any NaN half)."""
    h = buf.view(torch.bfloat16).reshape(buf.shape[0], ld // 32, 4, 2, 8)
    val = (h[:, :, :, 0, :].double() + h[:, :, :, 1, :].double()).reshape(buf.shape[0], ld)
    return val.cpu(), bool(torch.isnan(h.float()).any())


def _check_guards(out):
    for k in ("e0", "e_w", "var_w", "bias_var"):
        assert bool(torch.isnan(out[k][O:]).all()), k                     # nothing written past the O rows
    assert int(out["kept_rows"][O]) == 0x7FC00000


def _check_layer(bnn, dev, host, out, I, ld, split, mode, cut, rows=None, cols=None):
    """One layer's outputs against torch on the host; rows / cols: the compact map (None: the full layer)."""
    mu, rho, lam, bias_rho = host["mu"], host["rho"], host["lam"], host["bias_rho"]
    if rows is not None:
        r, c = torch.tensor(rows), torch.tensor(cols)
        mu, rho, lam, bias_rho = mu[r][:, c], rho[r][:, c], lam[r][:, c], bias_rho[r]
    assert mu.shape == (O, I)
    torch.cuda.synchronize()
    _check_guards(out)
    e0 = out["e0"][:O].cpu()
    keep = lam > torch.tensor(cut, dtype=torch.float32)                   # fp32, as the kernel compares
    assert torch.equal(out["kept_rows"][:O].cpu().long(), keep.sum(1))
    assert not bool(torch.isnan(e0).any())
    assert bool((e0[:, I:].view(torch.int32) == 0).all())                 # the padding: +0.0
    s2 = orc.sigma_of(rho.double()) ** 2
    if mode == 1:
        ref_e0 = torch.where(keep, mu, torch.zeros_like(mu))
        assert torch.equal(e0[:, :I].view(torch.int32), ref_e0.view(torch.int32))       # mu or +0.0, bit for bit
        a = keep.double()
    else:
        a = orc.alpha_of(lam.double())
        assert rel_err(e0[:, :I], mu.double() * a) < TIGHT
    ref_var = s2 * a ** 2
    assert rel_err(out["bias_var"][:O], orc.sigma_of(bias_rho.double()) ** 2) < TIGHT
    if not split:
        e_w, var_w = out["e_w"][:O].cpu(), out["var_w"][:O].cpu()
        assert torch.equal(e_w.view(torch.int32), e0.view(torch.int32))
        assert not bool(torch.isnan(var_w).any())
        assert bool((var_w[:, I:].view(torch.int32) == 0).all())
        ev, vv = rel_err(var_w[:, :I], ref_var), elementwise_violation(var_w[:, :I], ref_var)
        print("var_w I=%d mode=%d cut=%g rel_err %.3g elementwise %.3g" % (I, mode, cut, ev, vv))
        assert ev < TIGHT and vv <= 1.0
        if mode == 1:
            assert bool((var_w[:, :I][~keep] == 0).all())
        return e0, var_w
    # bf16 hi | lo units: the format kernel's bits of the fp32 operand, and close to it
    e_dec, e_nan = _decode_split(out["e_w"][:O], ld)
    v_dec, v_nan = _decode_split(out["var_w"][:O], ld)
    assert not e_nan and not v_nan
    assert bool((e_dec[:, I:] == 0).all()) and bool((v_dec[:, I:] == 0).all())
    es, vs = rel_err(e_dec[:, :I], e0[:, :I]), rel_err(v_dec[:, :I], ref_var)
    print("split I=%d mode=%d cut=%g decode rel_err e_w %.3g var_w %.3g" % (I, mode, cut, es, vs))
    assert es < SPLIT_BAR and vs < SPLIT_BAR
    assert torch.equal(out["e_w"][:O].view(torch.int32),
                       bnn.ops.format_operand(out["e0"][:O, :I], split=True).view(torch.int32))
    return e0, None


def _full_call(env, dev, shapes, split, mode, cut, seed=3):
    """One lbbnn_frozen_operands call over len(shapes) layers of O rows; shapes: (I, ld)."""
    bnn, _lib, lib = env
    descs = (_lib.FrozenDesc * len(shapes))()
    layers = []
    for i, (I, ld) in enumerate(shapes):
        host, p = _params(dev, O, I, cut, seed + i)
        out = _outputs(dev, ld)
        _fill(descs[i], p, out, I, ld, split, mode, cut, i)
        layers.append((host, p, out))
    assert lib.lbbnn_frozen_operands(descs, len(shapes), _stream(dev)) == 0
    return layers


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("mode", [0, 1], ids=["alpha", "mpm"])
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
def test_full_operands_second_batch_and_scalar_rows(env, dev, split, mode, cut):
    shapes = [(1028, 1056), (8, 32) if split else (7, 32)]
    layers = _full_call(env, dev, shapes, split, mode, cut)
    for (I, ld), (host, p, out) in zip(shapes, layers):
        _check_layer(env[0], dev, host, out, I, ld, split, mode, cut)
    if split:                                                             # the same call in fp32: the same values
        ref = _full_call(env, dev, shapes, False, mode, cut)
        torch.cuda.synchronize()
        for (I, ld), (_, _, out), (_, _, rout) in zip(shapes, layers, ref):
            assert torch.equal(out["e0"][:O].view(torch.int32), rout["e0"][:O].view(torch.int32))
            assert torch.equal(out["var_w"][:O].view(torch.int32),
                               env[0].ops.format_operand(rout["var_w"][:O, :I], split=True).view(torch.int32))
            assert torch.equal(out["kept_rows"][:O], rout["kept_rows"][:O])


def _compact_shapes(split):
    """(O_full, I_full, rows, cols, I', ld') of the two layers."""
    cols0 = [c for c in range(1300) if c % 5 != 4]                        # sorted, every fifth column out: 1040 left
    cols1 = [0, 1, 3, 4, 6, 8, 9, 11, 12]                                 # of 13
    n0, n1 = (1032, 8) if split else (1028, 7)
    return [(9, 1300, ROWS9, cols0[:n0], n0, 1056), (7, 13, ROWS7, cols1[:n1], n1, 32)]


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
def test_compact_operands_partial_batches_equal_the_full_operands_gathered(env, dev, split, cut):
    bnn, _lib, lib = env
    shapes = _compact_shapes(split)
    descs = (_lib.FrozenDesc * 2)()
    maps = (_lib.CompactMap * 2)()
    fdescs = (_lib.FrozenDesc * 2)()
    layers = []
    for i, (Of, If, rows, cols, I, ld) in enumerate(shapes):
        host, p = _params(dev, Of, If, cut, 11 + i)
        out = _outputs(dev, ld)
        _fill(descs[i], p, out, I, ld, split, 1, cut, i)
        r, c = _index(dev, rows), _index(dev, cols)
        maps[i].rows, maps[i].cols, maps[i].O_full, maps[i].I_full = r.data_ptr(), c.data_ptr(), Of, If
        # the full layer, fp32, to gather from
        ldf = bnn.ops.operand_ld(If)
        fout = dict(e0=_nan(dev, Of, ldf), e_w=_nan(dev, Of, ldf), var_w=_nan(dev, Of, ldf), bias_var=_nan(dev, Of),
                    kept_rows=_nan(dev, Of, dtype=torch.int32))
        _fill(fdescs[i], p, fout, If, ldf, False, 1, cut, i)
        fdescs[i].O = Of
        layers.append((host, p, out, fout, r, c))
    assert lib.lbbnn_frozen_operands_compact(descs, maps, 2, _stream(dev)) == 0
    assert lib.lbbnn_frozen_operands(fdescs, 2, _stream(dev)) == 0
    for (Of, If, rows, cols, I, ld), (host, p, out, fout, r, c) in zip(shapes, layers):
        _check_layer(bnn, dev, host, out, I, ld, split, 1, cut, rows, cols)
        rl, cl = r.long(), c.long()
        ref_e0, ref_var = fout["e0"][rl][:, cl], fout["var_w"][rl][:, cl]
        assert torch.equal(out["e0"][:O, :I].view(torch.int32), ref_e0.view(torch.int32))
        assert torch.equal(out["bias_var"][:O].view(torch.int32), fout["bias_var"][rl].view(torch.int32))
        if split:
            assert torch.equal(out["e_w"][:O].view(torch.int32), bnn.ops.format_operand(ref_e0, split=True).view(torch.int32))
            assert torch.equal(out["var_w"][:O].view(torch.int32), bnn.ops.format_operand(ref_var, split=True).view(torch.int32))
        else:
            assert torch.equal(out["e_w"][:O, :I].view(torch.int32), ref_e0.view(torch.int32))
            assert torch.equal(out["var_w"][:O, :I].view(torch.int32), ref_var.view(torch.int32))


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
def test_compact_member_operands_equal_the_full_members_gathered(env, dev, split):
    """One MNF layer, 5 of 7 rows and 8 of 12 columns, two planar transforms, three members one Philox offset apart: the flow
    runs at the full width in both calls, so e_w_members[m] of the compact call is the full call's, gathered."""
    bnn, _lib, lib = env
    Of, If, I, ld, T, S = 7, 12, 8, 32, 2, 3
    rows, cols = ROWS7, [0, 1, 3, 4, 6, 8, 9, 11]
    g = torch.Generator().manual_seed(5)
    e0_full = torch.zeros(Of, ld)
    e0_full[:, :If] = torch.randn(Of, If, generator=g)
    e0_c = torch.zeros(O, ld)
    e0_c[:, :I] = e0_full[torch.tensor(rows)][:, torch.tensor(cols)]
    e0_full, e0_c = e0_full.to(dev), e0_c.to(dev)
    q0_mean, q0_log_var = torch.randn(If, generator=g).to(dev), (torch.randn(If, generator=g) * 0.1 - 2.0).to(dev)
    u, w = (torch.randn(T, If, generator=g) * 0.3).to(dev), (torch.randn(T, If, generator=g) * 0.3).to(dev)
    b = torch.randn(T, 4, generator=g).to(dev)
    r, c = _index(dev, rows), _index(dev, cols)

    def call(compact):
        d = (_lib.FrozenDesc * 1)()
        z = _nan(dev, S, 32)
        n_rows = O if compact else Of
        ewm = _nan(dev, S, n_rows, ld)
        d[0].q0_mean, d[0].q0_log_var = q0_mean.data_ptr(), q0_log_var.data_ptr()
        d[0].z_flow.T = T
        for t in range(T):
            d[0].z_flow.u[t], d[0].z_flow.w[t], d[0].z_flow.b[t] = u[t].data_ptr(), w[t].data_ptr(), b[t].data_ptr()
        d[0].e0 = (e0_c if compact else e0_full).data_ptr()
        d[0].z_fwd, d[0].z_mstride, d[0].e_w_members = z.data_ptr(), 32, ewm.data_ptr()
        d[0].O, d[0].I, d[0].ld, d[0].layer_id = n_rows, I if compact else If, ld, 2
        d[0].flags = F_SPLIT16 if (split and compact) else 0
        rng = torch.tensor([3, 5], dtype=torch.int64, device=dev)
        if compact:
            m = (_lib.CompactMap * 1)()
            m[0].rows, m[0].cols, m[0].O_full, m[0].I_full = r.data_ptr(), c.data_ptr(), Of, If
            assert lib.lbbnn_frozen_members_compact(d, m, 1, S, rng.data_ptr(), 1, _stream(dev)) == 0
        else:
            assert lib.lbbnn_frozen_members(d, 1, S, rng.data_ptr(), 1, _stream(dev)) == 0
        torch.cuda.synchronize()
        return z, ewm

    zf, full = call(False)
    zc, comp = call(True)
    assert torch.equal(zf[:, :If].view(torch.int32), zc[:, :If].view(torch.int32)) and not bool(torch.isnan(zf[:, :If]).any())
    assert not torch.equal(zf[0, :If], zf[1, :If])                        # the members differ
    rl, cl = r.long(), c.long()
    for m in range(S):
        ref = full[m][rl][:, cl]
        assert not bool(torch.isnan(ref).any())
        assert torch.equal(ref.view(torch.int32), (e0_full[rl][:, cl] * zf[m, cl]).view(torch.int32)[:, :I])
        if split:
            _, has_nan = _decode_split(comp[m], ld)
            assert not has_nan
            assert torch.equal(comp[m].view(torch.int32), bnn.ops.format_operand(ref, split=True).view(torch.int32)), m
        else:
            assert torch.equal(comp[m][:, :I].view(torch.int32), ref.view(torch.int32)), m
            assert bool((comp[m][:, I:].view(torch.int32) == 0).all())
