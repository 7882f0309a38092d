"""CPU tier: which C call ops.lrt_gemm / ops.lrt_gemm16 make and with which arguments, with the library replaced by a recorder.
lbbnn_lrt_gemm stays positional and is the product alone; everything a forward adds to it (std_out, the KL finalize and the RNG
advance that ride in the launch, and the fp16 format's planes / head fold) goes through ONE lbbnn_gemm_desc_t."""
import ctypes

import pytest
import torch

B, I, O, LDX, LDO, STREAM = 5, 12, 20, 16, 24, 77


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: lets the host side of a launch run with the library replaced."""
    is_cuda = property(lambda self: True)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def rec(monkeypatch):
    from bnn_amd import _lib, ops
    r = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: r)
    monkeypatch.setattr(ops, "_ptr", lambda t, name="tensor": None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    return r


@pytest.fixture
def t():
    """The tensors of one call: x rows wider than I and an output wider than O (ldx, ldo are row strides)."""
    from bnn_amd import ops
    ld = ops.operand_ld(I)
    return dict(x=torch.rand(B, LDX)[:, :I].as_subclass(_OnDevice), e_w=torch.zeros(O, ld), var_w=torch.zeros(O, ld),
                bias_mean=torch.zeros(O), bias_var=torch.zeros(O), var_scale=torch.zeros(O), eps=torch.zeros(B, O),
                rng=torch.tensor([7, 11], dtype=torch.int64), out=torch.zeros(B, LDO)[:, :O], std_out=torch.zeros(B, O))


def _kw(t, *names):
    return dict(I=I, O=O, bias_mean=t["bias_mean"], bias_var=t["bias_var"], var_scale=t["var_scale"], eps=t["eps"], rng=t["rng"],
                rng_stream=70, row_offset=1000, relu=True, out=t["out"], **{n: t[n] for n in names})


_FP16_ONLY = ("mean_scale", "wvar_scale", "out_planes", "ldp", "head_e", "head_v", "head_ld", "head_classes", "head_bias_mean",
              "head_bias_var", "head_eps", "head_rng_stream", "head_out", "head_ldo", "head_slab", "head_flags")


def _the_desc(rec):
    """The descriptor of the one recorded call (the recorded byref keeps its struct alive)."""
    assert [c[0] for c in rec.calls] == ["lbbnn_lrt_gemm_ex"]
    args = rec.calls[0][1]
    assert len(args) == 2 and args[1] == STREAM
    return args[0]._obj


def _check_shared(d, t, flags, std_out, fin, rows=B):
    """Every field both formats have holds exactly what was given."""
    from bnn_amd import ops
    want = dict(x=t["x"].data_ptr(), ldx=LDX, e_w=t["e_w"].data_ptr(), var_w=t["var_w"].data_ptr(), ld=ops.operand_ld(I),
                bias_mean=t["bias_mean"].data_ptr(), bias_var=t["bias_var"].data_ptr(), var_scale=t["var_scale"].data_ptr(),
                eps=t["eps"].data_ptr(), rng=t["rng"].data_ptr(), rng_stream=70, row_offset=1000, out=t["out"].data_ptr(), ldo=LDO,
                std_out=t["std_out"].data_ptr() if std_out else 0, B=rows, I=I, O=O, flags=flags,
                n_layers=fin.n if fin else 0, fin_rng=(fin.fin_rng if fin else 0) or 0, kl_total=(fin.kl_total if fin else 0) or 0,
                rng_live=(fin.rng_live if fin else 0) or 0, advance=fin.advance if fin else 0)
    got = {k: getattr(d, k) or 0 for k in want}
    assert got == want
    if fin is not None and fin.layers is not None:
        assert ctypes.addressof(d.layers.contents) == ctypes.addressof(fin.layers)
    else:
        assert not d.layers


def test_the_plain_product_is_one_positional_call(rec, t):
    from bnn_amd import ops
    got = ops.lrt_gemm(t["x"], t["e_w"], t["var_w"], split=True, single=False, **_kw(t))
    assert got is t["out"]
    assert [c[0] for c in rec.calls] == ["lbbnn_lrt_gemm"]
    assert rec.calls[0][1] == (
        t["x"].data_ptr(), LDX, t["e_w"].data_ptr(), t["var_w"].data_ptr(), ops.operand_ld(I), t["bias_mean"].data_ptr(),
        t["bias_var"].data_ptr(), t["var_scale"].data_ptr(), t["eps"].data_ptr(), t["rng"].data_ptr(), 70, 1000,
        t["out"].data_ptr(), LDO, B, I, O, ops.F_RELU | ops.F_SPLIT16, STREAM)


@pytest.mark.parametrize("case", ["std_out", "n=0", "n=0+std_out", "layers", "layers+advance"])
def test_what_a_forward_adds_goes_through_the_descriptor(rec, t, case):
    from bnn_amd import _lib, ops
    layers = (_lib.LayerDesc * 2)()
    fin = {"std_out": None,
           "n=0": ops.Finalize(layers=None, n=0, fin_rng=None, kl_total=None, rng_live=t["rng"].data_ptr(), advance=1),
           "n=0+std_out": ops.Finalize(layers=None, n=0, fin_rng=None, kl_total=None),
           "layers": ops.Finalize(layers=layers, n=2, fin_rng=4096, kl_total=8192),
           "layers+advance": ops.Finalize(layers=layers, n=2, fin_rng=4096, kl_total=None, rng_live=12288, advance=3)}[case]
    std_out = "std_out" in case
    got = ops.lrt_gemm(t["x"], t["e_w"], t["var_w"], split=True, single=False, finalize=fin,
                       **_kw(t, *(("std_out",) if std_out else ())))
    assert got is t["out"]
    d = _the_desc(rec)
    _check_shared(d, t, ops.F_RELU | ops.F_SPLIT16, std_out, fin)
    assert all(not getattr(d, k) for k in _FP16_ONLY)


def test_a_plain_finalize_tuple_is_taken_as_a_finalize(rec, t):
    """(layers, n, fin_rng, kl_total[, rng_live, advance]) in that order is what ops.Finalize names."""
    from bnn_amd import _lib, ops
    layers = (_lib.LayerDesc * 1)()
    ops.lrt_gemm(t["x"], t["e_w"], t["var_w"], finalize=(layers, 1, 4096, None), **_kw(t))
    _check_shared(_the_desc(rec), t, ops.F_RELU, False, ops.Finalize(layers, 1, 4096, None))


@pytest.mark.parametrize("head", [False, True])
def test_the_fp16_form_adds_its_fields_to_the_same_descriptor(rec, t, head):
    from bnn_amd import _lib, ops
    C = 10
    e_scale, v_scale, planes = torch.zeros(O), torch.zeros(O), torch.zeros(B, ops.plane_ld(O))
    h = dict(e_w=torch.zeros(C, ops.operand_ld(O)), var_w=torch.zeros(C, ops.operand_ld(O)), bias_mean=torch.zeros(C),
             bias_var=torch.zeros(C), eps=None, rng_stream=9, out=torch.zeros(B, 16)[:, :C], slab=torch.zeros(ops.operand_ld(O) * B),
             log_softmax=True) if head else None
    layers = (_lib.LayerDesc * 2)()
    fin = ops.Finalize(layers=layers, n=2, fin_rng=4096, kl_total=8192, rng_live=12288, advance=1)
    o, p = ops.lrt_gemm16(t["x"], t["e_w"], t["var_w"], e_scale, v_scale, var1=True, out_planes=planes, finalize=fin, head=h,
                          **_kw(t, "std_out"))
    assert o is t["out"] and p is planes
    d = _the_desc(rec)
    _check_shared(d, t, ops.F_F16S | ops.F_RELU | ops.F_VAR1, True, fin)
    assert (d.mean_scale, d.wvar_scale, d.out_planes, d.ldp) == (e_scale.data_ptr(), v_scale.data_ptr(), planes.data_ptr(),
                                                                 ops.plane_ld(O))
    if head:
        assert (d.head_e, d.head_v, d.head_ld, d.head_classes) == (h["e_w"].data_ptr(), h["var_w"].data_ptr(), ops.operand_ld(O), C)
        assert (d.head_bias_mean, d.head_bias_var, d.head_eps, d.head_rng_stream) == (h["bias_mean"].data_ptr(),
                                                                                      h["bias_var"].data_ptr(), None, 9)
        assert (d.head_out, d.head_ldo, d.head_slab, d.head_flags) == (h["out"].data_ptr(), 16, h["slab"].data_ptr(),
                                                                       ops.F_LOG_SOFTMAX)
    else:
        assert all(not getattr(d, k) for k in _FP16_ONLY if k.startswith("head_"))


def test_x_planes_set_the_flag_and_the_plane_row_stride(rec, t):
    from bnn_amd import ops
    xp = torch.zeros(B, ops.plane_ld(I)).as_subclass(_OnDevice)
    ops.lrt_gemm16(xp, t["e_w"], t["var_w"], torch.zeros(O), torch.zeros(O), x_planes=True, **_kw(t))
    d = _the_desc(rec)
    assert (d.x, d.ldx, d.B, d.I, d.flags) == (xp.data_ptr(), ops.plane_ld(I), B, I, ops.F_F16S | ops.F_RELU | ops.F_XPLANES)
    with pytest.raises(RuntimeError, match="x planes must be"):
        ops.lrt_gemm16(t["x"], t["e_w"], t["var_w"], torch.zeros(O), torch.zeros(O), x_planes=True, **_kw(t))


@pytest.mark.parametrize("f16", [False, True])
def test_an_empty_batch_calls_only_for_its_finalize(rec, t, f16):
    from bnn_amd import _lib, ops
    x0 = torch.rand(0, I).as_subclass(_OnDevice)
    kw = dict(I=I, O=O, rng=t["rng"])
    call = ((lambda **k: ops.lrt_gemm16(x0, t["e_w"], t["var_w"], torch.zeros(O), torch.zeros(O), **kw, **k)[0]) if f16 else
            (lambda **k: ops.lrt_gemm(x0, t["e_w"], t["var_w"], **kw, **k)))
    out = call()
    assert tuple(out.shape) == (0, O) and rec.calls == []
    layers = (_lib.LayerDesc * 1)()
    out = call(finalize=ops.Finalize(layers=layers, n=1, fin_rng=4096, kl_total=None))
    d = _the_desc(rec)
    assert tuple(out.shape) == (0, O) and (d.B, d.I, d.O, d.n_layers) == (0, I, O, 1)
    with pytest.raises(RuntimeError, match="eps must be"):
        call(eps=torch.zeros(1, O))


def test_the_wrappers_refuse_a_wrong_input_shape(rec, t):
    from bnn_amd import ops
    with pytest.raises(RuntimeError, match=r"input must be \(B,12\)"):
        ops.lrt_gemm(torch.rand(B, I + 1), t["e_w"], t["var_w"], I=I, O=O)
    with pytest.raises(RuntimeError, match=r"input must be \(B,12\)"):
        ops.lrt_gemm16(torch.rand(B, I + 1), t["e_w"], t["var_w"], torch.zeros(O), torch.zeros(O), I=I, O=O)
    assert rec.calls == []
