"""CPU tier of the baseline LBBNN's batched ensemble evaluation (include/lbbnn.h lbbnn_gate_members /
lbbnn_gemm_members_mean, evaluate.base_ensemble): the new entry points are exported and bound, the new struct matches the
header, the argument checks return the documented codes without launching, the Python interface rejects what it cannot
run, and predictive_entropy is the reference's outofsample formula."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lbbnn_gate_members", "lbbnn_gemm_members_mean")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_new_symbols_exported_and_bound(lib):
    from bnn_amd import _lib
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n


def test_member_desc_layout_matches_the_header(tmp_path):
    from bnn_amd import _lib
    cname, cls = "lbbnn_gate_member_desc_t", _lib.GateMemberDesc
    fields = ("mu", "bias_rho", "w_out", "gate_rows", "gates", "O", "ld", "exact", "layer_id")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"),
             "int main(void) {", 'printf("size %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f in fields]
    lines += ["return 0; }"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict((l.split()[0], int(l.split()[1]))
               for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == got["size"]
    for f in fields:
        assert getattr(cls, f).offset == got[f], f


def test_gates_and_stream_constants_match_the_header():
    from bnn_amd import ops
    src = open(os.path.join(ROOT, "include", "lbbnn.h")).read()
    assert "#define LBBNN_GATES_SAMPLE %d" % ops.GATES_SAMPLE in src
    assert "#define LBBNN_GATES_MPM %d" % ops.GATES_MPM in src


def _desc(_lib, fake, O=4, I=4, ld=32):
    d = (_lib.GateMemberDesc * 1)()
    for n in ("mu", "rho", "lambdal", "bias_mu", "bias_rho", "w_out", "bias_out"):
        setattr(d[0], n, fake)
    d[0].O, d[0].I, d[0].ld = O, I, ld
    return d


def test_gate_members_argument_checks(lib):
    """Every bad argument returns its code before anything is launched (the pointers are never dereferenced)."""
    from bnn_amd import _lib
    fake = ctypes.c_void_p(4096)
    d = _desc(_lib, fake)
    assert lib.lbbnn_gate_members(None, 1, 3, 0, 0.5, fake, 1, None) == -1
    assert lib.lbbnn_gate_members(d, 0, 3, 0, 0.5, fake, 1, None) == -2
    assert lib.lbbnn_gate_members(d, 5, 3, 0, 0.5, fake, 1, None) == -2
    assert lib.lbbnn_gate_members(d, 1, 0, 0, 0.5, fake, 1, None) == -2                # members < 1
    assert lib.lbbnn_gate_members(d, 1, 65536, 0, 0.5, fake, 1, None) == -2            # members > 65535
    assert lib.lbbnn_gate_members(d, 1, 3, 2, 0.5, fake, 1, None) == -4                # unknown gates mode
    assert lib.lbbnn_gate_members(d, 1, 3, 0, 0.0, fake, 1, None) == -4                # relaxed gate needs T > 0
    assert lib.lbbnn_gate_members(d, 1, 3, 0, float("nan"), fake, 1, None) == -4
    assert lib.lbbnn_gate_members(d, 1, 3, 1, 0.5, None, 1, None) == -5                # MPM still draws eps: rng required
    for n in ("mu", "rho", "lambdal", "bias_mu", "bias_rho", "w_out", "bias_out"):
        e = _desc(_lib, fake)
        setattr(e[0], n, None)
        assert lib.lbbnn_gate_members(e, 1, 3, 0, 0.5, fake, 1, None) == -1, n
    e = _desc(_lib, fake, O=0)
    assert lib.lbbnn_gate_members(e, 1, 3, 0, 0.5, fake, 1, None) == -2
    e = _desc(_lib, fake, I=40, ld=32)                                                    # ld < I
    assert lib.lbbnn_gate_members(e, 1, 3, 0, 0.5, fake, 1, None) == -3
    e = _desc(_lib, fake, ld=48)                                                          # ld not a multiple of 32
    assert lib.lbbnn_gate_members(e, 1, 3, 0, 0.5, fake, 1, None) == -3
    e = _desc(_lib, fake, I=4100, ld=4128)                                                # wider than the kernel's rows
    assert lib.lbbnn_gate_members(e, 1, 3, 0, 0.5, fake, 1, None) == -2
    e = _desc(_lib, fake)
    e[0].w_out = 4100                                                                     # operand base not 16-B aligned
    assert lib.lbbnn_gate_members(e, 1, 3, 0, 0.5, fake, 1, None) == -3
    e = _desc(_lib, fake)
    e[0].flags = 0x1                                                                      # only LBBNN_F_SPLIT16
    assert lib.lbbnn_gate_members(e, 1, 3, 0, 0.5, fake, 1, None) == -4


def test_gemm_members_mean_argument_checks(lib):
    fake = ctypes.c_void_p(4096)
    B, I, O, ld = 8, 32, 24, 32
    ok = dict(x_ms=0, w_ms=O * ld, b_ms=O, o_ms=B * O, flags=0x1, members=3, O=O)

    def call(x=fake, w=fake, out=fake, **kw):
        a = dict(ok, **kw)
        return lib.lbbnn_gemm_members_mean(x, I, a["x_ms"], w, a["w_ms"], ld, fake, a["b_ms"], out, a["O"], a["o_ms"],
                                           B, I, a["O"], a["flags"], a["members"], None)
    assert call(x=None) == -1 and call(w=None) == -1 and call(out=None) == -1
    assert call(members=0) == -2 and call(members=65536) == -2
    assert call(flags=0x2) == -4                    # LBBNN_F_MEAN_ONLY is implied, not accepted
    assert call(flags=0x10) == -4 and call(flags=0x100) == -4
    assert call(flags=0x8, O=17, o_ms=B * 17 + 4) == -4      # the fused log_softmax needs O <= 16
    assert call(x_ms=2) == -3 and call(w_ms=O * ld + 2) == -3 and call(o_ms=B * O + 2) == -3
    assert call(o_ms=B * O - 4) == -2 and call(x_ms=-4) == -2 and call(b_ms=-1) == -2


def test_predictive_entropy_matches_the_reference_loop():
    """outofsample (LBBNN-GP-MF.py:476-496) restated with numpy on the CPU, as the reference runs it."""
    from scipy.special import expit
    from bnn_amd import evaluate
    g = torch.Generator().manual_seed(0)
    S, B, C = 10, 37, 10
    outputs = torch.log_softmax(3 * torch.randn(S, B, C, generator=g), dim=-1)
    o = outputs.numpy()
    for i in range(S):
        if i == 0:
            means = expit(o[i])
            for j in range(B):
                means[j] /= np.sum(means[j])
        else:
            tmp = expit(o[i])
            for j in range(B):
                tmp[j] /= np.sum(tmp[j])
            means = means + tmp
    means /= S
    ref = np.array([-np.sum(means[j] * np.log(means[j])) for j in range(B)])
    got = evaluate.predictive_entropy(outputs)
    assert got.shape == (B,)
    np.testing.assert_allclose(got.numpy(), ref, rtol=1e-5, atol=1e-6)
    assert (got > 0).all() and (got <= np.log(C) + 1e-5).all()
    with pytest.raises(ValueError):
        evaluate.predictive_entropy(outputs[0])


def test_python_interface_rejects_what_it_cannot_run():
    import bnn_amd
    from bnn_amd import evaluate
    torch.manual_seed(0)
    lrt = bnn_amd.lrt.BayesianNetwork((20, 16, 12, 3))
    x = torch.rand(4, 20)
    with pytest.raises(ValueError):
        evaluate.ensemble_forward(lrt, x, 3, gates="mpm")         # the median probability model is the baseline's
    with pytest.raises(ValueError):
        evaluate.ensemble_forward(lrt, x, 3, max_members=2)
    with pytest.raises(ValueError):
        evaluate.base_ensemble(lrt, x, 3)
    net = bnn_amd.base.BayesianNetwork((20, 16, 12, 3))
    with pytest.raises(ValueError):
        evaluate.ensemble_forward(net, x, 3, gates="median")
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.ensemble_forward(net, x, 3)                      # no quiet CPU fallback
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.sample_predict(x)
