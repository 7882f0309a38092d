"""CPU tier of the frozen baseline model (evaluate.freeze_base / FrozenBaseNetwork; include/lbbnn.h
lbbnn_base_frozen_operands, lbbnn_base_frozen_members): the argument checks of both entry points return their documented codes
before anything is launched, the ctypes struct has the header's layout, freeze_base refuses what it cannot take with an error
that names the cause, and the evaluation stack dispatches on the new model."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E_NULL, E_SHAPE, E_ALIGN, E_FLAGS, E_NOISE = -1, -2, -3, -4, -5
SAMPLE, MPM = 0, 1
FAKE = 4096                  # a 16-B aligned address that is never dereferenced: every call below fails before launching


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def _desc(n=1, **over):
    """n descriptors of a 6 x 40 layer (ld 64) with every pointer set to FAKE."""
    from bnn_amd import _lib
    d = (_lib.BaseFrozenDesc * n)()
    for i in range(n):
        for name in ("mu", "rho", "lambdal", "bias_mu", "bias_rho", "w_mu", "w_sigma", "alpha", "e_w", "b_mu", "b_sigma",
                     "kept_rows", "alpha_rows"):
            setattr(d[i], name, FAKE)
        d[i].O, d[i].I, d[i].ld, d[i].flags, d[i].exact, d[i].layer_id = 6, 40, 64, 0, 0, 32 + i
        for k, v in over.items():
            setattr(d[i], k, v)
    return d


def _map(n=1, **over):
    from bnn_amd import _lib
    m = (_lib.CompactMap * n)()
    for i in range(n):
        m[i].rows, m[i].cols, m[i].O_full, m[i].I_full = FAKE, FAKE, 16, 48
        for k, v in over.items():
            setattr(m[i], k, v)
    return m


def _ptrs(n=1, value=FAKE):
    return (ctypes.c_void_p * n)(*([value] * n))


def test_operands_argument_checks(lib):
    ops = lambda d, m, n=1, mode=MPM, thr=0.5: lib.lbbnn_base_frozen_operands(d, m, n, mode, thr, None)
    assert ops(None, None) == E_NULL
    assert ops(_desc(), None, 0) == E_SHAPE and ops(_desc(), None, 5) == E_SHAPE
    assert ops(_desc(), None, mode=2) == E_FLAGS
    assert ops(_desc(), _map(), mode=SAMPLE) == E_FLAGS                    # alpha gates are never exactly zero
    for thr in (0.0, 1.0, -0.1, float("nan")):
        assert ops(_desc(), None, thr=thr) == E_FLAGS, thr
    for src in ("mu", "rho", "lambdal", "bias_mu", "bias_rho"):
        assert ops(_desc(**{src: None}), None) == E_NULL, src
    none = dict((k, None) for k in ("w_mu", "w_sigma", "alpha", "e_w", "b_mu", "b_sigma", "kept_rows", "alpha_rows"))
    assert ops(_desc(**none), None) == E_NULL                              # at least one output
    assert ops(_desc(keep=FAKE), _map()) == E_FLAGS                        # the keep plane is the full layer's
    assert ops(_desc(O=0), None) == E_SHAPE and ops(_desc(I=0), None) == E_SHAPE
    assert ops(_desc(ld=32), None) == E_SHAPE                              # ld < I
    assert ops(_desc(I=4100, ld=4128), None) == E_SHAPE                    # ld > 4096
    assert ops(_desc(ld=72), None) == E_ALIGN                              # ld % 32
    assert ops(_desc(flags=0x1), None) == E_FLAGS
    for plane in ("w_mu", "w_sigma", "alpha", "e_w"):
        assert ops(_desc(**{plane: FAKE + 4}), None) == E_ALIGN, plane
    for vec in ("b_mu", "b_sigma", "kept_rows", "alpha_rows", "mu", "bias_rho"):
        assert ops(_desc(**{vec: FAKE + 2}), None) == E_ALIGN, vec
    assert ops(_desc(), _map(rows=None)) == E_NULL and ops(_desc(), _map(cols=None)) == E_NULL
    assert ops(_desc(), _map(O_full=5)) == E_SHAPE and ops(_desc(), _map(I_full=39)) == E_SHAPE
    assert ops(_desc(), _map(cols=FAKE + 2)) == E_ALIGN
    # the second of two layers is checked as well
    d = _desc(2)
    d[1].ld = 72
    assert ops(d, None, 2) == E_ALIGN


def test_members_argument_checks(lib):
    def mem(d, m=None, n=1, members=3, mode=MPM, T=0.5, w="ok", b="ok", g=None, rng=FAKE):
        w = _ptrs(n) if w == "ok" else w
        b = _ptrs(n) if b == "ok" else b
        return lib.lbbnn_base_frozen_members(d, m, n, members, mode, T, w, b, g, rng, 1, None)
    assert mem(None) == E_NULL
    assert mem(_desc(), w=None) == E_NULL and mem(_desc(), b=None) == E_NULL
    assert mem(_desc(), w=_ptrs(1, None)) == E_NULL and mem(_desc(), b=_ptrs(1, None)) == E_NULL
    assert mem(_desc(), n=0) == E_SHAPE and mem(_desc(), n=5) == E_SHAPE
    assert mem(_desc(), members=0) == E_SHAPE and mem(_desc(), members=65536) == E_SHAPE
    assert mem(_desc(), mode=7) == E_FLAGS
    assert mem(_desc(), _map(), mode=SAMPLE) == E_FLAGS
    assert mem(_desc(), mode=SAMPLE, T=0.0) == E_FLAGS
    assert mem(_desc(), mode=MPM, g=_ptrs(1)) == E_FLAGS
    for plane in ("w_mu", "w_sigma", "b_mu", "b_sigma"):
        assert mem(_desc(**{plane: None})) == E_NULL, plane
    assert mem(_desc(alpha=None), mode=SAMPLE) == E_NULL
    assert mem(_desc(alpha=None), mode=MPM, rng=None) == E_NOISE           # an MPM model needs no alpha plane; rng is required
    assert mem(_desc(ld=72)) == E_ALIGN and mem(_desc(ld=32)) == E_SHAPE and mem(_desc(ld=4128, I=4100)) == E_SHAPE
    assert mem(_desc(flags=0x2)) == E_FLAGS
    assert mem(_desc(), w=_ptrs(1, FAKE + 4)) == E_ALIGN
    assert mem(_desc(), mode=SAMPLE, g=_ptrs(1, FAKE + 2)) == E_ALIGN
    assert mem(_desc(), _map(rows=None)) == E_NULL and mem(_desc(), _map(O_full=5)) == E_SHAPE
    assert mem(_desc(), rng=None) == E_NOISE


def test_ctypes_layout_matches_the_header(tmp_path):
    """lbbnn_base_frozen_desc_t as gcc lays it out from the header itself: the size and the offset of every member."""
    from bnn_amd import _lib
    fields = [f[0] for f in _lib.BaseFrozenDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"),
             "int main(void) {", 'printf("size %zu\\n", sizeof(lbbnn_base_frozen_desc_t));']
    lines += ['printf("%s %%zu\\n", offsetof(lbbnn_base_frozen_desc_t, %s));' % (f, f) for f in fields]
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict((l.split()[0], int(l.split()[1])) for l in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.BaseFrozenDesc) == out["size"]
    for f in fields:
        assert getattr(_lib.BaseFrozenDesc, f).offset == out[f], f
    assert len(out) == len(fields) + 1


def test_freeze_base_refusals():
    import bnn_amd
    from bnn_amd import base, evaluate as ev, lrt, ops
    torch.manual_seed(0)
    net = base.BayesianNetwork((12, 6, 3))
    with pytest.raises(TypeError, match="baseline LBBNN network"):
        ev.freeze_base(lrt.BayesianNetwork((12, 6, 3)))
    with pytest.raises(TypeError, match="baseline LBBNN network"):
        ev.freeze_base(torch.nn.Linear(3, 2))
    with pytest.raises(ValueError, match="gates must be"):
        ev.freeze_base(net, "alpha")
    for thr in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError, match="threshold"):
            ev.freeze_base(net, "mpm", threshold=thr)
    with pytest.raises(ValueError, match="compact=True needs gates=\"mpm\""):
        ev.freeze_base(net, "sample", compact=True)
    with pytest.raises(ValueError, match="HIP device"):
        ev.freeze_base(net)
    net.l2.noise = {"eps_w": torch.zeros(3, 6)}
    with pytest.raises(ValueError, match="layer 2 has injected noise"):
        ev.freeze_base(net, "mpm")
    net.l2.noise = None
    wide = base.BayesianNetwork((ops.GATE_MEMBERS_MAX_LD + 1, 2))
    with pytest.raises(ValueError, match="layer 1: in_features = %d" % (ops.GATE_MEMBERS_MAX_LD + 1)):
        ev.freeze_base(wide)
    # freeze() keeps refusing a baseline network, and the new names are exported
    with pytest.raises(TypeError):
        ev.freeze(net)
    assert bnn_amd.freeze_base is ev.freeze_base and bnn_amd.FrozenBaseNetwork is ev.FrozenBaseNetwork


def test_model_constructor_and_surface():
    from bnn_amd import evaluate as ev
    fz = ev.FrozenBaseNetwork((12, 6, 3), "mpm", 0.4)
    assert fz.dims == fz.full_dims == (12, 6, 3) and fz.n_layers == 2 and fz.gates == "mpm" and fz.threshold == 0.4
    assert fz.head == "log_softmax" and not fz.compact and list(fz.parameters()) == []
    assert [tuple(k.shape) for k in fz.kept_rows] == [(6,), (3,)]
    with pytest.raises(RuntimeError, match="belongs to a compact model"):
        fz.live
    with pytest.raises(RuntimeError, match="not bound"):
        fz.refresh()
    live = [torch.tensor([1, 2, 7, 9, 10, 14, 17, 22], dtype=torch.int32), torch.arange(8, dtype=torch.int32),
            torch.arange(3, dtype=torch.int32)]
    cp = ev.FrozenBaseNetwork((24, 16, 3), "mpm", live=live, needed=[8, 5, 3])
    assert cp.compact and cp.dims == (8, 8, 3) and cp.full_dims == (24, 16, 3) and cp.needed == [8, 5, 3]
    assert torch.equal(cp.live[0], live[0]) and "full_dims=(24, 16, 3)" in repr(cp)
    with pytest.raises(NotImplementedError, match="freeze again"):
        cp.refresh()
    with pytest.raises(ValueError, match="gates"):
        ev.FrozenBaseNetwork((12, 6, 3), "alpha")
    with pytest.raises(ValueError, match="compact model needs"):
        ev.FrozenBaseNetwork((24, 16, 3), "sample", live=live, needed=[8, 5, 3])
    with pytest.raises(ValueError, match="boundaries"):
        ev.FrozenBaseNetwork((24, 16, 3), "mpm", live=live[:2], needed=[8, 5])


def test_the_stack_dispatches_on_the_new_model():
    """_is_frozen accepts the model, and ensemble_forward / ensemble_eval / evaluate_batches / make_graphed_eval_step take its
    frozen branch: a stub records the calls (no device)."""
    from bnn_amd import base, evaluate as ev, graphs
    calls = []

    class Stub(ev.FrozenBaseNetwork):
        density = 0.25

        def ensemble(self, data, samples=10, *, max_members=None, log_probs=False, keep_weights=False):
            calls.append(("ensemble", samples, max_members, log_probs))
            return torch.zeros(samples, data.shape[0], 2 if log_probs else self.dims[-1]).log_softmax(-1)

        def forward(self, data, sample=False, *, log_probs=False):
            calls.append(("forward", sample, log_probs))
            return torch.zeros(data.shape[0], 2 if log_probs else self.dims[-1]).log_softmax(-1)

    fz = Stub((12, 6, 3), "mpm")
    assert ev._is_frozen(fz) and not ev._is_frozen(base.BayesianNetwork((12, 6, 3))) and not ev._is_base(fz)
    x, y = torch.rand(4, 12), torch.tensor([0, 1, 2, 0])
    out = ev.ensemble_forward(fz, x, 5, max_members=2)
    assert out.shape == (5, 4, 3) and calls == [("ensemble", 5, 2, False)]
    with pytest.raises(ValueError, match="frozen model"):
        ev.ensemble_forward(fz, x, 5, gates="mpm")
    del calls[:]
    r = ev.ensemble_eval(fz, x, y, 5)
    assert calls == [("ensemble", 5, None, False), ("forward", False, False)]
    assert r["density"].tolist() == [0.25] * 5 and r["pred_posterior_mean"].shape == (4,)
    # a one-unit sigmoid head is two classes
    del calls[:]
    fb = Stub((12, 6, 1), "sample", head="sigmoid")
    ev.ensemble_eval(fb, x, torch.tensor([0., 1., 1., 0.]), 2)
    assert calls == [("ensemble", 2, None, True), ("forward", False, True)]
    # the graphed step takes it past the type check (and then asks for HIP tensors); anything else is a TypeError
    with pytest.raises(RuntimeError, match="HIP tensors"):
        graphs.make_graphed_eval_step(fz, x, y, 5, None)
    with pytest.raises(TypeError, match="frozen model"):
        graphs.make_graphed_eval_step(base.BayesianNetwork((12, 6, 3)), x, y, 5, None)
