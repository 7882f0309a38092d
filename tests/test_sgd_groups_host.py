"""CPU tier of the multi-group SGD (lbbnn_sgd_step_groups, bnn_amd.optim.SGD's device table): the symbol is declared, exported
and bound, the ctypes mirror of the table row matches the header, the argument checks return before any HIP call, and the pure
host logic (table rows, dirty check, keyword validation)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def test_symbol_is_declared_exported_and_bound(lib):
    from bnn_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbbnn.h")).read(), flags=re.S)
    name = "lbbnn_sgd_step_groups"
    assert re.search(r"\b%s\s*\(" % name, src)
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1])
    # the same argument list as the Adam entry point it is modelled on
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES["lbbnn_adam_step_groups"]


def test_hyper_row_layout_and_flags_match_the_header(tmp_path):
    from bnn_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"), "int main(void) {",
             'printf("%zu %zu %zu %d %d\\n", sizeof(lbbnn_sgd_hyper_t), offsetof(lbbnn_sgd_hyper_t, flags), '
             'offsetof(lbbnn_sgd_hyper_t, dampening), LBBNN_SGD_F_NESTEROV, LBBNN_SGD_F_INACTIVE);', "return 0; }"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(_lib.SgdHyper), _lib.SgdHyper.flags.offset, _lib.SgdHyper.dampening.offset,
                   _lib.SGD_F_NESTEROV, _lib.SGD_F_INACTIVE]
    assert ctypes.sizeof(_lib.SgdHyper) == 20 and _lib.SgdHyper.flags.offset == 16
    assert _lib.SGD_F_INACTIVE == _lib.ADAM_F_INACTIVE        # one advance routine reads the bit of either table


def test_argument_checks_return_codes_without_a_device(lib):
    from bnn_amd import _lib
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails before a launch
    lst = _lib.AdamGroupList()
    ref = ctypes.byref(lst)
    f = lib.lbbnn_sgd_step_groups
    assert f(None, fake, fake, 1, None, fake, 1, None) == -1
    assert f(ref, None, fake, 1, None, fake, 1, None) == -1
    assert f(ref, fake, None, 1, None, fake, 1, None) == -1
    assert f(ref, fake, fake, 1, None, None, 1, None) == -1          # advancing needs the ticket
    assert f(ref, fake, fake, 0, None, fake, 1, None) == -2          # no group
    assert f(ref, fake, fake, 65537, None, fake, 1, None) == -2
    lst.n = _lib.ADAM_GROUPS_MAX_TENSORS + 1
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -2
    lst.n = -1
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -2
    lst.n = 1
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -1          # tensor pointers missing
    lst.p[0] = 4096
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -1          # g
    lst.p[0], lst.g[0] = None, 4096
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -1          # p
    lst.p[0] = 4096                                                  # m and v stay NULL: no momentum buffer, v is never read
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -2          # numel 0
    lst.numel[0] = -5
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -2
    lst.numel[0], lst.group[0] = 10, 1
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -2          # group index outside the table
    lst.group[0] = -1
    assert f(ref, fake, fake, 1, None, fake, 1, None) == -2
    lst.group[0] = 2
    assert f(ref, fake, fake, 2, None, fake, 0, None) == -2
    empty = _lib.AdamGroupList()
    assert f(ctypes.byref(empty), fake, fake, 1, None, None, 0, None) == 0   # nothing to do, no launch
    # the Adam entry point still asks for both moments of the same list
    lst.group[0] = 0
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, fake, 1, None) == -1


def _groups(n=3):
    import torch
    return [dict(params=[torch.zeros(2)], lr=1e-3 * (i + 1), momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False)
            for i in range(n)]


def test_hyper_values_rows_and_dirty_check():
    from bnn_amd import _lib, optim
    groups = _groups()
    pushed = optim.sgd_hyper_values(groups)
    assert len(pushed) == 3 and pushed[1] == (2e-3, 0.9, 0.0, 0.0, 0)
    assert optim.hyper_dirty(None, pushed)
    assert not optim.hyper_dirty(pushed, optim.sgd_hyper_values(groups))
    for gi in range(3):
        for key, val in (("lr", 0.5), ("momentum", 0.5), ("dampening", 0.1), ("weight_decay", 0.01), ("nesterov", True)):
            old = groups[gi][key]
            groups[gi][key] = val
            assert optim.hyper_dirty(pushed, optim.sgd_hyper_values(groups)), (gi, key)
            groups[gi][key] = old
            assert not optim.hyper_dirty(pushed, optim.sgd_hyper_values(groups)), (gi, key)
    groups[0]["initial_lr"] = 7.0                       # keys the kernel does not read change nothing
    groups[1]["foreach"] = True
    assert not optim.hyper_dirty(pushed, optim.sgd_hyper_values(groups))
    groups[2]["lr"] = 0.0                               # the study's switch: 0.0 is a value like any other
    assert optim.hyper_dirty(pushed, optim.sgd_hyper_values(groups))
    assert optim.hyper_dirty(pushed, optim.sgd_hyper_values(_groups(4)))
    g2 = _groups(2)
    g2[0]["nesterov"] = True
    g2[1]["params"] = []
    assert [r[4] for r in optim.sgd_hyper_values(g2)] == [_lib.SGD_F_NESTEROV, _lib.SGD_F_INACTIVE]
    assert optim.SGD._COLS == 5 and optim.Adam._COLS == 6 and optim.SGD._hyper_values is optim.sgd_hyper_values


def test_keyword_validation_and_group_keys():
    import torch
    from bnn_amd import optim
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        optim.SGD(p, lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)       # as torch: Nesterov needs zero dampening
    with pytest.raises(ValueError):
        optim.SGD(p, lr=0.1, momentum=0.0, nesterov=True)                      # ... and a momentum
    with pytest.raises(ValueError):
        torch.optim.SGD(p, lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(NotImplementedError):
        optim.SGD(p, lr=0.1, maximize=True)
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-3)):
        with pytest.raises(ValueError):
            optim.SGD(p, **kw)
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            optim.SGD(p, lr=0.1, max_grad_norm=bad)
    with pytest.raises(TypeError):
        optim.SGD(p, lr=0.1, foreach=True)                                     # not a keyword here
    o = optim.SGD(p, 0.1, 0.9, 0, 1e-4, True, max_grad_norm=2)
    assert o.max_grad_norm == 2.0
    ref = torch.optim.SGD(p, 0.1, 0.9, 0, 1e-4, True)
    assert set(o.param_groups[0]) == set(ref.param_groups[0])                  # torch's group keys: state dicts interchange
    assert {k: v for k, v in o.param_groups[0].items() if k != "params"} == \
           {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    ref.load_state_dict(o.state_dict())
    with pytest.raises(ValueError):
        o.set_grad_mask(torch.nn.Parameter(torch.zeros(3)), torch.ones(3))
    p[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError):
        o.step()                                                               # CPU parameters: no fallback
