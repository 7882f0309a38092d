"""CPU tier of the multi-group Adam (lbbnn_adam_step_groups / lbbnn_grad_sumsq, bnn_amd.optim.Adam's device tables): exported
symbols, ctypes layouts against the header, argument checks that return before any HIP call, and the pure host logic
(dirty check of push_hyperparameters, chunking at the per-launch tensor limit, keyword validation)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesian-neural-nets_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "lbbnn.h")).read()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from bnn_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("lbbnn_adam_step_groups", "lbbnn_grad_sumsq", "lbbnn_grad_sumsq_workspace"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # the entry points the default optimizer used so far stay exported
    assert hasattr(lib, "lbbnn_adam_step") and hasattr(lib, "lbbnn_multi_copy")
    # argument counts of the ctypes table against the header's prototypes
    for name in ("lbbnn_adam_step_groups", "lbbnn_grad_sumsq", "lbbnn_grad_sumsq_workspace"):
        proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_ctypes_layouts_and_constants_match_the_header(tmp_path):
    from bnn_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"), "int main(void) {",
             'printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(lbbnn_adam_group_list_t), offsetof(lbbnn_adam_group_list_t, n), '
             'offsetof(lbbnn_adam_group_list_t, mask), sizeof(lbbnn_adam_hyper_t), offsetof(lbbnn_adam_hyper_t, flags), '
             'LBBNN_ADAM_GROUPS_MAX_TENSORS, LBBNN_ADAM_CHUNK, LBBNN_ADAM_F_DECOUPLED, LBBNN_ADAM_F_INACTIVE);', "return 0; }"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(_lib.AdamGroupList), _lib.AdamGroupList.n.offset, _lib.AdamGroupList.mask.offset,
                   ctypes.sizeof(_lib.AdamHyper), _lib.AdamHyper.flags.offset, _lib.ADAM_GROUPS_MAX_TENSORS, _lib.ADAM_CHUNK,
                   _lib.ADAM_F_DECOUPLED, _lib.ADAM_F_INACTIVE]
    assert ctypes.sizeof(_lib.AdamHyper) == 24
    # the list travels by value in the 4 KiB kernel-argument segment, next to one int per tensor (+1) and 48 bytes of scalars
    assert ctypes.sizeof(_lib.AdamGroupList) + 4 * (_lib.ADAM_GROUPS_MAX_TENSORS + 1) + 48 <= 4096
    # lbbnn_adam_step's own list is untouched
    assert _lib.ADAM_MAX_TENSORS == 80 and ctypes.sizeof(_lib.AdamList) == 80 * 40 + 8


def test_argument_checks_return_codes_without_a_device(lib):
    from bnn_amd import _lib
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails before a launch
    lst = _lib.AdamGroupList()
    ref = ctypes.byref(lst)
    # lbbnn_adam_step_groups
    assert lib.lbbnn_adam_step_groups(None, fake, fake, 1, None, fake, 1, None) == -1
    assert lib.lbbnn_adam_step_groups(ref, None, fake, 1, None, fake, 1, None) == -1
    assert lib.lbbnn_adam_step_groups(ref, fake, None, 1, None, fake, 1, None) == -1
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, None, 1, None) == -1          # advancing needs the ticket
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 0, None, fake, 1, None) == -2          # no group
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 65537, None, fake, 1, None) == -2
    lst.n = _lib.ADAM_GROUPS_MAX_TENSORS + 1
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, fake, 1, None) == -2
    lst.n = -1
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, fake, 1, None) == -2
    lst.n = 1
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, fake, 1, None) == -1          # tensor pointers missing
    lst.p[0] = lst.g[0] = lst.m[0] = lst.v[0] = 4096
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, fake, 1, None) == -2          # numel 0
    lst.numel[0], lst.group[0] = 10, 1
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, fake, 1, None) == -2          # group index outside the table
    lst.group[0] = -1
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, fake, 1, None) == -2
    lst.group[0], lst.v[0] = 0, None
    assert lib.lbbnn_adam_step_groups(ref, fake, fake, 1, None, fake, 1, None) == -1
    empty = _lib.AdamGroupList()
    assert lib.lbbnn_adam_step_groups(ctypes.byref(empty), fake, fake, 1, None, None, 0, None) == 0   # nothing to do, no launch
    # lbbnn_grad_sumsq
    lst.v[0] = 4096
    f = ctypes.c_float
    assert lib.lbbnn_grad_sumsq(None, fake, 0, 0, f(1.0), fake, fake, None) == -1
    assert lib.lbbnn_grad_sumsq(ref, None, 0, 0, f(1.0), fake, fake, None) == -1
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, 1, f(1.0), None, fake, None) == -1               # finalising needs norm and scale
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, 1, f(1.0), fake, None, None) == -1
    assert lib.lbbnn_grad_sumsq(ref, fake, -1, 0, f(1.0), fake, fake, None) == -2
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, -1, f(1.0), fake, fake, None) == -2
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, 2, f(1.0), fake, fake, None) == -2               # this list ends at partial 1
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, 1, f(0.0), fake, fake, None) == -2               # max_norm
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, 1, f(float("nan")), fake, fake, None) == -2
    lst.g[0] = None
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, 0, f(1.0), fake, fake, None) == -1
    lst.g[0], lst.numel[0] = 4096, 0
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, 0, f(1.0), fake, fake, None) == -2
    lst.n = _lib.ADAM_GROUPS_MAX_TENSORS + 1
    assert lib.lbbnn_grad_sumsq(ref, fake, 0, 0, f(1.0), fake, fake, None) == -2
    # workspace: the partials padded to a multiple of 64, plus the 64 column sums
    assert lib.lbbnn_grad_sumsq_workspace(0) == 64 and lib.lbbnn_grad_sumsq_workspace(1) == 128
    assert lib.lbbnn_grad_sumsq_workspace(64) == 128 and lib.lbbnn_grad_sumsq_workspace(150) == 256
    assert lib.lbbnn_grad_sumsq_workspace(-3) == 0


def _groups(n=3):
    import torch
    return [dict(params=[torch.zeros(2)], lr=1e-3 * (i + 1), betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 decoupled_weight_decay=False) for i in range(n)]


def test_dirty_check_reports_exactly_the_changes_of_the_five_values():
    from bnn_amd import _lib, optim
    groups = _groups()
    pushed = optim.hyper_values(groups)
    assert len(pushed) == 3 and pushed[1][:5] == (2e-3, 0.9, 0.999, 1e-8, 0.0) and pushed[1][5] == 0
    assert optim.hyper_dirty(None, pushed)                                 # never pushed
    assert not optim.hyper_dirty(pushed, optim.hyper_values(groups))       # nothing changed
    for gi in range(3):
        for key, val in (("lr", 0.5), ("betas", (0.8, 0.999)), ("betas", (0.9, 0.99)), ("eps", 1e-6), ("weight_decay", 0.01)):
            old = groups[gi][key]
            groups[gi][key] = val
            assert optim.hyper_dirty(pushed, optim.hyper_values(groups)), (gi, key)
            groups[gi][key] = old
            assert not optim.hyper_dirty(pushed, optim.hyper_values(groups)), (gi, key)
    # keys the kernel does not read change nothing
    groups[0]["initial_lr"] = 7.0
    groups[1]["foreach"] = True
    assert not optim.hyper_dirty(pushed, optim.hyper_values(groups))
    # the same value written again (what a scheduler does between two decays) is no change; 0.0 is a value like any other
    groups[2]["lr"] = 3e-3
    assert not optim.hyper_dirty(pushed, optim.hyper_values(groups))
    groups[2]["lr"] = 0.0
    assert optim.hyper_dirty(pushed, optim.hyper_values(groups))
    # another number of groups is a change; the flags column carries AdamW's bit and the empty-group bit
    assert optim.hyper_dirty(pushed, optim.hyper_values(_groups(4)))
    g2 = _groups(2)
    g2[0]["decoupled_weight_decay"] = True
    g2[1]["params"] = []
    assert [r[5] for r in optim.hyper_values(g2)] == [_lib.ADAM_F_DECOUPLED, _lib.ADAM_F_INACTIVE]


def test_tensors_are_chunked_at_the_new_per_launch_limit():
    from bnn_amd import _lib, optim
    assert _lib.ADAM_GROUPS_MAX_TENSORS == 64
    entries = list(range(150))
    chunks = optim.chunk_entries(entries)
    assert [len(c) for c in chunks] == [64, 64, 22] and sum(chunks, []) == entries
    assert [len(c) for c in optim.chunk_entries(list(range(64)))] == [64]
    assert [len(c) for c in optim.chunk_entries(list(range(65)))] == [64, 1]
    assert optim.chunk_entries([]) == [[]]                                 # the counters still advance: one (empty) list


def test_keyword_validation():
    import torch
    from bnn_amd import optim
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            optim.Adam(p, max_grad_norm=bad)
    with pytest.raises(NotImplementedError):
        optim.Adam(p, amsgrad=True)
    with pytest.raises(NotImplementedError):
        optim.Adam(p, maximize=True)
    with pytest.raises(ValueError):
        optim.Adam(p, lr=-1.0)
    o = optim.Adam(p, max_grad_norm=2, decoupled_weight_decay=True)
    assert o.max_grad_norm == 2.0 and o.param_groups[0]["decoupled_weight_decay"] is True
    assert optim.Adam(p).max_grad_norm is None and optim.Adam(p).param_groups[0]["decoupled_weight_decay"] is False
    with pytest.raises(ValueError):
        o.set_grad_mask(torch.nn.Parameter(torch.zeros(3)), torch.ones(3))     # not one of its parameters
    with pytest.raises(RuntimeError):
        o.step()                                                               # CPU parameters: no fallback


def test_product_sources_hold_no_forbidden_instruction_names():
    """Scalar stores to memory, scalar atomics and the scalar data-cache write-back are not used anywhere in the product
    sources (kernels, headers, Python): the names are assembled here so that this file does not contain them either."""
    words = ["s_" + w for w in ("store_dword", "buffer_store", "scratch_store", "atomic_", "buffer_atomic", "dcache_wb",
                                "dcache_discard")]
    roots = [CSRC, os.path.join(ROOT, "include"), os.path.join(ROOT, "bayesian-neural-nets_amd")]
    seen = 0
    for root in roots:
        for dirpath, _, files in os.walk(root):
            for fn in files:
                if not fn.endswith((".hip", ".h", ".py", ".cpp", ".s", ".S", "Makefile")):
                    continue
                text = open(os.path.join(dirpath, fn), errors="replace").read().lower()
                seen += 1
                for w in words:
                    assert w not in text, (fn, w)
    assert seen > 20
    adam = open(os.path.join(CSRC, "adam.hip")).read()
    assert "asm" not in adam and "atomicAdd(float" not in adam and "reduce_partials.h" in adam
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "reduce_partials.h" in mk.split("%.o:")[1].splitlines()[0]
