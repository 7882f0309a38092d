"""Host tier of evaluate.explain_ensemble (explanations of sampled-weight members of the sparse median-probability model): the
float64 restatement of tests/sparse_explain_ref.py against torch.autograd on a dense decode of the same member weights; the
transposed-pattern builder on CPU tensors against a brute-force transpose; the refusals and the argument checks of the C entry
points that need no device; the ctypes mirrors of the new structs against the header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import explain_ref as er
import frozen_sparse_ref as sr
import sparse_explain_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bnn():
    import __graft_entry__ as ge
    import bnn_amd
    from bnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return bnn_amd


def _csrs(dims, threshold):
    lams, _ = sr.lambdals(dims, threshold)
    return [sr.csr_of(lam, sr.cut_of(threshold))[:2] for lam in lams]


# --------------------------------------------------------------------------- 1. the restatement against autograd
@pytest.mark.parametrize("case", xr.CASES, ids=xr.IDS)
def test_restatement_agrees_with_autograd(case):
    _, dims, _, _ = case
    if dims[0] > 100:
        dims = (70,) + tuple(dims[1:])                       # (the long-row case: its structure at 70 inputs, a row of 65 kept)
    csrs = _csrs(dims, 0.5)
    g = torch.Generator().manual_seed(5)
    S, B = 2, 9
    weights = [torch.randn(S, col.numel(), generator=g, dtype=torch.float64) * (4.0 / dims[i]) ** 0.5
               for i, (_, col) in enumerate(csrs)]
    biases = [torch.randn(S, dims[i + 1], generator=g, dtype=torch.float64) * 0.5 for i in range(len(csrs))]
    x = torch.randn(B, dims[0], generator=g, dtype=torch.float64).numpy()
    for m in range(S):
        Ws, bs = xr.dense_member(csrs, weights, biases, dims, m)
        masks, _ = er.relu_masks(Ws, bs, x)
        ref = xr.member_ref(Ws, bs, x, masks)
        con, logits = xr.autograd_contributions(Ws, bs, x)
        scale = np.abs(con).max()
        assert scale > 0
        assert np.abs(ref["contributions"] - con).max() <= 1e-12 * scale
        assert np.abs(ref["logits"] - logits).max() <= 1e-12 * max(np.abs(logits).max(), 1.0)
        # completeness: the terms add up to the logits
        assert np.abs(ref["logits"] - (ref["contributions"].sum(-1) + ref["intercept"])).max() <= 1e-12 * ref["terms"].max()
        t = np.arange(B) % dims[-1]
        sel = xr.member_ref(Ws, bs, x, masks, targets=t)
        assert np.array_equal(sel["contributions"][:, 0], ref["contributions"][np.arange(B), t])
        assert np.array_equal(sel["intercept"][:, 0], ref["intercept"][np.arange(B), t])
    # a feature with no kept path contributes exactly 0 (column 0 of the first layer is kept by row 1 alone, and in a layer of
    # one row by nothing)
    if dims[1] == 1:
        assert np.all(ref["contributions"][:, :, 0] == 0.0)


def test_stats_ref():
    v = np.array([[1.0, -2.0, 0.0], [3.0, -2.0, 0.0], [-1.0, -2.0, 0.0]])
    mean, std, pos, neg = xr.stats_ref(v)
    assert np.allclose(mean, [1.0, -2.0, 0.0]) and np.allclose(std, [2.0, 0.0, 0.0])
    assert pos.tolist() == [2, 0, 0] and neg.tolist() == [1, 3, 0]
    assert np.array_equal(xr.stats_ref(v[:1])[1], np.zeros(3))


# --------------------------------------------------------------------------- 2. the transposed pattern
@pytest.mark.parametrize("threshold", sr.THRESHOLDS)
@pytest.mark.parametrize("case", xr.CASES, ids=xr.IDS)
def test_transposed_pattern_equals_brute_force(bnn, case, threshold):
    _, dims, _, _ = case
    for i, (row_ptr, col) in enumerate(_csrs(dims, threshold)):
        got = bnn.ops.sparse_transposed_pattern(row_ptr, col, dims[i])
        want = xr.transpose_brute(row_ptr, col, dims[i])
        for g, w in zip(got, want):
            assert g.dtype == torch.int32 and torch.equal(g, w)
        col_ptr, trow, tslot = got
        assert col_ptr.numel() == dims[i] + 1 and int(col_ptr[-1]) == col.numel()
        assert torch.equal(col[tslot.long()].long(), torch.repeat_interleave(torch.arange(dims[i]), (col_ptr[1:] - col_ptr[:-1]).long()))
        # twice the same (the build is deterministic)
        assert all(torch.equal(a, b) for a, b in zip(got, bnn.ops.sparse_transposed_pattern(row_ptr, col, dims[i])))


def test_transposed_pattern_of_an_empty_layer(bnn):
    col_ptr, trow, tslot = bnn.ops.sparse_transposed_pattern(torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 5)
    assert col_ptr.tolist() == [0] * 6 and trow.numel() == 0 and tslot.numel() == 0


# --------------------------------------------------------------------------- 3. refusals that need no device
def test_refusals_without_a_device(bnn):
    ev = bnn.evaluate
    x = torch.zeros(2, 20)
    net = bnn.lrt.BayesianNetwork((20, 1), head="sigmoid")
    with pytest.raises(TypeError, match="sparse=True"):
        ev.explain_ensemble(net, x)
    with pytest.raises(TypeError, match="sparse=True"):
        ev.explain_ensemble(object(), x)
    with pytest.raises(TypeError, match="sparse=True"):
        ev.explain_ensemble(bnn.base.BayesianNetwork((20, 1)), x)
    fz = ev.SparseFrozenNetwork((20, 1), "lrt", head="sigmoid")
    with pytest.raises(TypeError, match="device tensor"):
        ev.explain_ensemble(fz, [[0.0] * 20])
    with pytest.raises(ValueError, match="no CPU path"):
        ev.explain_ensemble(fz, x)


def test_work_bytes(bnn):
    wb = bnn.evaluate.explain_ensemble_work_bytes
    # 100 rows pad to 128 floats a line; per member 2400 kept units, per (member, output) two G buffers of 1200 and 784 features
    assert wb((784, 1200, 1200, 10), 100, 10, 1) == 4 * 128 * 10 * (2400 + 2 * 1200 + 784)
    assert wb((20, 1), 1, 3, 1) == 4 * 64 * 3 * 20           # one layer: no activations, no G
    assert wb((8, 32, 2), 65, 3, 2) == 4 * 128 * 3 * (32 + 2 * (64 + 8))


# --------------------------------------------------------------------------- 4. the C entry points' checks
def test_entry_points_argument_checks(bnn):
    """Early returns of the four entry points (nothing is launched)."""
    from bnn_amd import _lib
    lib = _lib.lib()
    F, ODD = 4096, 4100                                      # never dereferenced
    # lbbnn_sparse_draw_members
    d = (_lib.SparseDrawDesc * 5)()
    assert lib.lbbnn_sparse_draw_members(None, 1, 1, F, 0, None) == -1
    assert lib.lbbnn_sparse_draw_members(d, 0, 1, F, 0, None) == -2
    assert lib.lbbnn_sparse_draw_members(d, 5, 1, F, 0, None) == -2          # more than LBBNN_MAX_LAYERS
    assert lib.lbbnn_sparse_draw_members(d, 1, 0, F, 0, None) == -2
    assert lib.lbbnn_sparse_draw_members(d, 1, 65536, F, 0, None) == -2
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0x1, None) == -4
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, None, 0, None) == -5
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, None, 0x2, None) == -1     # mean only: no rng needed; the layer is empty
    for k in ("col", "mean", "var", "bias_mu", "bias_var", "w", "b"):
        setattr(d[0], k, F)
    d[0].O, d[0].I, d[0].nnz, d[0].w_mstride, d[0].b_mstride = 5, 7, 9, 12, 8
    d[0].I = 0
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -2
    d[0].I, d[0].w_mstride = 7, 11
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -2          # a member's row holds whole quads
    d[0].w_mstride, d[0].b_mstride = 12, 7
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -2
    d[0].b_mstride, d[0].z, d[0].z_mstride = 8, F, 6
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -2          # z_mstride < I
    d[0].z_mstride, d[0].w = 8, 4104
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -3          # w off a 16-B boundary
    d[0].w, d[0].col = F, 4098
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -3
    d[0].col = F
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, ODD, 0, None) == -3        # rng off 8 bytes
    d[0].w = None
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -1
    d[0].w, d[0].tpos = F, F
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -1          # tpos without wt
    d[0].wt = 4098
    assert lib.lbbnn_sparse_draw_members(d, 1, 1, F, 0, None) == -3
    # lbbnn_explain_seed
    seed = dict(logits=F, targets=None, pred=1, targets_out=F, bias=F, b_mstride=12, seed=F, ld=64, intercept=F, S=3, B=5, C=10, Cp=1,
                rng_live=None, advance=0)

    def seed_call(**kw):
        return lib.lbbnn_explain_seed(*dict(seed, **kw).values(), None)
    assert seed_call(B=0, bias=None) == 0
    for k in ("bias", "seed", "intercept", "logits", "targets_out"):
        assert seed_call(**{k: None}) == -1, k
    for kw in (dict(S=0), dict(S=65536), dict(B=-1), dict(C=0), dict(ld=4), dict(Cp=10), dict(pred=0, targets_out=None, Cp=1),
               dict(pred=0, targets=F, Cp=10), dict(b_mstride=8), dict(b_mstride=-4)):
        assert seed_call(**kw) == -2, kw
    assert seed_call(targets=F) == -4
    for k in ("logits", "bias", "seed", "intercept"):
        assert seed_call(**{k: 4098}) == -3, k
    assert seed_call(targets_out=4100) == -3 and seed_call(pred=0, targets=4100) == -3 and seed_call(rng_live=4100, advance=3) == -3
    # lbbnn_sparse_gather_members
    assert lib.lbbnn_sparse_gather_members(None, None) == -1
    base = dict(ptr=F, idx=F, slot=F, w=F, w_mstride=16, bias=F, b_mstride=8, a=F, a_mstride=0, h=F, h_mstride=0, out=F,
                o_mstride=8 * 64, lda=64, ldh=64, ldo=64, B=3, K=5, N=8, nnz=9, mode=0, relu=1, out_rows=0, a_shared=0, blocks=2,
                per_member=1, dot_bias=None, dot_b_mstride=0, dot_acc=None)

    def gather(**kw):
        g = _lib.SparseGatherArgs()
        for k, v in dict(base, **kw).items():
            setattr(g, k, v)
        return lib.lbbnn_sparse_gather_members(ctypes.byref(g), None)
    assert gather(B=0, ptr=None) == 0
    assert gather(mode=3) == -4
    for k in ("ptr", "a", "out", "bias", "idx", "w"):
        assert gather(**{k: None}) == -1, k
    assert gather(mode=1, h=None) == -1 and gather(mode=2, h=None) == -1 and gather(slot=None, h=None, mode=0, B=-1) == -2
    assert gather(mode=2, slot=None, B=-1) == -2             # (the slot array is optional in every mode)
    for kw in (dict(B=-1), dict(K=0), dict(N=0), dict(nnz=-1), dict(blocks=0), dict(blocks=65536), dict(per_member=0),
               dict(blocks=3, per_member=2), dict(lda=2), dict(mode=1, ldh=2), dict(ldo=2), dict(out_rows=1, ldo=7),
               dict(w_mstride=-1), dict(o_mstride=7 * 64 + 2), dict(K=1 << 24, lda=1 << 8)):
        assert gather(**kw) == -2, kw
    for k in ("ptr", "idx", "slot", "w", "bias", "a", "h", "out"):
        assert gather(**{k: 4098}) == -3, k
    assert gather(dot_bias=F) == -1 and gather(dot_acc=F) == -1            # the bias path takes both or neither
    assert gather(dot_bias=F, dot_acc=F, a_shared=1) == -4 and gather(dot_bias=F, dot_acc=F, dot_b_mstride=-1) == -4
    assert gather(dot_bias=4098, dot_acc=F) == -3 and gather(dot_bias=F, dot_acc=4098) == -3
    # lbbnn_explain_member_stats
    assert lib.lbbnn_explain_member_stats(None, None) == -1
    sbase = dict(t=F, t_mstride=20 * 64, ldt=64, S=3, C=2, F=20, B=5, mean=F, std=F, prob_pos=F, prob_neg=F, members=None, logits=F,
                 ldl=2, n_logits=2, targets=None, intercept=F, residual=F)

    def stats(**kw):
        a = _lib.MemberStatsArgs()
        for k, v in dict(sbase, **kw).items():
            setattr(a, k, v)
        return lib.lbbnn_explain_member_stats(ctypes.byref(a), None)
    assert stats(B=0, t=None) == 0
    for k in ("t", "mean", "std", "prob_pos", "prob_neg", "logits", "intercept"):
        assert stats(**{k: None}) == -1, k
    for kw in (dict(S=0), dict(S=65536), dict(S=40000), dict(C=0), dict(F=0), dict(B=-1), dict(ldt=4), dict(t_mstride=19 * 64),
               dict(targets=F), dict(ldl=1), dict(n_logits=1, ldl=1), dict(n_logits=0)):
        assert stats(**kw) == -2, kw
    for k in ("t", "mean", "std", "prob_pos", "prob_neg", "members", "logits", "intercept", "residual"):
        assert stats(**{k: 4098}) == -3, k
    assert stats(targets=4100, C=1) == -3


def test_ctypes_struct_layouts_match_the_header(bnn, tmp_path):
    """The three structs the new entry points take have the size and the last member's offset gcc gives the header's."""
    from bnn_amd import _lib
    pairs = [("lbbnn_sparse_draw_desc_t", _lib.SparseDrawDesc, "layer_id"),
             ("lbbnn_sparse_gather_args_t", _lib.SparseGatherArgs, "dot_acc"),
             ("lbbnn_member_stats_args_t", _lib.MemberStatsArgs, "residual")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "lbbnn.h"), "int main(void) {"]
    for cname, _, last in pairs:
        lines.append('printf("%s %%zu %%zu\\n", sizeof(%s), offsetof(%s, %s));' % (cname, cname, cname, last))
    lines += ["return 0; }"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict((l.split()[0], (int(l.split()[1]), int(l.split()[2])))
               for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls, last in pairs:
        assert ctypes.sizeof(cls) == out[cname][0], cname
        assert getattr(cls, last).offset == out[cname][1], cname
    assert (_lib.GATHER_FORWARD, _lib.GATHER_SWEEP, _lib.GATHER_FINISH) == (0, 1, 2)
