"""GPU tier: the two keep rules of the sparse models' one count / pack kernel (csrc/csr_pack.h) stay two.

An LRT / MNF model keeps ``lambdal > logit(threshold)``, a baseline model ``sigmoid(lambdal) > threshold`` in fp32.  Every other
test's lambdal lies at least 1e-3 from the cut, where the rules agree; here it sits on the boundary of threshold 0.5 (cut 0.0).
For |x| <= 1e-8 the sum 1 + expf(-x) rounds to exactly 2 in fp32 (for any expf within an ulp), so sigmoid is exactly 0.5 and the
baseline rule DROPS +1e-8, which ``lambdal > 0`` keeps; at +-1e-6 the sum is one fp32 step from 2 and the rules agree.

One layer, I = 70 (a full 64-column step and a partial one), O = 5 (a partial workgroup of four rows, O % 4 != 0); lambdal cycles
through VALUES along the flattened (O, I) weights, so every value appears in both column steps of every row."""
import pytest
import torch

import frozen_sparse_ref as sr

pytestmark = pytest.mark.gpu

DIMS = (70, 5)
VALUES = (1e-8, -1e-8, 1e-6, -1e-6, 1.0, -1.0)


@pytest.fixture(scope="module")
def patterns():
    import bnn_amd
    bnn_amd.set_precision("fp32")
    ev = bnn_amd.evaluate
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    O, I = DIMS[1], DIMS[0]
    lam = torch.tensor(VALUES, dtype=torch.float32).repeat(O * I // len(VALUES) + 1)[:O * I].view(O, I)
    for v in VALUES:                                          # every value in both column steps of every row
        assert bool((lam[:, :64] == v).any(1).all()) and bool((lam[:, 64:] == v).any(1).all())
    torch.manual_seed(5)
    lrt = bnn_amd.lrt.BayesianNetwork(DIMS).to(dev).eval()
    base = bnn_amd.base.BayesianNetwork(DIMS).to(dev).eval()
    with torch.no_grad():
        base._layers()[0].weight_mu.copy_(torch.randn(O, I, generator=torch.Generator().manual_seed(6)) + 3.0)
    assert bool((base._layers()[0].weight_mu != 0).all())
    sr.apply(lrt, [lam])
    sr.apply(base, [lam])
    decode = lambda csr: sr.decode(csr[0].cpu(), csr[1].cpu(), torch.ones(csr[1].numel()), O, I) > 0
    return dict(lam=lam, lrt=ev.freeze(lrt, "mpm", sparse=True).csr(0), sweep=ev.threshold_sweep(lrt, (0.5, 0.9)).model(0).csr(0),
                base=ev.freeze_base(base, "mpm", sparse=True).csr(0),
                dense=ev.freeze_base(base, "mpm")._buf("w_mu", 0)[:, :I].cpu(),       # (the plane's rows are padded)
                decode=decode)


def test_lrt_rule_keeps_lambdal_above_the_cut(patterns):
    """``freeze(net, "mpm", sparse=True)`` keeps exactly ``lambdal > 0`` -- +1e-8 included -- and level 0 of a sweep is that CSR."""
    want_ptr, want_col, keep = sr.csr_of(patterns["lam"], sr.cut_of(0.5))
    assert torch.equal(keep, patterns["lam"] > 0)
    row_ptr, col = patterns["lrt"][:2]
    assert torch.equal(row_ptr.cpu(), want_ptr) and torch.equal(col.cpu(), want_col)
    assert torch.equal(patterns["sweep"][0], row_ptr) and torch.equal(patterns["sweep"][1], col)


def test_base_rule_keeps_sigmoid_above_the_threshold(patterns):
    """``freeze_base(net, "mpm", sparse=True)`` keeps exactly {+1e-6, +1}: the nonzero pattern of the dense ``freeze_base(net,
    "mpm")``; it differs from the LRT rule's pattern exactly at the +1e-8 columns."""
    lam = patterns["lam"]
    got = patterns["decode"](patterns["base"])
    assert torch.equal(got, (lam == VALUES[2]) | (lam == VALUES[4]))
    assert torch.equal(got, patterns["dense"] != 0)
    assert torch.equal(got != patterns["decode"](patterns["lrt"]), lam == VALUES[0])
