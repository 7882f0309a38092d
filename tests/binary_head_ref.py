"""Restatement of the four binary-head formulas of include/lbbnn.h (lbbnn_binary_head, lbbnn_elbo_bce_loss,
lbbnn_elbo_bce_loss_backward, lbbnn_sigmoid_backward) in torch CPU ops: float64 for the error bars of the GPU tests, and
``dtype=torch.float32`` for the statement that the formulas ARE torch's (tests/test_binary_head_host.py holds the float32 form
against torch.sigmoid + nn.BCELoss(reduction='sum') autograd on the saturation vector).  Every function takes anything
``torch.as_tensor`` takes and returns CPU tensors of ``dtype``."""
import torch

# logits at which the float32 forms saturate: p == 1.0f from x >= 17 (a loss term of exactly 100 against y = 0, a logit gradient of
# exactly 0), p underflows to 0 below -104, the 1e-12 floor of the backward's denominator is reached from |x| ~ 28
SATURATION = torch.tensor([-110, -40, -20, -17, -3, -1e-3, 0, 1e-3, 0.5, 3, 16, 17, 20, 40, 110], dtype=torch.float32)
SATURATION_TARGETS = (torch.arange(SATURATION.numel()) % 2).to(torch.float32)          # 0, 1, 0, 1, ...
FLOOR = 1e-12                                          # as a float32 value in every dtype (the kernel's 1e-12f)


def _t(a, dtype):
    return torch.as_tensor(a).detach().cpu().to(dtype)


def sigmoid(x, dtype=torch.float64):
    x = _t(x, dtype)
    return 1.0 / (1.0 + torch.exp(-x))


def logp2(x, dtype=torch.float64):
    """(.., 2): [logsigmoid(-x), logsigmoid(x)] with logsigmoid(x) = min(x, 0) - log1p(exp(-|x|)), from the logit."""
    x = _t(x, dtype)
    t = torch.log1p(torch.exp(-x.abs()))
    return torch.stack([torch.clamp(-x, max=0) - t, torch.clamp(x, max=0) - t], dim=-1)


def target_ok(y):
    y = torch.as_tensor(y).detach().cpu()
    return (y >= 0) & (y <= 1)                        # False for NaN


def bce_terms(p, y, dtype=torch.float64):
    """Per element (y - 1) max(log1p(-p), -100) - y max(log p, -100) -- -(y log p + (1 - y) log(1 - p)) as torch's
    binary_cross_entropy spells it; 0 where the target is outside [0, 1] or not finite."""
    p, y = _t(p, dtype), _t(y, dtype)
    ok = target_ok(y)
    ys = torch.where(ok, y, torch.zeros_like(y))
    lp = torch.clamp(torch.log(p), min=-100)
    lq = torch.clamp(torch.log1p(-p), min=-100)
    t = (ys - 1) * lq - ys * lp
    return torch.where(ok, t, torch.zeros_like(t))


def loss(p, y, kl=None, kl_scale=1.0):
    """float64: sum of the terms + kl * kl_scale."""
    return float(bce_terms(p, y).sum()) + (0.0 if kl is None else float(kl) * float(kl_scale))


def stats(p, y):
    """[correct, elements, bad_targets, nonfinite_probs] as lbbnn_elbo_bce_loss counts them (p, y: the float32 values)."""
    p, y = _t(p, torch.float32), _t(y, torch.float32)
    ok = target_ok(y)
    correct = ((p > 0.5) == (y > 0.5)) & ok
    return [int(correct.sum()), int(p.numel()), int((~ok).sum()), int((~torch.isfinite(p)).sum())]


def backward(g, p, y, kl_scale=1.0, dtype=torch.float64):
    """(g_probs, g_logits, g_kl): g (p - y) / max((1 - p) p, 1e-12), g_probs ((1 - p) p), g kl_scale; zeros at bad targets."""
    p, y, g = _t(p, dtype), _t(y, dtype), _t(g, dtype)
    ok = target_ok(y)
    d = (1 - p) * p
    floor = torch.tensor(FLOOR, dtype=torch.float32).to(dtype)
    gp = g * (p - y) / torch.maximum(d, floor)
    gl = gp * d
    zero = torch.zeros_like(gp)
    return torch.where(ok, gp, zero), torch.where(ok, gl, zero), g * torch.tensor(kl_scale, dtype=torch.float32).to(dtype)


def sigmoid_backward(g, p, dtype=torch.float64):
    p, g = _t(p, dtype), _t(g, dtype)
    return g * ((1 - p) * p)
