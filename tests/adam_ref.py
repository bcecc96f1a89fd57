"""Referee of the native Adam (gsn_amd/optim.py, csrc/optim.hip): the formulas of torch.optim.Adam (amsgrad=False, maximize=False)
restated per tensor in float64, with the scale against which the error of each output is read.  The scales are absolute: ``m`` cancels
when gradient and momentum disagree, so an error relative to the result would say nothing."""
import math

import torch


def adam_ref(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay, decoupled):
    """One update of one tensor.  ``t``: the number of this step (the tensor's counter + 1).  Returns ``((p, m, v), (sp, sm, sv))``,
    float64 tensors: the new values and the normalisation scale of each."""
    p, g, m, v = (x.detach().to("cpu", torch.float64) for x in (p, g, m, v))
    lr, beta1, beta2, eps, weight_decay, t = float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), float(t)
    if decoupled:
        p0, gp = p * (1.0 - lr * weight_decay), g
    else:
        p0, gp = p, g + weight_decay * p
    a, b = beta1 * m, (1.0 - beta1) * gp
    m1 = a + b
    v1 = beta2 * v + (1.0 - beta2) * gp * gp
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    p1 = p0 - (lr / bc1) * m1 / denom
    sm = a.abs() + b.abs()
    return (p1, m1, v1), (p.abs() + (lr / bc1) * sm / denom, sm, v1)


def normalised_error(x, ref, scale):
    """max |x - ref| / scale over the tensor (0 for an empty one; an element whose scale is 0 must be exact)."""
    if ref.numel() == 0:
        return 0.0
    d = (x.detach().to("cpu", torch.float64) - ref).abs()
    e = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    return float(e.max())
