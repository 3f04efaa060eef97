"""What the FusedLAMB tests share: the tests' own copy of the rule.

``lamb_rule`` is one step of LAMB as the documentation states it (README,
"LAMB"), written with plain tensor operations in the dtype asked for: float64
is the reference, float32 on the GPU the comparator.  Nothing of it is imported
from the package, and it knows nothing of the kernels' operation order."""
import math

import torch


def clip_coefficient(sq, max_norm):
    """``min(1, max_norm / (norm + 1e-6))`` from the squared norm ``sq`` (a number)."""
    return min(1.0, max_norm / (math.sqrt(sq) + 1e-6))


def lamb_rule(p, m, v, g, missing, ends, wd, lr, adapt, t, betas, eps, dtype=torch.float64, weights=None):
    """One LAMB step in ``dtype``.  ``g``: the round's mean gradient with the clip coefficient applied;
    ``missing``: the elements of count-0 chunks; ``ends``: the layers' exclusive ends; ``wd``, ``lr``,
    ``adapt``: one per layer; ``t``: the step, already advanced; ``weights``: ``(1 - b1, 1 - b2)`` where the
    caller holds them as numbers of their own (a kernel receives each rounded once from double).  Returns
    ``(p, m, v, r)``, ``r`` one ratio per layer."""
    p, m, v, g = (x.to(dtype) for x in (p, m, v, g))
    b1, b2 = betas
    w1, w2 = (1 - b1, 1 - b2) if weights is None else weights
    mn = b1 * m + w1 * g
    vn = b2 * v + w2 * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    pn = p.clone()
    ratios = []
    s = 0
    for li, e in enumerate(ends):
        pl, live = p[s:e], ~missing[s:e]
        u = (mn[s:e] / bc1) / ((vn[s:e] / bc2).sqrt() + eps) + wd[li] * pl
        np_, nu = pl[live].norm(), u[live].norm()
        r = torch.ones((), dtype=dtype, device=p.device)
        if adapt[li] and float(np_) > 0 and float(nu) > 0 and math.isfinite(float(np_)) and math.isfinite(float(nu)):
            r = np_ / nu
        pn[s:e] = torch.where(live, pl - lr[li] * r * u, pl)
        ratios.append(r)
        s = e
    return pn, torch.where(missing, m, mn), torch.where(missing, v, vn), torch.stack(ratios)
