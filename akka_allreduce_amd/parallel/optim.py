"""Momentum SGD and AdamW fused into the gradient averaging.

``GradientBucket.sgd_from`` turns a round's sum into new parameters in one
pass, for plain SGD only.  ``FusedSGD`` / ``FusedAdamW`` do the same for the
optimizers people train with: ``step_from`` runs the round and then ONE gfx950
pass over its output (``AllReduceOutput.optim_step_``) that averages by the
per-chunk counts, optionally clips by the global norm, updates the flat fp32
parameters and the optimizer state, and writes the bf16 weight shadow.  No
averaged-gradient tensor, no per-parameter optimizer kernels, no separate
shadow copy; and every buffer is allocated once, so ``GraphedDPStep`` can
capture the pass.

The updates are torch's (``torch.optim.SGD`` with dampening 0,
``torch.optim.AdamW``), with one difference a threshold allreduce needs: a
chunk that no contributor reached (count 0) is *missing*, not a zero gradient.
Its parameters, momentum, second moment and shadow stay exactly as they are,
so a parameter does not drift on stale momentum because a round dropped its
chunk.  AdamW's bias corrections use the global step for every element.

The step counter ``t`` lives on the device (one int32, advanced by an in-place
add before the pass), so a captured step advances it on every replay.  The
learning rate is a launch argument: a captured step keeps the one it was
captured with.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..data import AllReduceOutput, sqnorm_workspace
from .dp import AllreduceFn, GradientBucket


class _FusedOptimizer:
    kind = ""
    hyper: Tuple[str, ...] = ()  # the attributes ``optim_step_`` takes as keywords
    needs_round = True  # without an allreduce: the bucket's round of one contributor

    def __init__(self, bucket: GradientBucket, max_grad_norm: Optional[float]):
        if bucket.pflat is None or bucket.pflat.dtype != torch.float32 or bucket.flat.dtype != torch.float32:
            raise ValueError(f"{type(self).__name__}: needs GradientBucket(flatten_params=True) with float32 "
                             "parameters")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm={max_grad_norm}: a positive norm, or None")
        self.bucket = bucket
        self.max_grad_norm = max_grad_norm
        dev = bucket.pflat.device
        # allocated once: a captured step bakes these pointers in
        self.m = torch.zeros_like(bucket.pflat)
        self.v: Optional[torch.Tensor] = None
        self.t = torch.zeros(1, dtype=torch.int32, device=dev)
        self.norm_ws = sqnorm_workspace(dev) if max_grad_norm is not None else None

    def state_pointers(self) -> Tuple[int, ...]:
        """Addresses of everything a captured step reads or writes."""
        return tuple(0 if x is None else x.data_ptr() for x in (self.m, self.v, self.t, self.norm_ws))

    def state_tensors(self) -> Tuple[torch.Tensor, ...]:
        return tuple(x for x in (self.m, self.v, self.t) if x is not None)

    def step_from(self, allreduce: Optional[AllreduceFn], lr: float,
                  out_buf: Optional[torch.Tensor] = None) -> Optional[AllReduceOutput]:
        """Average the bucket's gradients over the contributors and apply one
        optimizer step to its flat parameters (``GradientBucket.sgd_from`` for
        this optimizer).  ``out_buf``: the round's output buffer (reused; a
        captured step needs fixed buffers).  ``allreduce=None``: this rank's
        gradients alone, as a round of one contributor."""
        return self.bucket.update_from(allreduce, lr, self, out_buf)

    def apply(self, bucket: GradientBucket, out: AllReduceOutput, lr: float, shadow: Optional[torch.Tensor]) -> None:
        """The rule of ``GradientBucket.update_from``: one fused pass over the round's output."""
        self.t.add_(1)
        out.optim_step_(self.kind, bucket.pflat, self.m, self.v, self.t, lr, shadow=shadow, max_norm=self.max_grad_norm,
                        norm_ws=self.norm_ws, **{k: getattr(self, k) for k in self.hyper})


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD(momentum, nesterov, weight_decay)`` (dampening 0) on a
    ``GradientBucket(flatten_params=True)``, fused into the averaging."""

    kind, hyper = "sgd", ("momentum", "nesterov", "weight_decay")

    def __init__(self, bucket: GradientBucket, momentum: float = 0.9, nesterov: bool = False,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None):
        if momentum < 0 or weight_decay < 0:
            raise ValueError("FusedSGD: momentum and weight_decay are >= 0")
        if nesterov and momentum <= 0:
            raise ValueError("FusedSGD: Nesterov momentum needs momentum > 0")
        super().__init__(bucket, max_grad_norm)
        self.momentum, self.nesterov, self.weight_decay = float(momentum), bool(nesterov), float(weight_decay)


class FusedAdamW(_FusedOptimizer):
    """``torch.optim.AdamW(betas, eps, weight_decay)`` on a
    ``GradientBucket(flatten_params=True)``, fused into the averaging."""

    kind, hyper = "adamw", ("betas", "eps", "weight_decay")

    def __init__(self, bucket: GradientBucket, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01, max_grad_norm: Optional[float] = None):
        if not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or eps < 0 or weight_decay < 0:
            raise ValueError("FusedAdamW: betas in [0, 1), eps and weight_decay >= 0")
        super().__init__(bucket, max_grad_norm)
        self.v = torch.zeros_like(bucket.pflat)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
