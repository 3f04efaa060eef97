"""fp32 -> bf16 pack with error feedback: the sending end of a compressed
gradient wire (``GradientBucket(wire_dtype=torch.bfloat16)``, the DDP hook).

Per element ``e = g + r``, ``q = bf16(e)`` (round to nearest even),
``r = e - float(q)``: what the rounding drops this step is added to the next
step's gradient instead of being lost.  ``g + r`` and ``e - q`` are single fp32
operations, so ``float(q) + r == e`` exactly for finite values.  Where ``e`` or
``q`` is not finite the residual becomes 0 (one overflowing step does not stay
in it).

CUDA tensors always go to the native gfx950 kernel (no silent fallback: a
missing extension raises); CPU tensors use the plain torch expression, which
is also the numerics reference the GPU tests compare against.
"""
from __future__ import annotations

from typing import Optional

import torch

from .._native_loader import load as _load


def pack_bf16(g: torch.Tensor, residual: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out = bf16(g + residual)``; ``residual`` (fp32, same shape as ``g``)
    is updated in place to the rounding error.  ``residual=None``: a plain
    cast.  Returns ``out`` (allocated when not given)."""
    if g.dtype != torch.float32:
        raise TypeError(f"pack_bf16: g must be float32, got {g.dtype}")
    if out is None:
        out = torch.empty(g.shape, dtype=torch.bfloat16, device=g.device)
    for name, t, dt in (("residual", residual, torch.float32), ("out", out, torch.bfloat16)):
        if t is None:
            continue
        if t.dtype != dt:
            raise TypeError(f"pack_bf16: {name} must be {dt}, got {t.dtype}")
        if t.shape != g.shape or t.device != g.device:
            raise ValueError(f"pack_bf16: {name} must have g's shape and device")
        if not t.is_contiguous():
            raise ValueError(f"pack_bf16: {name} must be contiguous")
    if not g.is_contiguous():
        raise ValueError("pack_bf16: g must be contiguous")
    if g.device.type != "cuda":
        e = g if residual is None else g + residual
        q = e.to(torch.bfloat16)
        if residual is not None:
            f = q.float()
            residual.copy_(torch.where(torch.isfinite(f), e - f, torch.zeros_like(e)))
        out.copy_(q)
        return out
    _load().pack_bf16(out.data_ptr(), g.data_ptr(), residual.data_ptr() if residual is not None else 0, g.numel(),
                      torch.cuda.current_stream(g.device).cuda_stream)
    return out
