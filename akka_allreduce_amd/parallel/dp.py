"""Data-parallel gradient averaging on top of the threshold allreduce.

The reference is the allreduce primitive a DP trainer would call: its
``dataSource(iteration)`` / ``dataSink(sum, counts, iteration)`` pair is the
integration hook and ``count`` lets a consumer average partial (thresholded)
sums.  ``GradientBucket`` packs every parameter gradient into one
flat buffer (the grads are views into it, so there is no pack/unpack copy) and
averages with the per-element contributor counts, so a round that completed
without a straggler's contribution still yields an unbiased mean of the
gradients that did arrive.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import torch

from ..data import AllReduceOutput, Geometry

AllreduceFn = Callable[[torch.Tensor], AllReduceOutput]


class GradientBucket:
    """``flatten_params=True`` also moves the parameters into one flat buffer
    with the gradients' layout, so the SGD update fuses into the averaging
    (``sgd_from``: one pass ``p -= lr * sum / count`` on the GPU).

    ``wire_dtype=torch.bfloat16`` (fp32 gradients only) halves the bytes a
    round moves: ``average`` / ``sgd_from`` pack ``flat`` into the bf16
    ``wire`` buffer (``ops.pack_bf16``), the allreduce -- built with
    ``dtype=torch.bfloat16`` -- runs on ``wire``, and the bf16 sum is read
    straight into fp32 (``flat``, or the fused update of ``pflat``).  With
    ``error_feedback`` the fp32 ``residual`` carries what this rank's rounding
    dropped into its next step's gradient.  It does not make up for a
    contribution that a threshold round left out, nor for the owner's single
    rounding of the fp32 sum to bf16."""

    def __init__(self, params: List[torch.nn.Parameter], dtype: Optional[torch.dtype] = None,
                 flatten_params: bool = False, wire_dtype: Optional[torch.dtype] = None,
                 error_feedback: bool = True):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        dev = self.params[0].device
        dt = dtype or self.params[0].dtype
        self.numel = sum(p.numel() for p in self.params)
        if wire_dtype is not None and (wire_dtype != torch.bfloat16 or dt != torch.float32):
            raise ValueError(f"wire_dtype={wire_dtype} with {dt} gradients: only bfloat16 for float32 gradients")
        self.flat = torch.zeros(self.numel, dtype=dt, device=dev)
        self.wire_dtype = wire_dtype
        self.wire: Optional[torch.Tensor] = None
        self.residual: Optional[torch.Tensor] = None
        if wire_dtype is not None:
            self.wire = torch.empty(self.numel, dtype=wire_dtype, device=dev)
            if error_feedback:
                self.residual = torch.zeros(self.numel, dtype=dt, device=dev)
        self.pflat: Optional[torch.Tensor] = None
        # low-precision copy of pflat kept current by the fused update (use_shadow)
        self.sflat: Optional[torch.Tensor] = None
        self._shadow_on = False
        self._shadow_versions: Optional[List[int]] = None
        self.sgd = PlainSGD()
        # without an allreduce the bucket is a round of one contributor
        self._solo = AllReduceOutput(self.flat, counts_per_chunk=torch.ones((1, 1), dtype=torch.int32, device=dev),
                                     geometry=Geometry(self.numel, 1, self.numel))
        if flatten_params and all(p.dtype == dt for p in self.params):
            self.pflat = torch.empty(self.numel, dtype=dt, device=dev)
        off = 0
        for p in self.params:
            n = p.numel()
            p.grad = self.flat[off:off + n].view_as(p)
            if self.pflat is not None:
                view = self.pflat[off:off + n].view_as(p)
                view.copy_(p.data)
                p.data = view
            off += n

    def zero_(self) -> None:
        self.flat.zero_()

    def spans(self) -> List[tuple]:
        """``(offset, numel)`` of every parameter in the flat buffers, in the bucket's order."""
        out, off = [], 0
        for p in self.params:
            out.append((off, p.numel()))
            off += p.numel()
        return out

    # ---- bf16 shadow weights -------------------------------------------------
    # A bf16 forward under autocast casts every fp32 weight to bf16 each step
    # (4 B read + 2 B written per parameter).  With flattened fp32 parameters
    # the fused average + SGD pass (``count_mean`` kernel) can store the bf16
    # copy of each updated parameter as it writes it, so the next forward reads
    # that copy instead: the cast disappears from the step.
    #
    # The shadow is trusted only while nothing else touched the parameters: a
    # torch in-place op on a parameter bumps its version counter, and any
    # mismatch with the versions recorded at the last refresh re-copies the
    # shadow (our kernel writes through raw pointers and bumps none).  Writes
    # through ``p.data`` bypass the counter (torch's documented caveat): call
    # ``invalidate_shadow()`` after such writes.

    def use_shadow(self, dtype: Optional[torch.dtype]) -> bool:
        """Keep a ``dtype`` copy of the parameters current from now on (None:
        stop updating it).  Returns whether the shadow is in use."""
        ok = (dtype is not None and dtype != self.flat.dtype and self.pflat is not None
              and self.pflat.is_cuda and self.pflat.dtype == torch.float32 and dtype == torch.bfloat16
              and self.params_bound())
        if not ok:
            self._shadow_on = False
            return False
        if self.sflat is None or self.sflat.dtype != dtype:
            self.sflat = torch.empty(self.numel, dtype=dtype, device=self.pflat.device)
            self._shadow_versions = None
        if not self._shadow_on or self._shadow_versions != [p._version for p in self.params]:
            self.sflat.copy_(self.pflat)
            self._shadow_versions = [p._version for p in self.params]
        self._shadow_on = True
        return True

    def invalidate_shadow(self) -> None:
        self._shadow_versions = None

    def shadow_of(self, p: torch.nn.Parameter) -> Optional[torch.Tensor]:
        """The current low-precision copy of parameter ``p`` (None if the
        shadow is not in use)."""
        if not self._shadow_on or self.sflat is None:
            return None
        off = 0
        for q in self.params:
            if q is p:
                return self.sflat[off:off + p.numel()].view_as(p)
            off += q.numel()
        return None

    def params_bound(self) -> bool:
        """Is every parameter still its view of ``pflat``?"""
        if self.pflat is None:
            return False
        off = 0
        es = self.pflat.element_size()
        base = self.pflat.data_ptr()
        for p in self.params:
            if p.data_ptr() != base + off * es:
                return False
            off += p.numel()
        return True

    def bound(self) -> bool:
        """Is every parameter's ``.grad`` still its view of ``flat``?"""
        off = 0
        es = self.flat.element_size()
        base = self.flat.data_ptr()
        for p in self.params:
            g = p.grad
            if g is None or g.data_ptr() != base + off * es or g.shape != p.shape:
                return False
            off += p.numel()
        return True

    def rebind(self) -> bool:
        """Re-attach every ``.grad`` that is no longer a view of ``flat``
        (``zero_grad()`` sets them to ``None`` by default; an optimizer or
        user code may assign fresh tensors).  Any gradient held outside the
        bucket is copied into its view first.  Returns True if anything had
        to be re-attached."""
        if self.bound():
            return False
        off = 0
        for p in self.params:
            n = p.numel()
            view = self.flat[off:off + n].view_as(p)
            g = p.grad
            if g is None:
                view.zero_()
            elif g.data_ptr() != view.data_ptr():
                view.copy_(g)
            p.grad = view
            off += n
        return True

    def average(self, allreduce: Optional[AllreduceFn]) -> Optional[AllReduceOutput]:
        """flat <- mean over contributors (no-op without an allreduce)."""
        if allreduce is None:
            return None
        out = self._round(allreduce)
        self.average_out(out)  # one fused pass on the GPU, straight into the bucket
        return out

    def reset_residual(self) -> None:
        """Zero the error-feedback residual.  It holds rounding error of
        gradients scaled for the run so far: call this when the learning-rate
        regime changes abruptly, or after loading a checkpoint (parameters
        the residual was not accumulated against)."""
        if self.residual is not None:
            self.residual.zero_()

    def _round(self, allreduce: AllreduceFn, out_buf: Optional[torch.Tensor] = None) -> AllReduceOutput:
        """One round over the gradients, packed onto the compressed ``wire`` when there is one."""
        if self.wire is None:
            return allreduce(self.flat) if out_buf is None else allreduce(self.flat, out=out_buf)
        from ..ops.compress import pack_bf16

        if out_buf is not None and out_buf.dtype != self.wire_dtype:
            raise ValueError(f"out_buf must be {self.wire_dtype} with a compressed wire")
        pack_bf16(self.flat, self.residual, out=self.wire)
        out = allreduce(self.wire) if out_buf is None else allreduce(self.wire, out=out_buf)
        if out.data.dtype != self.wire_dtype:
            raise RuntimeError(f"the allreduce returned {out.data.dtype} for a {self.wire_dtype} wire: "
                               "build the engine with dtype=torch.bfloat16")
        return out

    def update_from(self, allreduce: Optional[AllreduceFn], lr: float, rule,
                    out_buf: Optional[torch.Tensor] = None) -> Optional[AllReduceOutput]:
        """Run the round and hand its output to ``rule`` (``self.sgd``, a ``FusedSGD`` or a ``FusedAdamW`` on this
        bucket), which updates the parameters and the shadow it is given.  Without an allreduce, None is
        returned: a rule that ``needs_round`` gets the bucket as a round of one contributor, any other gets
        None and leaves the shadow to the next ``use_shadow``."""
        out = self._solo if rule.needs_round else None
        if allreduce is not None:
            out = self._round(allreduce, out_buf)
        # A rule that may skip the step on the device (skip_nonfinite) then writes no shadow, and the host cannot
        # know: a shadow that was stale before the pass must not be marked current after it.  Current before, it
        # is current after either way: a skipped pass leaves the parameters as they were too.
        stale = getattr(rule, "guard", None) is not None and self._shadow_on \
            and self._shadow_versions != [p._version for p in self.params]
        rule.apply(self, out, lr, self.sflat if self._shadow_on else None)
        if out is not None and not stale:
            self.shadow_written()
        return None if allreduce is None else out

    def shadow_written(self) -> None:
        """An update wrote the shadow with the parameters: it is current for their versions as they are now
        (the kernels write through raw pointers and bump none; ``sgd_step``'s in-place adds bump them)."""
        if self._shadow_on:
            self._shadow_versions = [p._version for p in self.params]

    def sgd_from(self, allreduce: Optional[AllreduceFn], lr: float,
                 out_buf: Optional[torch.Tensor] = None) -> Optional[AllReduceOutput]:
        """Average the gradients over the contributors and apply SGD.  With
        flattened parameters this is one fused pass over the allreduce output
        (no averaged-gradient tensor is written).  ``out_buf``: the round's
        output buffer (reused; a captured step needs fixed buffers)."""
        return self.update_from(allreduce, lr, self.sgd, out_buf)

    def average_out(self, out: AllReduceOutput) -> None:
        if out.data.dtype == self.flat.dtype or self.wire is not None:
            out.mean(out=self.flat, dtype=self.flat.dtype)  # a compressed wire: the fp32 mean of its bf16 sum
        else:
            self.flat.copy_(out.mean().to(self.flat.dtype))

    def snapshot(self) -> tuple:
        """Copies of what an update changes, the flat parameters and the error-feedback residual, for ``restore``."""
        return tuple(None if x is None else x.clone() for x in (self.pflat, self.residual))

    def restore(self, snap: tuple) -> None:
        for x, keep in zip((self.pflat, self.residual), snap):
            if keep is not None:
                x.copy_(keep)
        if self.sflat is not None:
            self.sflat.copy_(self.pflat)
        self.shadow_written()

    def pointers(self) -> tuple:
        """Addresses of every buffer a captured step reads or writes."""
        bufs = (self.flat, self.pflat, self.sflat, self.wire, self.residual)
        return ([0 if x is None else x.data_ptr() for x in bufs],
                [p.data_ptr() for p in self.params], [0 if p.grad is None else p.grad.data_ptr() for p in self.params])


class PlainSGD:
    """The plain SGD update as a rule of ``GradientBucket.update_from`` (``bucket.sgd``): ``p -= lr * mean``,
    fused into the averaging where the parameters are flat."""

    needs_round = False  # without an allreduce: the per-parameter update of the local gradients
    state_tensors = state_pointers = staticmethod(lambda: ())  # no state

    def apply(self, b: GradientBucket, out: Optional[AllReduceOutput], lr: float,
              shadow: Optional[torch.Tensor]) -> None:
        if out is None:
            sgd_step(b.params, lr)
        elif b.pflat is not None and (b.wire is not None or out.data.dtype == b.pflat.dtype):
            # one pass into the parameters (and the bf16 shadow); a compressed wire's bf16 sum is read wide
            out.axpy_mean_(b.pflat, -lr, shadow=shadow, wide=b.wire is not None)
        else:
            b.average_out(out)
            sgd_step(b.params, lr)
            if shadow is not None:
                shadow.copy_(b.pflat)


def sgd_step(params: List[torch.nn.Parameter], lr: float) -> None:
    with torch.no_grad():
        for p in params:
            if p.grad is not None:
                p.add_(p.grad, alpha=-lr)
