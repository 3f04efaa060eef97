"""User I/O contract (reference: ``DataWrapper.scala:3-7``).

``AllReduceInputRequest(iteration)`` -> ``AllReduceInput(data)`` is the data
source; ``AllReduceOutput(data, count, iteration)`` goes to the data sink.

``count`` is the per-element contributor count of the reference
(ReducedDataBuffer.getWithCounts, RB:26-53).  It is carried compactly as one
count per (block, chunk) and expanded to one int32 per element only when the
``count`` attribute is first read (a gfx950 kernel on GPU), so a sink that
never looks at counts does not pay an extra S-element int32 write per round.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Any, Optional

import torch


@dataclass(frozen=True)
class Geometry:
    """Block/chunk layout (W:240-250 with exact integer arithmetic)."""

    dataSize: int
    workerNum: int
    maxChunkSize: int

    @property
    def step(self) -> int:
        return (self.dataSize + self.workerNum - 1) // self.workerNum

    def block_range(self, j: int) -> tuple[int, int]:
        s = min(j * self.step, self.dataSize)
        e = self.dataSize if j >= self.workerNum - 1 else min((j + 1) * self.step, self.dataSize)
        return s, e

    def block_len(self, j: int) -> int:
        s, e = self.block_range(j)
        return e - s

    def num_chunks(self, j: int) -> int:
        return -(-self.block_len(j) // self.maxChunkSize)

    @functools.cached_property
    def kmax(self) -> int:
        return max(1, max(self.num_chunks(j) for j in range(self.workerNum)))

    @functools.cached_property
    def total_chunks(self) -> int:
        return sum(self.num_chunks(j) for j in range(self.workerNum))

    def chunk_range(self, j: int, k: int) -> tuple[int, int]:
        s, e = self.block_range(j)
        cs = s + k * self.maxChunkSize
        return cs, min(cs + self.maxChunkSize, e)

    def expand_counts(self, per_chunk: torch.Tensor) -> torch.Tensor:
        """[N, kmax] counts -> [S] per-element counts (torch reference path)."""
        per_chunk = per_chunk.reshape(self.workerNum, self.kmax)
        idx = torch.arange(self.dataSize, device=per_chunk.device, dtype=torch.int64)
        step = max(self.step, 1)
        blk = torch.clamp(idx // step, max=self.workerNum - 1)
        k = (idx - blk * step) // self.maxChunkSize
        return per_chunk.reshape(-1)[blk * self.kmax + k].to(torch.int32)


DTYPE_NAME = {torch.float32: "float32", torch.bfloat16: "bfloat16"}  # the native module's dtype names


def counts_table(per_chunk: torch.Tensor, g: Geometry) -> tuple:
    """The counts-table argument of the native count passes, behind the contiguous counts tensor it points
    into: hold that until the call returns."""
    pc = per_chunk.contiguous()
    return pc, (pc.data_ptr(), g.dataSize, g.step, g.workerNum, g.maxChunkSize, g.kmax)


def sqnorm_workspace(device) -> torch.Tensor:
    """Workspace of ``AllReduceOutput.sqnorm`` (the global-norm clip of
    ``optim_step_``): the result, the kernel's ticket and one partial per
    workgroup.  Zeroed once here; every pass leaves the ticket zero again, so
    one workspace serves every step, and every replay of a captured one."""
    device = torch.device(device)
    n = 0
    if device.type == "cuda":
        from ._native_loader import load

        n = load().count_sqnorm_partials()
    return torch.zeros(2 + n, dtype=torch.float32, device=device)


def lamb_workspace(numel: int, layers: int, device) -> torch.Tensor:
    """Workspace of ``optim_step_(kind="lamb")``: the norm pass's partial sums,
    one pair of floats (``sum p^2``, ``sum u^2``) per slot and ``tiles + layers``
    slots, the tile length being the native module's (``lamb_tile``).  Every
    slot that is read is written by the same step first, so it is allocated
    once and never reset.  The torch path on the CPU keeps no partials: one
    pair per layer."""
    device = torch.device(device)
    tiles = 0
    if device.type == "cuda":
        from ._native_loader import load

        tiles = -(-int(numel) // load().lamb_tile())
    return torch.zeros(2 * (tiles + int(layers)), dtype=torch.float32, device=device)


def guard_state(device) -> torch.Tensor:
    """The guard record of ``optim_step_(guard=...)`` / ``sqnorm(guard=...)``:
    int32[4] on ``device``, zeroed once.  ``[0]``: 1 if the last pass was
    applied, 0 if it was skipped; ``[1]``: steps skipped in total; ``[2]``:
    steps skipped in a row; ``[3]``: reserved, 0."""
    return torch.zeros(4, dtype=torch.int32, device=torch.device(device))


def _mul32(x: torch.Tensor, c: int) -> torch.Tensor:
    """``x * c`` modulo 2^32 on int64 values below 2^32 (no int64 overflow: the constant in two 16-bit halves)."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & 0xFFFFFFFF


def _mix32(x: torch.Tensor) -> torch.Tensor:
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def sr_bits(n: int, t: torch.Tensor, seed: int, device=None) -> tuple:
    """The 16 rounding bits of ``m`` and of ``v`` for the elements ``0 .. n-1`` at device step ``t`` (int64
    tensors), as the bf16-state pass of ``optim_step_`` draws them: ``key = mix(seed ^ mix(t))``,
    ``h = mix(lo32(i) ^ (hi32(i) * 0x9e3779b9) ^ key)``, ``m`` takes ``h & 0xffff`` and ``v`` ``h >> 16``
    (torch integer ops, int64 masked to 32 bits; the definition is in ``csrc/kernels/optim.hip``)."""
    h = _sr_hash(n, t, seed, device)
    return h & 0xFFFF, h >> 16


def _sr_hash(n: int, t: torch.Tensor, seed: int, device=None) -> torch.Tensor:
    """``h(i)`` of ``sr_bits`` for the elements ``0 .. n-1`` (int64 values below 2^32)."""
    device = t.device if device is None else device
    key = _mix32((_mix32(t.reshape(()).to(device=device, dtype=torch.int64) & 0xFFFFFFFF)) ^ int(seed))
    i = torch.arange(n, dtype=torch.int64, device=device)
    return _mix32((i & 0xFFFFFFFF) ^ _mul32((i >> 32) & 0xFFFFFFFF, 0x9E3779B9) ^ key)


def sr_bits_p(n: int, t: torch.Tensor, seed: int, device=None) -> torch.Tensor:
    """The 16 rounding bits of a bfloat16 ``p`` for the elements ``0 .. n-1`` at device step ``t`` (an int64
    tensor): ``h2 & 0xffff`` with ``h2 = mix(h ^ 0x85ebca6b)``, a second hash of the ``h`` of ``sr_bits`` --
    ``m`` and ``v`` use all 32 bits of ``h`` itself."""
    return _mix32(_sr_hash(n, t, seed, device) ^ 0x85EBCA6B) & 0xFFFF


def sr_bf16(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """fp32 ``x`` rounded stochastically to bfloat16 with the 16 bits ``r`` (int64): the upper half of
    ``bits(x) + r`` where ``x`` is finite, round-to-nearest (which keeps NaN and inf) elsewhere."""
    bits = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    up = (bits + r) >> 16
    up = torch.where(up >= 0x8000, up - 0x10000, up).to(torch.int16).view(torch.bfloat16)
    return torch.where(torch.isfinite(x), up, x.to(torch.bfloat16))


class OptimGroups:
    """Parameter groups of ``AllReduceOutput.optim_step_(groups=...)``: the
    flat buffer cut into segments and one row of scalars per group, all in
    device memory so the update reads them when it RUNS (a captured step
    follows whatever the rows hold at each replay).

    ``seg_end``: ascending exclusive ends of the segments (the last one is the
    buffer's size); ``seg_group``: each segment's group.  ``rows`` is float32
    ``[groups, 4]`` = ``{-lr_g, wd_g, lr_g, 1 - lr_g * wd_g}``, each computed
    in double and rounded once (``row_values``); ``write_rows`` uploads them
    with one stream-ordered copy on the current stream."""

    __slots__ = ("seg_end", "seg_group", "rows", "host_seg_end", "host_seg_group", "ngroups", "numel")

    def __init__(self, seg_end, seg_group, ngroups: int, device):
        self.host_seg_end = [int(e) for e in seg_end]
        self.host_seg_group = [int(g) for g in seg_group]
        self.ngroups = int(ngroups)
        prev = 0
        for e, g in zip(self.host_seg_end, self.host_seg_group):
            if e <= prev:
                raise ValueError(f"OptimGroups: segment ends must be positive and ascending, got {self.host_seg_end}")
            if not 0 <= g < self.ngroups:
                raise ValueError(f"OptimGroups: group {g} is outside [0, {self.ngroups})")
            prev = e
        if not self.host_seg_end or len(self.host_seg_end) != len(self.host_seg_group):
            raise ValueError("OptimGroups: one group per segment, at least one segment")
        self.numel = prev
        device = torch.device(device)
        self.seg_end = torch.tensor(self.host_seg_end, dtype=torch.int64, device=device)
        self.seg_group = torch.tensor(self.host_seg_group, dtype=torch.int32, device=device)
        self.rows = torch.zeros((self.ngroups, 4), dtype=torch.float32, device=device)  # allocated once

    @staticmethod
    def row_values(lr: float, group_hyper) -> torch.Tensor:
        """The rows of ``[(lr_scale, weight_decay)]`` at learning rate ``lr``, as a CPU tensor."""
        rows = []
        for scale, wd in group_hyper:
            lr_g = float(lr) * float(scale)
            rows.append([-lr_g, float(wd), lr_g, 1.0 - lr_g * float(wd)])
        return torch.tensor(rows, dtype=torch.float64).to(torch.float32)

    def write_rows(self, values: torch.Tensor) -> None:
        if values.shape != self.rows.shape or values.dtype != torch.float32:
            raise ValueError(f"OptimGroups: rows are float32 {tuple(self.rows.shape)}")
        if self.rows.is_cuda:
            # pinned staging from torch's caching host allocator: the copy is ordered on the current stream and
            # the block is not reused before it ran
            self.rows.copy_(values.pin_memory(), non_blocking=True)
        else:
            self.rows.copy_(values)

    def expand(self, column: int) -> torch.Tensor:
        """One column of the rows as a per-element vector (the torch path of ``optim_step_``)."""
        ends = torch.tensor(self.host_seg_end, dtype=torch.int64, device=self.rows.device)
        lens = torch.diff(ends, prepend=ends.new_zeros(1))
        return torch.repeat_interleave(self.rows[:, column][self.seg_group.long()], lens)


@dataclass
class AllReduceInputRequest:
    iteration: int


@dataclass
class AllReduceInput:
    data: Any


class AllReduceOutput:
    """Reduced vector of one round + contributor counts.

    ``data``: 1-D tensor of ``dataSize`` elements (sum over contributors;
    chunks that did not reach the completion threshold are 0).
    ``count``: int32 tensor, per-element contributor count (0 where missing).
    ``iteration``: the round.
    """

    __slots__ = ("data", "iteration", "counts_per_chunk", "geometry", "_count", "_expander", "_event")

    def __init__(
        self,
        data: torch.Tensor,
        count: Optional[torch.Tensor] = None,
        iteration: int = 0,
        *,
        counts_per_chunk: Optional[torch.Tensor] = None,
        geometry: Optional[Geometry] = None,
        expander: Any = None,
        event: Any = None,
    ):
        self.data = data
        self.iteration = iteration
        self.counts_per_chunk = counts_per_chunk
        self.geometry = geometry
        self._count = count
        self._expander = expander
        self._event = event

    @classmethod
    def _make(cls, data: torch.Tensor, iteration: int, counts_per_chunk: torch.Tensor, geometry: "Geometry",
              expander: Any, event: Any) -> "AllReduceOutput":
        """The engine's per-round constructor: positional, no keyword parsing
        (one of these per round; small rounds are priced by their host path)."""
        o = cls.__new__(cls)
        o.data, o.iteration, o.counts_per_chunk, o.geometry = data, iteration, counts_per_chunk, geometry
        o._count, o._expander, o._event = None, expander, event
        return o

    def wait(self) -> "AllReduceOutput":
        """Async rounds: make the current stream wait for the result (no-op otherwise)."""
        if self._event is not None:
            torch.cuda.current_stream(self.data.device).wait_event(self._event)
        return self

    @property
    def count(self) -> torch.Tensor:
        self.wait()
        if self._count is None:
            if self.counts_per_chunk is None or self.geometry is None:
                raise ValueError("AllReduceOutput has no count information")
            if self._expander is not None:
                self._count = self._expander(self.counts_per_chunk)
            else:
                self._count = self.geometry.expand_counts(self.counts_per_chunk)
        return self._count

    def _feeds_count_pass(self) -> bool:
        """Can this sum feed a native count pass (per-chunk counts not yet expanded, 16-B aligned)?"""
        d = self.data
        return (d.is_cuda and d.dtype in DTYPE_NAME and d.is_contiguous() and d.data_ptr() % 16 == 0
                and self.counts_per_chunk is not None and self.geometry is not None and self._count is None)

    def _flat_ok(self, t: torch.Tensor, dtype: torch.dtype, wide: bool = False, align: int = 16) -> bool:
        """Can the flat tensor ``t`` be a destination, state or shadow of a count pass over this sum?
        ``wide``: ``t`` takes the fp32 mean of a bf16 sum."""
        d = self.data
        return (t.dtype == dtype and (not wide or self._is_wide(dtype)) and t.is_contiguous()
                and t.device == d.device and t.numel() == d.numel() and t.data_ptr() % align == 0)

    def _count_mean(self, dst: torch.Tensor, axpy: bool, alpha: float, shadow: Optional[torch.Tensor] = None) -> None:
        from ._native_loader import load

        d = self.data
        pc, table = counts_table(self.counts_per_chunk, self.geometry)
        load().count_mean(dst.data_ptr(), d.data_ptr(), table, DTYPE_NAME[dst.dtype],
                          torch.cuda.current_stream(d.device).cuda_stream, axpy, float(alpha),
                          shadow.data_ptr() if shadow is not None else 0, DTYPE_NAME[d.dtype])

    def _is_wide(self, dst_dtype: torch.dtype) -> bool:
        return self.data.dtype == torch.bfloat16 and dst_dtype == torch.float32

    def axpy_mean_(self, y: torch.Tensor, alpha: float, shadow: Optional[torch.Tensor] = None, *,
                   wide: bool = False) -> torch.Tensor:
        """``y += alpha * mean()`` in one fused pass on the GPU (the SGD update
        of a flat parameter buffer: alpha = -lr); ``y`` is updated in place.
        ``shadow`` (bf16, same length as fp32 ``y``) also receives the updated
        values, stored by the same pass (a separate cast off the fused path).
        ``wide=True`` with fp32 ``y`` and a bf16 sum (a compressed wire) uses
        the fp32 mean of the sum, not its bf16 rounding: the same single pass
        on the GPU, reading bf16 and writing fp32."""
        self.wait()
        wide = wide and self._is_wide(y.dtype)
        if self._feeds_count_pass() and self._flat_ok(y, torch.float32 if wide else self.data.dtype, wide) and (
                shadow is None or (y.dtype == torch.float32 and self._flat_ok(shadow, torch.bfloat16))):
            self._count_mean(y, True, alpha, shadow)
            return y
        m = self.mean(dtype=torch.float32) if wide else self.mean()
        y.add_(m.view_as(y).to(y.dtype), alpha=alpha)
        if shadow is not None:
            shadow.copy_(y.view_as(shadow))
        return y

    def optim_step_(self, kind: str, p: torch.Tensor, m: torch.Tensor, v: Optional[torch.Tensor], t: torch.Tensor,
                    lr: float, *, weight_decay: float = 0.0, momentum: float = 0.0, nesterov: bool = False,
                    betas: tuple = (0.9, 0.999), eps: float = 1e-8, shadow: Optional[torch.Tensor] = None,
                    max_norm: Optional[float] = None, norm_ws: Optional[torch.Tensor] = None,
                    nt: bool = False, groups: Optional[OptimGroups] = None, seed: int = 0,
                    guard: Optional[torch.Tensor] = None, lamb_ws: Optional[torch.Tensor] = None,
                    trust: Optional[torch.Tensor] = None,
                    layer_adapt: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimizer step of the flat fp32 parameters ``p`` from this
        round, in one fused pass on the GPU: per element ``g = sum / count``,
        then ``kind="sgd"`` (``torch.optim.SGD``: weight decay into ``g``,
        ``m = momentum * m + g``, Nesterov or not, dampening 0) or
        ``kind="adamw"`` (``torch.optim.AdamW``: decoupled decay, ``m`` / ``v``
        with the bias corrections of step ``t``).  ``m`` and ``v`` are the
        flat fp32 state (``v`` only for AdamW); ``t`` is the step, one int32 on
        ``p``'s device, already advanced for this step by the caller.  A bf16
        sum (a compressed wire) is read wide into fp32.  ``shadow`` (bf16)
        receives the updated parameters from the same pass.

        ``max_norm`` clips by the global norm as ``clip_grad_norm_`` does:
        ``g`` is scaled by ``min(1, max_norm / (norm + 1e-6))``, the norm taken
        over the mean gradient of this round (one extra pass over the sum into
        ``norm_ws``, see ``sqnorm``) and read on the device, no host sync.

        A chunk whose count is 0 is MISSING, not zero: its ``p``, ``m``, ``v``
        and ``shadow`` stay exactly as they are (stale momentum must not move a
        parameter whose gradient a threshold round dropped); the bias
        corrections still use the global ``t``.

        CUDA tensors always go to the native kernel, under the conditions of
        ``axpy_mean_``'s fused pass (anything else raises); CPU tensors run the
        same formulas as torch operations.  ``nt`` streams with nontemporal
        accesses instead of plain ones (slower where measured: kept for
        ``bench/fused_opt.py``).

        ``groups`` (``OptimGroups``) gives every segment its group's learning
        rate and weight decay, read from the groups' device rows when the pass
        runs, in place of ``lr`` and ``weight_decay`` (``nt`` is ignored).  A
        group whose learning rate is 0 advances ``m`` / ``v`` and leaves ``p``
        where it is; the shadow is still written.

        ``m`` and ``v`` may be bfloat16 instead (both, never one): they are
        widened exactly, the update runs in fp32 as above, ``p`` and the
        shadow come from the unrounded new moments, and only the stores of
        ``m`` and ``v`` are rounded -- stochastically (``sr_bf16``), with the
        bits of ``sr_bits``: a function of the element's index, ``t`` and
        ``seed`` alone (the definition is at the top of the bf16 code in
        ``csrc/kernels/optim.hip``), so ranks that share a seed round alike
        and a replayed capture draws new bits each time.  ``nt`` is not
        offered with bfloat16 state.

        ``p`` may be bfloat16 as well (a model trained in pure bf16: ``p`` is
        the weight the forward reads), with bfloat16 ``m`` / ``v``, no
        ``shadow`` and no ``nt``; anything else raises.  ``p`` is widened
        exactly, everything above runs in fp32 on the widened value (LAMB's
        ``||p||`` included), ``m`` and ``v`` get the bits they would get from
        an fp32 ``p`` of that value, and only the store of ``p`` is rounded:
        ``sr_bf16(p_new, r)`` with the 16 bits of ``sr_bits_p``, a second hash
        of the same (index, ``t``, ``seed``).  Nearest rounding would not do:
        a step of ``lr * u = 1e-4`` at ``p = 1`` is 1/39 of a bf16 ulp and
        would never move the parameter.  An element whose fp32 result equals
        its old value (a zero update, a group at ``lr == 0``) keeps its bits.

        ``guard`` (``guard_state``) skips a step whose gradient is not finite,
        on the device.  The norm pass then runs whether or not there is a clip
        (``norm_ws`` is required) and judges the step by ``sq``, the squared
        global norm of the round's mean gradient over the elements whose count
        is > 0: the step is APPLIED iff ``sq`` is a finite fp32 number.  A NaN
        or an inf in a chunk that has a contributor, or a finite gradient whose
        squared norm overflows, makes it a SKIPPED step: ``p``, ``m``, ``v``,
        ``shadow`` and ``t`` keep their bits, and the record counts it
        (``guard_state``).  With a guard ``t`` is advanced BY THE PASS, and only
        for an applied step: the caller passes the step before this one and
        does not advance it, so the bias corrections and the rounding bits of a
        run with a skipped step are those of a run in which that round never
        happened.  A non-finite value inside a count-0 chunk is never read and
        skips nothing.

        ``kind="lamb"``: AdamW's ``m`` and ``v`` (the same operations, the
        same bits), then ``u = (m / bc1) / (sqrt(v / bc2) + eps) + wd * p`` and
        ``p -= lr * r * u`` with one trust ratio ``r`` per LAYER.  It needs
        ``groups`` with one segment per layer (``lr`` and the decay come from
        their rows), ``trust`` (float32, one per segment: the pass writes the
        ratios there and the update reads them), ``layer_adapt`` (int32, one
        per segment: 0 pins that layer's ``r`` to 1) and ``lamb_ws``
        (``lamb_workspace``).  ``r = ||p|| / ||u||`` where both norms are
        positive and finite, else 1; both norms run over the layer's elements
        whose count is > 0 (``p`` before the step), so a missing chunk enters
        neither and a layer without a contributor keeps ``r = 1``.  On the GPU
        three kernels: the norm pass (fixed tiles, one partial pair per tile
        and layer, no atomics), one workgroup per layer that sums them in a
        fixed order, and the update -- the same bits for the same inputs on
        every call, no host sync, nothing to reset.  ``nt`` is refused.
        Returns ``p``."""
        self.wait()
        if kind not in ("sgd", "adamw", "lamb"):
            raise ValueError(f"optim_step_: kind={kind!r} (sgd, adamw or lamb)")
        lamb = kind == "lamb"
        adam = kind == "adamw" or lamb  # a second moment and the bias corrections
        d = self.data
        if d.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"optim_step_: a float32 or bfloat16 sum, not {d.dtype}")
        state =[("m", m)] + ([("v", v)] if adam else [])
        sdt = m.dtype if m is not None else torch.float32
        if sdt not in (torch.float32, torch.bfloat16):
            raise ValueError(f"optim_step_: m and v are float32 or bfloat16, not {sdt}")
        if adam and v is not None and v.dtype != sdt:
            raise ValueError(f"optim_step_: m is {sdt} and v is {v.dtype}; they must agree")
        bf_state = sdt == torch.bfloat16
        if bf_state and nt:
            raise ValueError("optim_step_: nt=True is not offered with bfloat16 state")
        pdt = p.dtype if p is not None else torch.float32
        if pdt not in (torch.float32, torch.bfloat16):
            raise ValueError(f"optim_step_: p is float32 or bfloat16, not {pdt}")
        bf_param = pdt == torch.bfloat16
        if bf_param and not bf_state:
            raise ValueError(f"optim_step_: bfloat16 p needs bfloat16 m and v, not {sdt}")
        if bf_param and shadow is not None:
            raise ValueError("optim_step_: no shadow with bfloat16 p (p is the bf16 weight itself)")
        if bf_param and nt:
            raise ValueError("optim_step_: nt=True is not offered with bfloat16 p")
        seed = int(seed)
        if not 0 <= seed < 1 << 32:
            raise ValueError(f"optim_step_: seed={seed} is not an unsigned 32-bit value")
        for name, s, dt in [("p", p, pdt)] + [(n, s, sdt) for n, s in state]:
            if s is None or not self._flat_ok(s, dt, align=1):
                raise ValueError(f"optim_step_: {name} must be contiguous {str(dt)[6:]} of the round's size and "
                                 "device")
        if shadow is not None and not self._flat_ok(shadow, torch.bfloat16, align=1):
            raise ValueError("optim_step_: shadow must be contiguous bfloat16 of p's size and device")
        if t.dtype != torch.int32 or t.numel() != 1 or t.device != p.device:
            raise ValueError("optim_step_: t is one int32 on p's device")
        if max_norm is not None and norm_ws is None:
            raise ValueError("optim_step_: max_norm needs a norm workspace (sqnorm_workspace)")
        if guard is not None and norm_ws is None:
            raise ValueError("optim_step_: a guard needs a norm workspace (sqnorm_workspace): the norm pass gives "
                             "the verdict")
        if groups is not None and (groups.numel != d.numel() or groups.rows.device != d.device):
            raise ValueError(f"optim_step_: the groups cover {groups.numel} elements on {groups.rows.device}, the "
                             f"round has {d.numel()} on {d.device}")
        if lamb:
            if nt:
                raise ValueError("optim_step_: nt=True is not offered with kind='lamb'")
            if groups is None:
                raise ValueError("optim_step_: kind='lamb' needs groups, one segment per layer")
            nseg = len(groups.host_seg_end)
            for name, x, dt in (("trust", trust, torch.float32), ("layer_adapt", layer_adapt, torch.int32)):
                if x is None or x.dtype != dt or x.shape != (nseg,) or x.device != d.device or not x.is_contiguous():
                    raise ValueError(f"optim_step_: kind='lamb' needs {name}, contiguous {str(dt)[6:]} [{nseg}] "
                                     "(one per segment) on the round's device")
            # the size: the launcher checks it against its tiles; the torch path uses none of it
            if lamb_ws is None or lamb_ws.dtype != torch.float32 or lamb_ws.device != d.device \
                    or not lamb_ws.is_contiguous():
                raise ValueError("optim_step_: kind='lamb' needs lamb_ws, a float32 workspace from lamb_workspace "
                                 "on the round's device")
        if d.is_cuda:
            if not (self._feeds_count_pass() and self._flat_ok(p, pdt)
                    and all(self._flat_ok(s, sdt) for _, s in state)
                    and (shadow is None or self._flat_ok(shadow, torch.bfloat16))):
                raise ValueError("optim_step_: the fused pass needs a float32 or bfloat16 sum with its per-chunk "
                                 "counts (not expanded) and 16-B aligned buffers")
            from ._native_loader import load

            # with a guard the norm pass always runs: it writes the verdict and advances t for an applied step
            sq = None
            if guard is not None:
                sq = self.sqnorm(norm_ws, guard, t)
            elif max_norm is not None:
                sq = self.sqnorm(norm_ws)
            pc, table = counts_table(self.counts_per_chunk, self.geometry)
            # the tables stay alive in `groups` until the call returns; nt is not offered with groups
            gr = None if groups is None else (groups.seg_end.data_ptr(), groups.seg_group.data_ptr(),
                                              groups.rows.data_ptr(), groups.host_seg_end, groups.host_seg_group,
                                              groups.ngroups)
            # a guard without a clip: the pass still takes sq, and an infinite max_norm makes its coefficient
            # exactly 1
            mx = max_norm if max_norm is not None else (math.inf if guard is not None else 0.0)
            stream = torch.cuda.current_stream(d.device).cuda_stream
            pk = {"param_dtype": DTYPE_NAME[pdt]} if bf_param else {}  # fp32 p: the calls as they always were
            if lamb:
                # the layers' norms, then their ratios; the launcher checks the workspace's size
                nat, slots = load(), lamb_ws.numel() // 2
                if lamb_ws.data_ptr() % 8:
                    raise ValueError("optim_step_: lamb_ws must be 8-B aligned")
                nat.lamb_norms(lamb_ws.data_ptr(), slots, p.data_ptr(), m.data_ptr(), v.data_ptr(), d.data_ptr(),
                               DTYPE_NAME[d.dtype], table, t.data_ptr(), sq.data_ptr() if sq is not None else 0, gr,
                               stream, beta1=betas[0], beta2=betas[1], eps=eps, max_norm=mx,
                               state_dtype=DTYPE_NAME[sdt], guard=guard.data_ptr() if guard is not None else 0,
                               **pk)
                nat.lamb_trust(trust.data_ptr(), lamb_ws.data_ptr(), slots, gr, d.numel(), layer_adapt.data_ptr(),
                               stream, guard.data_ptr() if guard is not None else 0)
            load().count_optim(kind, p.data_ptr(), m.data_ptr(), v.data_ptr() if adam else 0,
                               shadow.data_ptr() if shadow is not None else 0, d.data_ptr(), DTYPE_NAME[d.dtype],
                               table, t.data_ptr(), sq.data_ptr() if sq is not None else 0,
                               stream, bool(nt) and groups is None, lr=lr,
                               weight_decay=weight_decay, momentum=momentum, nesterov=nesterov, beta1=betas[0],
                               beta2=betas[1], eps=eps, max_norm=mx,
                               state_dtype=DTYPE_NAME[sdt], seed=seed, groups=gr,
                               guard=guard.data_ptr() if guard is not None else 0,
                               trust=trust.data_ptr() if lamb else 0, **pk)
            return p
        # the same formulas as torch operations (count-0 elements keep everything)
        sq = None
        if guard is not None:
            # the verdict first: an applied step advances t before the bias corrections and the rounding bits
            # read it, a skipped one touches nothing else
            sq = self.sqnorm(norm_ws, guard, t)
            if int(guard[0]) == 0:
                return p
        elif max_norm is not None:
            sq = self.sqnorm(norm_ws)
        keep = (self.count <= 0).view_as(p)
        g = self.mean(dtype=torch.float32) if d.dtype != torch.float32 else self.mean()
        g = g.view_as(p)
        if bf_state:
            # widened exactly; the formulas run in fp32 and only what is stored into m and v is rounded
            m_st, v_st, m, v = m, v, m.float(), v.float() if adam else None
            r_m, r_v = sr_bits(p.numel(), t, seed, p.device)
        p_st = p
        if bf_param:
            # likewise: the formulas see the widened p, and only what is stored into p is rounded
            p, r_p = p.float(), sr_bits_p(p.numel(), t, seed, p.device)
        if max_norm is not None:
            g = g * torch.clamp(max_norm / (sq.sqrt() + 1e-6), max=1.0)
        # the scalars as the kernel receives them, each rounded to fp32 once: a group's rows expanded to
        # per-element vectors, or 0-dim values for the whole buffer
        if groups is not None:
            neg_lr, wd, lr_v, decay = (groups.expand(c).view_as(p) for c in range(4))
        else:
            neg_lr, wd, lr_v, decay = OptimGroups.row_values(lr, [(1.0, weight_decay)])[0].to(p.device)
        if lamb:
            b1, b2 = betas
            tf = t.to(torch.float32)
            mn = torch.lerp(m, g, 1 - b1)
            vn = (v * b2).addcmul_(g, g, value=1 - b2)
            # u as the kernel spells it: (m * (1 / bc1)) / (sqrt(v) / sqrt(bc2) + eps), then wd * p fused in
            u = torch.addcmul((mn * (1 - b1 ** tf).reciprocal()) / (vn.sqrt() / (1 - b2 ** tf).sqrt()).add_(eps),
                              p, wd)
            # the layers' squared norms over the elements that have a contributor
            ends = torch.tensor(groups.host_seg_end, dtype=torch.int64, device=p.device)
            lens = torch.diff(ends, prepend=ends.new_zeros(1))
            layer = torch.repeat_interleave(torch.arange(len(lens), device=p.device), lens)
            zero = torch.zeros_like(p)
            pp = torch.zeros(len(lens), device=p.device).index_add_(0, layer, torch.where(keep, zero, p * p))
            uu = torch.zeros(len(lens), device=p.device).index_add_(0, layer, torch.where(keep, zero, u * u))
            ok = (pp > 0) & (uu > 0) & torch.isfinite(pp) & torch.isfinite(uu) & (layer_adapt != 0)
            trust.copy_(torch.where(ok, pp.sqrt() / uu.sqrt(), torch.ones_like(pp)))
            pn = p
            step = torch.addcmul(p, u, -(lr_v * trust[layer]))
        elif adam:
            b1, b2 = betas
            tf = t.to(torch.float32)
            pn = p * decay
            mn = torch.lerp(m, g, 1 - b1)
            vn = (v * b2).addcmul_(g, g, value=1 - b2)
            # p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps), bc_k = 1 - b_k^t, with the step size folded
            # into the denominator as AdamW(capturable=True) and the kernel spell it; both quotients as the
            # kernel's reciprocal times the numerator (what float / tensor computes, not tensor / tensor)
            nss = -((1 - b1 ** tf).reciprocal() * lr_v)
            step = pn.addcdiv(mn, (vn.sqrt() / ((1 - b2 ** tf).sqrt() * nss)).add_(nss.reciprocal() * eps))
        else:
            g = torch.addcmul(g, p, wd)
            mn = (m * momentum).add_(g)
            pn = p
            step = torch.addcmul(p, g.add(mn, alpha=momentum) if nesterov else mn, neg_lr)
        # a group at lr 0: the state advances, p only takes its decay (AdamW's step is 0 / -0 at v = 0)
        pn = torch.where(lr_v != 0, step, pn) if groups is not None else step
        if bf_state:
            m_st.copy_(torch.where(keep, m_st, sr_bf16(mn, r_m.view_as(mn))))
            if adam:
                v_st.copy_(torch.where(keep, v_st, sr_bf16(vn, r_v.view_as(vn))))
        else:
            m.copy_(torch.where(keep, m, mn))
            if adam:
                v.copy_(torch.where(keep, v, vn))
        if bf_param:
            p_st.copy_(torch.where(keep, p_st, sr_bf16(pn, r_p.view_as(pn))))
            return p_st
        p.copy_(torch.where(keep, p, pn))
        if shadow is not None:
            shadow.copy_(torch.where(keep.view_as(shadow), shadow, p.view_as(shadow).to(shadow.dtype)))
        return p

    def sqnorm(self, ws: torch.Tensor, guard: Optional[torch.Tensor] = None,
               t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Squared global norm of this round's mean gradient: the sum over the
        elements whose count is > 0 of ``(sum / count) ** 2``, in fp32, as a
        one-element view of the workspace ``ws`` (``sqnorm_workspace``).  On
        the GPU one pass over the sum (fp32 or bf16), deterministic for a
        given shape; no host sync.

        ``guard`` (``guard_state``) and ``t`` (the step, one int32), both or
        neither: the pass also judges the step.  A finite result: ``guard[0] =
        1``, ``guard[2] = 0`` and ``t += 1``.  Otherwise ``guard[0] = 0``,
        ``guard[1] += 1``, ``guard[2] += 1`` and ``t`` stays.  The result has
        the same bits with and without a guard."""
        self.wait()
        d = self.data
        if ws.dtype != torch.float32 or ws.device != d.device or not ws.is_contiguous():
            raise ValueError("sqnorm: the workspace is float32 on the round's device (sqnorm_workspace)")
        if (guard is None) != (t is None):
            raise ValueError("sqnorm: a guard and the step t, both or neither")
        if guard is not None:
            if (guard.dtype != torch.int32 or guard.numel() != 4 or guard.device != d.device
                    or not guard.is_contiguous()):
                raise ValueError("sqnorm: the guard is int32[4] on the round's device (guard_state)")
            if t.dtype != torch.int32 or t.numel() != 1 or t.device != d.device:
                raise ValueError("sqnorm: t is one int32 on the round's device")
        if d.is_cuda:
            from ._native_loader import load

            nat = load()
            if not (self._feeds_count_pass() and ws.numel() >= 2 + nat.count_sqnorm_partials()):
                raise ValueError("sqnorm: needs a 16-B aligned float32 or bfloat16 sum with its per-chunk counts "
                                 "and a workspace from sqnorm_workspace")
            pc, table = counts_table(self.counts_per_chunk, self.geometry)
            # [0]: the result, [1]: the ticket (zero bits), [2:]: one partial per workgroup
            nat.count_sqnorm(ws.data_ptr(), d.data_ptr(), DTYPE_NAME[d.dtype], table, ws.data_ptr() + 8,
                             ws.data_ptr() + 4, torch.cuda.current_stream(d.device).cuda_stream,
                             guard.data_ptr() if guard is not None else 0, t.data_ptr() if t is not None else 0)
            return ws[:1]
        g = self.mean(dtype=torch.float32) if d.dtype != torch.float32 else self.mean()
        ws[0] = (g * g).sum()
        if guard is not None:
            if bool(torch.isfinite(ws[0])):
                guard[0] = 1
                guard[2] = 0
                t.add_(1)
            else:
                guard[0] = 0
                guard[1] += 1
                guard[2] += 1
        return ws[:1]

    def mean(self, out: Optional[torch.Tensor] = None, *, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """Element-wise average over the contributors that made it (0 where none).

        On the GPU this is one fused pass (``count_mean`` kernel: each element
        divided by its chunk's count from the tiny per-chunk table) instead of
        expanding per-element counts; ``out`` may be any same-shape tensor,
        including the buffer that was reduced (gradient buckets).
        ``dtype=torch.float32`` on a bf16 sum gives the fp32 mean (the division
        in fp32, no second rounding to bf16), into an fp32 ``out`` if given."""
        self.wait()
        d = self.data
        if dtype is not None and dtype != d.dtype:
            if not self._is_wide(dtype):
                raise ValueError(f"mean: dtype={dtype} from {d.dtype} data (only float32 from bfloat16)")
            if out is not None and out.dtype != dtype:
                raise ValueError(f"mean: out must be {dtype}")
            dst = torch.empty(d.shape, dtype=dtype, device=d.device) if out is None else out
            if self._feeds_count_pass() and self._flat_ok(dst, dtype, True):
                self._count_mean(dst, False, 0.0)
                return dst
            c = self.count.to(dtype)
            m = torch.where(c > 0, d.to(dtype) / c.clamp(min=1), torch.zeros_like(c))
            dst.copy_(m.view_as(dst))
            return dst
        if d.is_cuda:
            dst = torch.empty_like(d) if out is None else out
            if self._feeds_count_pass() and self._flat_ok(dst, d.dtype):
                self._count_mean(dst, False, 0.0)
                return dst
        c = self.count.to(d.dtype if d.is_floating_point() else torch.float32)
        m = torch.where(c > 0, d / c.clamp(min=1), torch.zeros_like(d))
        if out is None:
            return m
        out.copy_(m.view_as(out))
        return out

    def __repr__(self) -> str:  # pragma: no cover - debugging aid
        return f"AllReduceOutput(iteration={self.iteration}, n={self.data.numel()}, dtype={self.data.dtype})"
