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
add before the pass), so a captured step advances it on every replay.

Built plainly, an optimizer has one weight decay for the whole buffer and its
learning rate is a launch argument: a captured step keeps the one it was
captured with.  ``param_groups=`` (per-group ``weight_decay`` and ``lr_scale``)
or ``device_lr=True`` move both into a small device table, one row per group,
that the pass reads when it runs (``data.OptimGroups``): biases and norm
scales can stay out of the decay, and ``set_lr`` between two replays of a
captured step changes its learning rate.  Betas, eps, momentum and the clip
norm stay per optimizer.

``state_dtype=torch.bfloat16`` keeps the moments ``m`` and ``v`` in bf16: half
the optimizer memory and 8 (AdamW) or 4 (SGD) bytes per element less for the
pass to move.  The pass widens them, updates in fp32, takes the parameters and
the shadow from the unrounded moments and rounds only what it stores into
``m`` and ``v`` -- stochastically, because a nearest-rounded bf16 ``v`` stops
moving (docs/DESIGN.md).  The rounding bits are a function of the element's
index, the device step and ``seed``: every rank must use the same seed (the
default, 0, is), or their parameters drift apart.

A bucket of bf16 parameters and bf16 gradients (``model.to(torch.bfloat16)``)
is taken as well, with ``state_dtype=torch.bfloat16`` (it must be given: the
default stays float32).  The parameter then is the bf16 weight the forward
reads: no fp32 copy, no shadow, 14 instead of 20 bytes per element for AdamW's
pass.  The pass widens ``p``, computes exactly what it computes for fp32
parameters of those values and rounds only the store of ``p`` -- stochastically
again, since a nearest-rounded bf16 parameter never moves by a step that is a
small part of its ulp -- with bits from a second hash of the same index, device
step and ``seed``.  The rule above therefore now covers ``p`` itself: the seed
must be the same on every rank.  ``param_dtype`` tells which kind of bucket the
optimizer was built on; ``state_dict()`` carries it.

``skip_nonfinite=True`` drops a bad step on the device.  The norm pass (which
then runs with or without a clip) judges the round by the squared global norm
of its mean gradient: finite, and the step is applied; a NaN, an inf or an
overflowing norm, and the update pass returns before its first load --
parameters, moments, shadow and ``t`` keep their bits, and a small device
record counts the skip (``skipped_steps``, ``skipped_in_a_row``,
``last_step_applied``).  The norm pass, not ``apply``, then advances ``t``, and
only for an applied step, so a run with a skipped step continues exactly as a
run in which that round never happened -- eager and on every replay of a
captured step.  ``FusedSGD(momentum=0, skip_nonfinite=True)`` is the guarded
plain SGD (``bucket.sgd`` itself has no norm pass to judge by).

``FusedLAMB`` adds the layer-wise adaptive rate large global batches want:
AdamW's moments, and per parameter of the bucket a trust ratio ``||p|| /
||u||`` computed on the device by a deterministic pass in front of the update
(its docstring has the rule).  It keeps everything above: the missing-chunk
semantics (a missing chunk enters no norm), the clip, the guard, bf16 moments,
the device-resident learning rate, capture.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch

from ..data import AllReduceOutput, OptimGroups, guard_state, lamb_workspace, sqnorm_workspace
from .dp import AllreduceFn, GradientBucket

_GROUP_KEYS = ("params", "weight_decay", "lr_scale")
_STATE_DTYPES = (torch.float32, torch.bfloat16)
_PARAM_DTYPES = (torch.float32, torch.bfloat16)


class _FusedOptimizer:
    kind = ""
    hyper: Tuple[str, ...] = ()  # the attributes ``optim_step_`` takes as keywords
    group_keys: Tuple[str, ...] = _GROUP_KEYS  # what a ``param_groups`` entry may hold
    merge_segments = True  # adjacent parameters of one group are one segment
    needs_round = True  # without an allreduce: the bucket's round of one contributor

    def __init__(self, bucket: GradientBucket, max_grad_norm: Optional[float],
                 state_dtype: torch.dtype = torch.float32, seed: int = 0, skip_nonfinite: bool = False):
        if bucket.pflat is None or bucket.pflat.dtype not in _PARAM_DTYPES or bucket.flat.dtype != bucket.pflat.dtype:
            raise ValueError(f"{type(self).__name__}: needs GradientBucket(flatten_params=True) with float32 "
                             "parameters and gradients, or bfloat16 ones (both, not a mix)")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm={max_grad_norm}: a positive norm, or None")
        if state_dtype not in _STATE_DTYPES:
            raise ValueError(f"{type(self).__name__}: state_dtype={state_dtype} (torch.float32 or torch.bfloat16)")
        if bucket.pflat.dtype == torch.bfloat16 and state_dtype != torch.bfloat16:
            raise ValueError(f"{type(self).__name__}: a GradientBucket(flatten_params=True) with bfloat16 parameters "
                             "keeps its moments in bfloat16 too; pass state_dtype=torch.bfloat16")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 32:
            raise ValueError(f"{type(self).__name__}: seed={seed!r}, an integer in [0, 2**32)")
        if not isinstance(skip_nonfinite, bool):
            raise ValueError(f"{type(self).__name__}: skip_nonfinite={skip_nonfinite!r}, True or False")
        self.bucket = bucket
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self.state_dtype, self.seed = state_dtype, seed
        self._param_dtype = bucket.pflat.dtype
        dev = bucket.pflat.device
        # allocated once: a captured step bakes these pointers in
        self.m = torch.zeros_like(bucket.pflat, dtype=state_dtype)
        self.v: Optional[torch.Tensor] = None
        self.t = torch.zeros(1, dtype=torch.int32, device=dev)
        # the norm pass runs for the clip, and for the guard's verdict
        self.norm_ws = sqnorm_workspace(dev) if (max_grad_norm is not None or skip_nonfinite) else None
        self.guard = guard_state(dev) if skip_nonfinite else None
        self.device_lr = False
        self.groups: Optional[OptimGroups] = None  # segments and the device rows (device_lr)
        self._group_hyper: List[Dict[str, Any]] = []
        self._lr: Optional[float] = None  # the learning rate the rows hold

    # ---- parameter groups ------------------------------------------------------

    def _init_groups(self, param_groups, device_lr: bool) -> None:
        """Called by the subclass once ``weight_decay`` is set."""
        b = self.bucket
        spans = b.spans()
        if param_groups is None:
            if device_lr:
                param_groups = []
            else:
                self._group_hyper = [{"lr_scale": 1.0, "weight_decay": self.weight_decay, "spans": [(0, b.numel)]}]
                return
        index = {id(p): i for i, p in enumerate(b.params)}
        owner: List[Optional[int]] = [None] * len(b.params)
        hyper = []
        for gi, g in enumerate(param_groups):
            if not isinstance(g, dict) or "params" not in g:
                raise ValueError(f"param_groups[{gi}]: a dict with 'params'")
            unknown = sorted(set(g) - set(self.group_keys))
            if unknown:
                raise ValueError(f"param_groups[{gi}]: unknown key {unknown[0]!r} (known: "
                                 f"{', '.join(self.group_keys)})")
            wd, scale = float(g.get("weight_decay", self.weight_decay)), float(g.get("lr_scale", 1.0))
            if not (wd >= 0 and scale >= 0):
                raise ValueError(f"param_groups[{gi}]: weight_decay and lr_scale are >= 0")
            ps = g["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            if not ps:
                raise ValueError(f"param_groups[{gi}]: no parameters")
            for p in ps:
                i = index.get(id(p))
                if i is None:
                    raise ValueError(f"param_groups[{gi}]: a parameter that is not in the bucket")
                if owner[i] is not None:
                    raise ValueError(f"param_groups[{gi}]: parameter {i} of the bucket is already in group {owner[i]}")
                owner[i] = gi
            hyper.append({"lr_scale": scale, "weight_decay": wd, "spans": []})
            if "layer_adaptation" in self.group_keys:
                adapt = g.get("layer_adaptation", True)
                if not isinstance(adapt, bool):
                    raise ValueError(f"param_groups[{gi}]: layer_adaptation={adapt!r}, True or False")
                hyper[-1]["layer_adaptation"] = adapt
        if any(o is None for o in owner):  # listed nowhere: a last group with the defaults
            hyper.append({"lr_scale": 1.0, "weight_decay": self.weight_decay, "spans": []})
            if "layer_adaptation" in self.group_keys:
                hyper[-1]["layer_adaptation"] = True
            owner = [len(hyper) - 1 if o is None else o for o in owner]
        # adjacent parameters of one group are one segment (not for LAMB: a segment is a layer)
        seg_end: List[int] = []
        seg_group: List[int] = []
        for (off, n), gi in zip(spans, owner):
            if n == 0:
                continue
            if self.merge_segments and seg_group and seg_group[-1] == gi:
                seg_end[-1] = off + n
                o, k = hyper[gi]["spans"][-1]
                hyper[gi]["spans"][-1] = (o, k + n)
            else:
                seg_end.append(off + n)
                seg_group.append(gi)
                hyper[gi]["spans"].append((off, n))
        self.device_lr = True
        self._group_hyper = hyper
        self.groups = OptimGroups(seg_end, seg_group, len(hyper), b.pflat.device)

    @property
    def param_groups(self) -> List[Dict[str, Any]]:
        """Copies of the groups: ``lr_scale``, ``weight_decay`` and the ``spans`` (offset, numel) of the flat
        buffer each one covers.  Change them with ``set_group``."""
        return [{**g, "spans": list(g["spans"])} for g in self._group_hyper]

    @property
    def lr(self) -> Optional[float]:
        """The learning rate the device rows hold (None: none uploaded yet, or no ``device_lr``)."""
        return self._lr

    def _need_device_lr(self, what: str) -> None:
        if not self.device_lr:
            raise RuntimeError(f"{type(self).__name__}.{what}: built without param_groups / device_lr, the learning "
                               "rate and the weight decay are launch arguments")

    def _upload(self) -> None:
        self.groups.write_rows(OptimGroups.row_values(
            self._lr, [(g["lr_scale"], g["weight_decay"]) for g in self._group_hyper]))

    def set_lr(self, lr: float) -> None:
        """Recompute the groups' rows for ``lr`` on the host and upload them (one stream-ordered copy on the
        current stream): the next pass, eager or replayed, steps with it."""
        self._need_device_lr("set_lr")
        self._lr = float(lr)
        self._upload()

    def set_group(self, i: int, weight_decay: Optional[float] = None, lr_scale: Optional[float] = None) -> None:
        self._need_device_lr("set_group")
        g = self._group_hyper[i]
        for key, val in (("weight_decay", weight_decay), ("lr_scale", lr_scale)):
            if val is not None:
                if not float(val) >= 0:
                    raise ValueError(f"set_group: {key} is >= 0")
                g[key] = float(val)
        if self._lr is not None:
            self._upload()

    # ---- state -------------------------------------------------------------------

    @property
    def param_dtype(self) -> torch.dtype:
        """The dtype of the bucket's flat parameters this optimizer was built on (read-only)."""
        return self._param_dtype

    def state_pointers(self) -> Tuple[int, ...]:
        """Addresses of everything a captured step reads or writes.  The guard's record joins them only
        where the optimizer has one, so without ``skip_nonfinite`` the tuple is what it always was."""
        gr = self.groups
        return tuple(0 if x is None else x.data_ptr() for x in (
            self.m, self.v, self.t, self.norm_ws,
            *((self.guard,) if self.guard is not None else ()),
            *((gr.rows, gr.seg_end, gr.seg_group) if gr is not None else ()),
            *self._step_buffers().values()))

    def _step_buffers(self) -> Dict[str, torch.Tensor]:
        """What ``optim_step_`` takes beyond the state, by keyword (LAMB's tables)."""
        return {}

    def state_tensors(self) -> Tuple[torch.Tensor, ...]:
        return tuple(x for x in (self.m, self.v, self.t, self.guard) if x is not None)

    # ---- the guard's record ------------------------------------------------------------

    def _need_guard(self, what: str) -> torch.Tensor:
        if self.guard is None:
            raise RuntimeError(f"{type(self).__name__}.{what}: built without skip_nonfinite")
        return self.guard

    @property
    def last_step_applied(self) -> bool:
        """Was the last step applied (False: skipped, its gradient was not finite)?  A host sync, like
        ``int(opt.t)``; False before the first step."""
        return int(self._need_guard("last_step_applied")[0]) == 1

    @property
    def skipped_steps(self) -> int:
        """Steps skipped in total (a host sync)."""
        return int(self._need_guard("skipped_steps")[1])

    @property
    def skipped_in_a_row(self) -> int:
        """Steps skipped since the last applied one (a host sync)."""
        return int(self._need_guard("skipped_in_a_row")[2])

    def grad_norm(self) -> torch.Tensor:
        """The global norm of the last round's mean gradient, as the norm pass left it: a 0-dim device tensor
        ``sqrt(norm_ws[0])``, no host sync.  Available whenever the optimizer runs a norm pass (a clip or
        ``skip_nonfinite``); inf or NaN after a skipped step."""
        if self.norm_ws is None:
            raise RuntimeError(f"{type(self).__name__}.grad_norm: no norm pass (neither max_grad_norm nor "
                               "skip_nonfinite)")
        return self.norm_ws[0].sqrt()

    def _hyper_dict(self) -> Dict[str, Any]:
        return {**{k: getattr(self, k) for k in self.hyper}, "max_grad_norm": self.max_grad_norm}

    def state_dict(self) -> Dict[str, Any]:
        """The optimizer's state with cloned tensors (``t`` is read from the device: a host sync)."""
        return {"kind": self.kind, "numel": self.bucket.numel, "t": int(self.t), "m": self.m.clone(),
                "v": None if self.v is None else self.v.clone(), "hyper": self._hyper_dict(), "lr": self._lr,
                "param_groups": self.param_groups, "state_dtype": self.state_dtype, "seed": self.seed,
                "skip_nonfinite": self.skip_nonfinite, "param_dtype": self.param_dtype,
                "guard": None if self.guard is None else [int(x) for x in self.guard.tolist()]}

    def load_state_dict(self, d: Dict[str, Any]) -> None:
        """Load a ``state_dict`` of an optimizer of the same kind, size and group layout.  Everything is copied
        IN PLACE: no address changes, so a captured step stays valid.  The hyper-parameters that are launch
        arguments (betas, eps, momentum, the clip norm; without ``device_lr`` the weight decay too) must match
        the ones this optimizer was built with -- a captured step has them baked in; the groups' weight decay
        and lr scale and the uploaded learning rate are taken from ``d`` and the rows written again.
        ``seed`` is a launch argument too and must match (a dict without one was saved with seed 0).

        ``m`` and ``v`` may be float32 or bfloat16 whatever this optimizer's ``state_dtype``: float32 into
        bfloat16 state rounds to nearest, once; bfloat16 into float32 state is exact.  Any other dtype raises.

        ``param_dtype`` must be this optimizer's (a dict without one was saved from float32 parameters).

        ``skip_nonfinite`` decides which kernels a capture holds and must match this optimizer's own (a dict
        saved before the guard existed counts as guard off with zero counters); the guard's record is copied
        in place."""
        if d.get("kind") != self.kind:
            raise ValueError(f"load_state_dict: kind {d.get('kind')!r}, this optimizer is {self.kind!r}")
        if d.get("numel") != self.bucket.numel:
            raise ValueError(f"load_state_dict: numel {d.get('numel')}, this bucket has {self.bucket.numel}")
        mine, theirs = self._group_hyper, list(d.get("param_groups") or [])
        if len(mine) != len(theirs):
            raise ValueError(f"load_state_dict: {len(theirs)} param_groups, this optimizer has {len(mine)}")
        for i, (a, b) in enumerate(zip(mine, theirs)):
            if [tuple(s) for s in b["spans"]] != [tuple(s) for s in a["spans"]]:
                raise ValueError(f"load_state_dict: param_groups[{i}] spans {list(b['spans'])}, this optimizer "
                                 f"has {a['spans']}")
            if "layer_adaptation" in a and bool(b.get("layer_adaptation", True)) != a["layer_adaptation"]:
                raise ValueError(f"load_state_dict: param_groups[{i}] layer_adaptation="
                                 f"{bool(b.get('layer_adaptation', True))}, this optimizer was built with "
                                 f"{a['layer_adaptation']} (a device table of the captured step)")
        hyper = d.get("hyper") or {}
        for k, mine_v in self._hyper_dict().items():
            if k == "weight_decay" and self.device_lr:
                continue  # per group, in the rows
            theirs_v = hyper.get(k)
            theirs_v = tuple(theirs_v) if isinstance(theirs_v, (list, tuple)) else theirs_v
            if theirs_v != mine_v:
                raise ValueError(f"load_state_dict: {k}={theirs_v!r}, this optimizer was built with {mine_v!r} "
                                 "(a launch argument)")
        if not self.device_lr and (theirs[0]["lr_scale"] != 1.0 or theirs[0]["weight_decay"] != self.weight_decay):
            raise ValueError("load_state_dict: the group's lr_scale / weight_decay differ; without device_lr they "
                             "are launch arguments")
        if d.get("param_dtype", torch.float32) != self.param_dtype:
            raise ValueError(f"load_state_dict: param_dtype={d.get('param_dtype', torch.float32)}, this optimizer's "
                             f"parameters are {self.param_dtype} (it decides which kernels a capture holds)")
        if d.get("seed", 0) != self.seed:
            raise ValueError(f"load_state_dict: seed={d.get('seed', 0)!r}, this optimizer was built with {self.seed!r} "
                             "(a launch argument)")
        if bool(d.get("skip_nonfinite", False)) != self.skip_nonfinite:
            raise ValueError(f"load_state_dict: skip_nonfinite={bool(d.get('skip_nonfinite', False))}, this optimizer "
                             f"was built with {self.skip_nonfinite} (it decides which kernels a capture holds)")
        record = d.get("guard")
        if self.guard is not None and record is not None and len(record) != 4:
            raise ValueError(f"load_state_dict: the guard's record has 4 entries, not {len(record)}")
        if (d.get("v") is None) != (self.v is None):
            raise ValueError("load_state_dict: v does not match the optimizer's kind")
        for name, dst in (("m", self.m), ("v", self.v)):
            if dst is not None and (d[name].shape != dst.shape or d[name].dtype not in _STATE_DTYPES):
                raise ValueError(f"load_state_dict: {name} is {d[name].dtype} {tuple(d[name].shape)}")
        self.m.copy_(d["m"])
        if self.v is not None:
            self.v.copy_(d["v"])
        self.t.fill_(int(d["t"]))
        if self.guard is not None:
            self.guard.copy_(torch.tensor([0, 0, 0, 0] if record is None else [int(x) for x in record],
                                          dtype=torch.int32))
        if self.device_lr:
            for a, b in zip(mine, theirs):
                a["lr_scale"], a["weight_decay"] = float(b["lr_scale"]), float(b["weight_decay"])
            self._lr = None if d.get("lr") is None else float(d["lr"])
            if self._lr is not None:
                self._upload()

    # ---- the step ------------------------------------------------------------------

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
        if self.device_lr and lr != self._lr:
            # the rows are written outside a graph: a capture holds the pass, never the upload
            if self.t.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: lr={lr} while capturing, the rows hold {self._lr}; call "
                                   "set_lr before the capture")
            self.set_lr(lr)
        if self.guard is None:
            self.t.add_(1)  # with a guard the norm pass advances the step, and only for an applied one
        out.optim_step_(self.kind, bucket.pflat, self.m, self.v, self.t, lr, shadow=shadow, max_norm=self.max_grad_norm,
                        norm_ws=self.norm_ws, groups=self.groups, seed=self.seed, guard=self.guard,
                        **self._step_buffers(), **{k: getattr(self, k) for k in self.hyper})


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD(momentum, nesterov, weight_decay)`` (dampening 0) on a
    ``GradientBucket(flatten_params=True)``, fused into the averaging.

    ``param_groups``: a list of dicts ``{"params": [...], "weight_decay": wd,
    "lr_scale": s}`` (both optional: the optimizer's ``weight_decay`` and 1.0)
    over parameters of the bucket, each in at most one group; the parameters
    listed nowhere form a last group with the defaults.  A group steps with
    ``lr * lr_scale``.  ``device_lr=True`` alone is one group; either keeps the
    learning rate in device memory (``set_lr``).

    ``state_dtype=torch.bfloat16`` keeps the momentum in bf16, stored with
    stochastic rounding; ``seed`` keys the rounding bits and must be the same
    on every rank.  A bucket of bf16 parameters and gradients needs it, and
    then stores the parameters with stochastic rounding too, from the same
    ``seed`` (``param_dtype``; the module's docstring).

    ``skip_nonfinite=True`` drops a step whose gradient is not finite on the
    device and counts it (the module's docstring); with ``momentum=0`` this is
    the guarded plain SGD."""

    kind, hyper = "sgd", ("momentum", "nesterov", "weight_decay")

    def __init__(self, bucket: GradientBucket, momentum: float = 0.9, nesterov: bool = False,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None, param_groups=None,
                 device_lr: bool = False, state_dtype: torch.dtype = torch.float32, seed: int = 0,
                 skip_nonfinite: bool = False):
        if momentum < 0 or weight_decay < 0:
            raise ValueError("FusedSGD: momentum and weight_decay are >= 0")
        if nesterov and momentum <= 0:
            raise ValueError("FusedSGD: Nesterov momentum needs momentum > 0")
        super().__init__(bucket, max_grad_norm, state_dtype, seed, skip_nonfinite)
        self.momentum, self.nesterov, self.weight_decay = float(momentum), bool(nesterov), float(weight_decay)
        self._init_groups(param_groups, device_lr)


class FusedAdamW(_FusedOptimizer):
    """``torch.optim.AdamW(betas, eps, weight_decay)`` on a
    ``GradientBucket(flatten_params=True)``, fused into the averaging.
    ``param_groups`` / ``device_lr`` / ``state_dtype`` / ``seed`` /
    ``skip_nonfinite`` as for ``FusedSGD`` (bf16 state: ``m`` and ``v``)."""

    kind, hyper = "adamw", ("betas", "eps", "weight_decay")

    def __init__(self, bucket: GradientBucket, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01, max_grad_norm: Optional[float] = None, param_groups=None,
                 device_lr: bool = False, state_dtype: torch.dtype = torch.float32, seed: int = 0,
                 skip_nonfinite: bool = False):
        if not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or eps < 0 or weight_decay < 0:
            raise ValueError("FusedAdamW: betas in [0, 1), eps and weight_decay >= 0")
        super().__init__(bucket, max_grad_norm, state_dtype, seed, skip_nonfinite)
        self.v = torch.zeros_like(self.m)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self._init_groups(param_groups, device_lr)


class FusedLAMB(_FusedOptimizer):
    """LAMB on a ``GradientBucket(flatten_params=True)``, fused into the
    averaging: AdamW's moments, then per layer (one parameter of the bucket)

        u = (m / bc1) / (sqrt(v / bc2) + eps) + weight_decay * p
        r = ||p|| / ||u||  where both are positive and finite, else 1
        p = p - lr * r * u

    with ``bc_k = 1 - beta_k^t``, ``p`` in ``r`` taken before the step, no clamp
    on ``r``.  Both norms run over the layer's elements whose chunk had a
    contributor: a missing chunk (count 0) enters neither norm and keeps ``p``,
    ``m``, ``v`` and the shadow, and a layer with no contributing element has
    ``r = 1`` and does not move.  The norms are computed on the device by a
    pass of their own in front of the update (fixed tiles, partial sums in a
    fixed order, no atomics): the same inputs give the same bits on every call
    and every replay of a captured step, with no host sync and nothing to
    reset.

    The learning rate and the decay always live in the device rows (as with
    ``device_lr=True``: ``set_lr`` between replays works), and every non-empty
    parameter is a segment of its own.  ``param_groups`` as for ``FusedSGD``,
    with one more key: ``layer_adaptation`` (default True); False pins ``r = 1``
    for that group's layers (biases, norm scales).  ``trust_ratios()`` gives
    the last step's ratios.  ``state_dtype`` / ``seed`` / ``skip_nonfinite`` /
    ``max_grad_norm`` as for ``FusedAdamW``; the clip coefficient enters the
    gradient before the moments."""

    kind, hyper = "lamb", ("betas", "eps", "weight_decay")
    group_keys = _GROUP_KEYS + ("layer_adaptation",)
    merge_segments = False

    def __init__(self, bucket: GradientBucket, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.01, max_grad_norm: Optional[float] = None, param_groups=None,
                 state_dtype: torch.dtype = torch.float32, seed: int = 0, skip_nonfinite: bool = False):
        if not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or eps < 0 or weight_decay < 0:
            raise ValueError("FusedLAMB: betas in [0, 1), eps and weight_decay >= 0")
        super().__init__(bucket, max_grad_norm, state_dtype, seed, skip_nonfinite)
        self.v = torch.zeros_like(self.m)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self._init_groups(param_groups, True)
        gr, dev = self.groups, bucket.pflat.device
        nseg = len(gr.host_seg_end)
        # allocated once, like the state: the per-layer opt-out, the ratios and the norm pass's partials
        self.layer_adapt = torch.tensor([int(self._group_hyper[g]["layer_adaptation"]) for g in gr.host_seg_group],
                                        dtype=torch.int32, device=dev)
        self.trust = torch.ones(nseg, dtype=torch.float32, device=dev)
        self.lamb_ws = lamb_workspace(bucket.numel, nseg, dev)
        # each parameter's segment (an empty one has none)
        self._layer: List[Optional[int]] = []
        for _, n in bucket.spans():
            self._layer.append(None if n == 0 else sum(x is not None for x in self._layer))

    def _step_buffers(self) -> Dict[str, torch.Tensor]:
        return {"lamb_ws": self.lamb_ws, "trust": self.trust, "layer_adapt": self.layer_adapt}

    def state_tensors(self) -> Tuple[torch.Tensor, ...]:
        """With the trust table: a captured step's warm-up writes it, and it is put back with ``m``, ``v`` and ``t``."""
        return (*super().state_tensors(), self.trust)

    def trust_ratios(self) -> List[torch.Tensor]:
        """The trust ratios of the last applied step, one one-element view of the device table per parameter
        of the bucket (an empty view for an empty parameter), no host sync; 1 before the first step."""
        return [self.trust[:0] if i is None else self.trust[i:i + 1] for i in self._layer]
