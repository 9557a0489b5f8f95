"""Fused optimizer step: AdamW / Adam / SGD with parameter groups, global-norm clipping and GradScaler's overflow skip in
three HIP launches over all parameter tensors (csrc/optim.hip: m3_optim_prepare, m3_optim_step).

What every trainer of the reference runs behind the backward - torch.optim.SGD / Adam / AdamW with parameter groups
(utils/common_config.py:866-896, pretrain/optim/optimizer.py:6-46) after GradScaler.unscale_, clip_grad_norm_ and inside
scaler.step (pretrain/engine/train_one_epoch.py:35-61) - is several passes over ~300 tensors in torch.  Here the gradients
are read once for the norm and once for the update; the unscale and clip factors are applied in registers, so the gradient
buffer is never written.

    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.05, max_grad_norm=1.0)     # instead of torch.optim.AdamW
    scaler.scale(loss).backward(); scaler.step(opt); scaler.update()                        # no unscale_ / clip_grad_norm_

The classes are torch.optim.Optimizer subclasses (param groups, add_param_group, lr schedulers, zero_grad) and take torch's
arguments plus max_grad_norm.  Per-parameter state carries torch's key names (exp_avg, exp_avg_sq, step; momentum_buffer) as
views of flat fp32 buffers, and state_dict() / load_state_dict() exchange checkpoints with the matching torch optimizer.
The kernels keep ONE step counter on the device (a skipped step does not advance it): state_dict() writes it into every
parameter's `step`, load_state_dict() refuses a checkpoint whose parameters disagree.

step() reads nothing from the device: whether an overflow skipped the update is known to the GPU alone, so the parameters'
version counters (what FusedBackbone watches to refresh its operand copies) are bumped on every call.

Not here: amsgrad, maximize, dampening != 0 (refused); hipGraph capture of the step; the data-parallel 1 / world factor (the
gradients are taken as they are); max_grad_norm under expert parallelism (the norm would need a cross-rank sum of the expert
shards)."""
from __future__ import annotations

import torch

from . import ops

NO_DECAY = ("bias", "norm", "pos_embed", "cls_token", "dist_token", "w_gate")


def _round4(n: int) -> int:
    return (n + 3) & ~3


class _FusedOptimizer(torch.optim.Optimizer):
    _step_supports_amp_scaling = True      # torch.amp.GradScaler.step then installs grad_scale / found_inf and calls step()
    _kind = None                           # "adamw" / "adam" / "sgd"
    _state_keys = ()                       # torch's names of the flat state buffers, first moment first

    def __init__(self, params, defaults, max_grad_norm=None):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be positive or None, got {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._plan = None                  # ops.OptimPlan of the current (parameter, gradient) pointers
        self._sig = None
        self._live = []
        self._block = None                 # the device state block (step counter, norm, ...): survives plan rebuilds
        self._pending_step = None          # a loaded step count that has not reached the device yet
        self._mine = set()                 # id(p) of the parameters whose state tensors are views of self._flats
        self._flats = []
        self._bound = {}                   # id(p) -> gradient tensor (for_engine: the executor's tensors have no .grad)
        self._engine = None
        super().__init__(params, defaults)

    # ------------------------------------------------------------------------------------------------ groups
    def _check_group(self, group):
        for key in ("amsgrad", "maximize"):
            if group.get(key, False):
                raise NotImplementedError(f"{type(self).__name__}: {key}=True is not supported by the fused kernels; "
                                          f"use torch.optim for it")
        if group.get("dampening", 0) != 0:
            raise NotImplementedError(f"{type(self).__name__}: dampening != 0 is not supported by the fused kernels")
        if group.get("nesterov", False) and not group.get("momentum", 0) > 0:
            raise ValueError("nesterov momentum requires a momentum")
        for key in ("lr", "eps", "weight_decay", "momentum"):
            v = group.get(key, 0.0)
            if torch.is_tensor(v):
                raise NotImplementedError(f"{type(self).__name__}: a tensor {key} is not supported; pass a Python number")
            if v < 0.0:
                raise ValueError(f"invalid {key}: {v}")
        for b in group.get("betas", ()):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"invalid beta: {b}")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        self._sig = None

    def _hyper_row(self, group):
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------------- state
    def _ensure_state(self, params):
        """flat fp32 state buffers (each tensor's offset rounded up to 4 elements) for those of `params` - the parameters
        that take this step - that have none yet: as in torch, a parameter gets state when it first steps.  Tensors a
        load_state_dict() left in self.state are copied into them"""
        new = [p for p in params if id(p) not in self._mine]
        if not new:
            return
        by_dev = {}
        for p in new:
            by_dev.setdefault(p.device, []).append(p)
        for dev, ps in by_dev.items():
            total = sum(_round4(p.numel()) for p in ps)
            flats = [torch.zeros(total, dtype=torch.float32, device=dev) for _ in self._state_keys]
            self._flats.append(flats)
            o = 0
            for p in ps:
                st = self.state[p]
                for key, flat in zip(self._state_keys, flats):
                    view = flat[o:o + p.numel()].view(p.shape)
                    old = st.get(key)
                    if torch.is_tensor(old):
                        view.copy_(old)
                    st[key] = view
                if "step" in self._state_keys_extra and "step" not in st:
                    st["step"] = torch.tensor(0.0)
                o += _round4(p.numel())
                self._mine.add(id(p))
        self._sig = None

    _state_keys_extra = ()

    def _step_count(self) -> int:
        """the device's step counter (a host read)"""
        if self._pending_step is not None:
            return self._pending_step
        return int(self._block[1:2].view(torch.int32).item()) if self._block is not None else 0

    def state_dict(self):
        if "step" in self._state_keys_extra and self.state:
            t = float(self._step_count())
            for st in self.state.values():
                if "step" in st:
                    st["step"] = torch.tensor(t)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            self._check_group(g)
        steps = set()
        for st in self.state.values():
            if "step" in st:
                steps.add(int(round(float(st["step"]))))
        if len(steps) > 1:
            raise ValueError(f"{type(self).__name__} keeps one step counter for all parameters; the checkpoint holds "
                             f"different ones: {sorted(steps)}")
        if steps:
            self._set_step(steps.pop())
        self._mine.clear()                  # the loaded tensors are copies: move them into flat buffers on the next step
        self._flats = []
        self._sig = None

    def _set_step(self, t: int):
        if self._block is not None:
            self._block[1:2].view(torch.int32).fill_(t)
        else:
            self._pending_step = t

    # -------------------------------------------------------------------------------------------------- step
    def _rebuild(self, live):
        entries = []
        for p, g, gi in live:
            if g.is_sparse:
                raise ops._lib.M3Error(f"{type(self).__name__} does not support sparse gradients")
            st = self.state[p]
            entries.append((p, g, st[self._state_keys[0]], st[self._state_keys[1]] if len(self._state_keys) > 1 else None, gi))
        n_groups = len(self.param_groups)
        block = self._block
        if block is not None and block.numel() != ops.lib().m3_optim_state_elems(n_groups):
            block = None                   # a group was added: a larger block, the header (step counter) carried over
        self._plan = ops.OptimPlan(entries, n_groups, self._kind, state=block)
        if block is None and self._block is not None:
            self._plan.state[:8].copy_(self._block[:8])
        self._block = self._plan.state
        if self._pending_step is not None:
            t, self._pending_step = self._pending_step, None
            self._set_step(t)
        self._live = [p for p, _, _ in live]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        live, sig = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = self._bound.get(id(p))
                if g is None:
                    g = p.grad
                if g is None:               # as in torch: a parameter without a gradient sits this step out
                    continue
                live.append((p, g, gi))
                sig.append((p.data_ptr(), g.data_ptr(), gi))
        if not live:
            return loss
        self._ensure_state([p for p, _, _ in live])
        sig.append(len(self.param_groups))
        if sig != self._sig:
            self._rebuild(live)
            self._sig = sig
        plan = self._plan
        plan.set_hyper([self._hyper_row(g) for g in self.param_groups])
        plan.prepare(grad_scale=getattr(self, "grad_scale", None), found_inf=getattr(self, "found_inf", None),
                     max_norm=self.max_grad_norm or 0.0)
        plan.step()
        # the kernels wrote through raw pointers: tell autograd (and FusedBackbone._check_params, which learns of an optimizer
        # step from p._version) that the values changed.  On a skipped step too - the host does not know.
        torch.autograd.graph.increment_version(self._live)
        if self._engine is not None:
            self._engine.prepare_weights()
        return loss

    def zero_grad(self, set_to_none: bool = True):
        if self._engine is not None:
            self._engine.zero_grad()
        else:
            super().zero_grad(set_to_none=set_to_none)

    @property
    def last_grad_norm(self):
        """the global gradient norm of the last step() (unscaled: what clip_grad_norm_ would have returned), a 0-dim device
        tensor that aliases the kernels' state block; reading it is the caller's synchronisation"""
        if self.max_grad_norm is None:
            raise RuntimeError("last_grad_norm needs max_grad_norm: without it the norm pass does not run")
        if self._block is None:
            raise RuntimeError("last_grad_norm: no step() has run yet")
        return self._block[2]

    # ------------------------------------------------------------------------------------------------ engine
    @classmethod
    def for_engine(cls, engine_or_step, no_decay=NO_DECAY, **hyper):
        """The optimizer of a BackboneEngine (or of a MultiTaskStep, through its first engine): parameters from
        engine.params, gradients from the buffer that holds the step's summed gradients (engine.grads), two groups -
        names that contain one of `no_decay` get weight_decay 0.  step() ends with the engine's prepare_weights(), so the
        operand copies are fresh when it returns; zero_grad() is the engine's."""
        eng = getattr(engine_or_step, "eng", engine_or_step)
        if getattr(eng, "ep_world", 1) > 1 and hyper.get("max_grad_norm") is not None:
            raise NotImplementedError("max_grad_norm under expert parallelism needs a cross-rank sum of the expert shards' "
                                      "norms, which the fused step does not do; clip outside or leave it None")
        decay = [p for n, p in eng.params.items() if not any(k in n for k in no_decay)]
        plain = [p for n, p in eng.params.items() if any(k in n for k in no_decay)]
        groups = [{"params": decay}] if decay else []
        if plain:
            groups.append({"params": plain, "weight_decay": 0.0})
        opt = cls(groups, **hyper)
        opt._bound = {id(p): eng.grads[n] for n, p in eng.params.items()}
        opt._engine = eng
        return opt


class _FusedAdamBase(_FusedOptimizer):
    _state_keys = ("exp_avg", "exp_avg_sq")
    _state_keys_extra = ("step",)
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 max_grad_norm=None):
        # the keys torch's Adam / AdamW expect in a param group, so that a state_dict() loads there
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=self._decoupled)
        super().__init__(params, defaults, max_grad_norm=max_grad_norm)

    def _hyper_row(self, g):
        return ops.optim_hyper_row(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                                   decoupled=self._decoupled)


class FusedAdamW(_FusedAdamBase):
    """torch.optim.AdamW (decoupled weight decay) on the fused kernels."""
    _kind, _decoupled = "adamw", True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, max_grad_norm=max_grad_norm)


class FusedAdam(_FusedAdamBase):
    """torch.optim.Adam (weight decay as L2 added to the gradient) on the fused kernels."""
    _kind, _decoupled = "adam", False


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD (momentum, weight decay, nesterov; dampening 0) on the fused kernels."""
    _kind = "sgd"
    _state_keys = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 max_grad_norm=None):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, max_grad_norm=max_grad_norm)

    def _hyper_row(self, g):
        return ops.optim_hyper_row(g["lr"], g["momentum"], weight_decay=g["weight_decay"], nesterov=g["nesterov"])
