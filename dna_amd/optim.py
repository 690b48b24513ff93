"""Fused optimizer step and LR schedule of the DNABERT-2 pretraining path.

FusedAdamW = Lightning `gradient_clip_val: 1.0` (torch.nn.utils.clip_grad_norm_) + torch AdamW
(reference: train.py:462-542, registry.optimizer["adamw"], configs/optimizer/adamw.yaml,
experiment overrides lr 5e-4 / weight_decay 1e-5) over the flat buffers of dna_amd.flat: one
sum-of-squares launch and one AdamW launch per step, clip coefficient read on the device.

LinearLRSchedulerWarmup restates src/utils/optim/schedulers.py:92-147 (timm Scheduler subclass,
stepped per optimizer step with t_in_epochs False). The reference leaves `cycle_limit` and
`cycle_decay` unset and raises AttributeError once t >= warmup_t; here they default to
no limit / decay 1, the values the formula needs.

ParamGroups restates the grouping of the reference's configure_optimizers (train.py:462-487):
parameters tagged `_optim` (the Hyena filter: its own lr, weight_decay 0) get AdamW groups of
their own. add_optimizer_hooks restates the reference's hook that writes such `_optim` tags
(no weight decay on biases, `_no_weight_decay` parameters, embeddings, torch norm layers;
src/utils/optim_groups.py:14-38). TimmCosineLRScheduler restates timm.scheduler.CosineLRScheduler with its defaults
(registry scheduler "cosine_warmup_timm"); timm is not a dependency, so nothing pins it to
timm's output -- the same standing as the linear schedule above.
"""
import math

import torch

from . import _native as N
from .flat import note_raw_write


def add_optimizer_hooks(model, bias_weight_decay=False, normalization_weight_decay=False):
    """The reference's add_optimizer_hooks (src/utils/optim_groups.py:14-38, called from
    train.py:464-465 when train.optimizer_param_grouping is set), restated as written: walking
    every module's named_parameters() (a module's own and its descendants'), it sets
    `_optim = {"weight_decay": 0.0}` on
      * parameters whose name ends in `bias`, unless bias_weight_decay;
      * parameters tagged `_no_weight_decay` (the Mamba mixer's A_log and D);
      * every parameter of an nn.Embedding (blacklisted regardless of the flags);
      * every parameter of a torch normalization module (nn.LayerNorm, nn.GroupNorm, the
        BatchNorm / InstanceNorm family, nn.LocalResponseNorm), unless normalization_weight_decay.
    ParamGroups then gives these parameters an AdamW group of their own. As in the reference, an
    `_optim` a layer set before (the Hyena filter's lr) is replaced where the rule applies, and a
    tied tensor is one parameter: tagged once, whichever module reaches it.

    Deviation kept on purpose: the project's RMSNorm (caduceus.RMSNorm, as mamba_ssm's) is not in
    the reference's list, so its weight stays decayed, as it does in the reference's Caduceus
    runs. hyena_lm.LayerNorm subclasses nn.LayerNorm and functional.HipEmbedding nn.Embedding, so
    both fall under the rule."""
    import torch.nn as nn
    blacklist = (nn.Embedding,)
    if not normalization_weight_decay:
        blacklist += (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.GroupNorm,
                      nn.SyncBatchNorm, nn.InstanceNorm1d, nn.InstanceNorm2d, nn.InstanceNorm3d,
                      nn.LayerNorm, nn.LocalResponseNorm)
    for _, m in model.named_modules():
        for pn, p in m.named_parameters():
            if (not bias_weight_decay and pn.endswith("bias")) \
                    or getattr(p, "_no_weight_decay", False) \
                    or isinstance(m, blacklist):
                p._optim = {"weight_decay": 0.0}


class ParamGroups:
    """The reference's optimizer grouping rule: parameters without `_optim` form group 0 (the
    optimizer config as it is); every distinct `_optim` dict forms one more group, in the order
    Python's sorted() gives the dicts' frozenset(items()) after first-appearance de-duplication
    (what the reference sorts), with `{**optimizer_cfg, **_optim}` as hyperparameters.
    Callable: parameter -> group index (FlatParams' group_of)."""

    def __init__(self, module):
        self.registration = list(module.parameters())
        tagged = [p for p in self.registration if hasattr(p, "_optim")]
        keys = sorted(dict.fromkeys(frozenset(p._optim.items()) for p in tagged))
        self.overrides = [{}] + [{k: v for k, v in dict(key).items() if v is not None}
                                 for key in keys]
        self._index = {}
        for p in self.registration:
            hp = getattr(p, "_optim", None)
            self._index[id(p)] = 0 if hp is None else 1 + keys.index(frozenset(hp.items()))

    def __call__(self, p):
        return self._index[id(p)]

    def __len__(self):
        return len(self.overrides)

    def members(self, gi):
        """The group's parameters in registration order (torch's indices inside the group)."""
        return [p for p in self.registration if self._index[id(p)] == gi]


class FusedAdamW:
    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=1.0, groups=None):
        """groups: a ParamGroups over the model, with `flat` laid out by it
        (FlatParams(group_of=groups)): one AdamW launch per group over its contiguous extent, one
        clip coefficient from the one global gradient norm. None: one group, one launch."""
        self.flat = flat
        # elements of the flat buffers the step covers: all of them, or the leading part when the
        # parameters behind it are frozen (trainer.SeqClsTrainer). What it leaves out gets no
        # update, no weight decay and no share in the clip norm, like torch's AdamW and
        # clip_grad_norm_ treat parameters without a gradient
        self.numel = flat.numel
        dev = flat.flat.device
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        base = dict(lr=float(lr), betas=tuple(betas), eps=float(eps),
                    weight_decay=float(weight_decay))
        self.groups = groups
        self.extents = [(0, None)]  # None: up to self.numel
        overrides = [{}]
        if groups is not None:
            if flat.group_extents is None or sorted(flat.group_extents) != list(range(len(groups))):
                raise ValueError("FusedAdamW(groups=...): the flat buffers must be laid out by the "
                                 "same grouping (FlatParams(group_of=groups))")
            self.extents = [flat.group_extents[g] for g in range(len(groups))]
            overrides = groups.overrides
        self.param_groups = []
        for ov in overrides:
            g = dict(base, **ov)
            g["lr"] = float(g["lr"])
            g["weight_decay"] = float(g["weight_decay"])
            g["betas"] = tuple(g["betas"])
            g["initial_lr"] = g["lr"]
            self.param_groups.append(g)
        self.max_grad_norm = max_grad_norm
        self.step_count = 0
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        nws = N.lib().dna_sumsq_workspace(flat.numel)
        self._ws = torch.empty(nws // 4 + 4, dtype=torch.float32, device=dev)
        self._nws = nws

    def grad_norm_sq(self):
        """Launch the global sum of squares of the gradient (device scalar, no sync)."""
        N.call("dna_sumsq", self.flat.grad.data_ptr(), self.numel, self._sumsq.data_ptr(),
               self._ws.data_ptr(), self._nws, N.stream_ptr())
        return self._sumsq

    def step(self, grad_scale: float = 1.0):
        self.step_count += 1
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        if clip:
            self.grad_norm_sq()
        shadow = self.flat.shadow
        for g, (s, e) in zip(self.param_groups, self.extents):
            e = self.numel if e is None else e
            if e <= s:
                continue
            # extents start and end on FlatParams.ALIGN (64 elements): 16-byte aligned pointers
            N.call("dna_adamw_step", self.flat.flat.data_ptr() + 4 * s,
                   self.flat.grad.data_ptr() + 4 * s, self.exp_avg.data_ptr() + 4 * s,
                   self.exp_avg_sq.data_ptr() + 4 * s,
                   None if shadow is None else shadow.data_ptr() + shadow.element_size() * s,
                   e - s, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                   self.step_count, self._sumsq.data_ptr() if clip else None,
                   float(self.max_grad_norm or 0.0), float(grad_scale), N.stream_ptr())
        note_raw_write()  # the parameters changed behind torch's version counters
        self.flat.refresh_transposed()

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    def _ordered_params(self):
        """Parameters in module registration order = torch's optimizer param indices for the
        reference's single AdamW group (train.py:462-473: list(self.parameters())). With groups:
        the normal parameters first, then each `_optim` group, each in registration order -- the
        order in which the reference hands them to torch (train.py:467-487)."""
        if self.groups is None:
            return self.flat.params[::-1]
        return [p for gi in range(len(self.groups)) for p in self.groups.members(gi)]

    @staticmethod
    def _torch_group(g, params):
        g = dict(g)
        g.setdefault("amsgrad", False)
        g.setdefault("maximize", False)
        g.setdefault("foreach", None)
        g.setdefault("capturable", False)
        g.setdefault("differentiable", False)
        g.setdefault("fused", None)
        g["params"] = params
        return g

    @staticmethod
    def _own_group(g):
        return dict(lr=float(g["lr"]), betas=tuple(g["betas"]), eps=float(g["eps"]),
                    weight_decay=float(g["weight_decay"]),
                    initial_lr=float(g.get("initial_lr", g["lr"])))

    def state_dict(self, torch_layout=True):
        """torch.optim.AdamW layout ({"state": {i: {step, exp_avg, exp_avg_sq}}, "param_groups"}),
        which Lightning's checkpoint loader and torch AdamW.load_state_dict accept; per-parameter
        moments are copied out of the flat buffers. torch_layout=False: the flat form."""
        if not torch_layout:
            return {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                    "param_groups": [dict(g) for g in self.param_groups]}
        params = self._ordered_params()
        state = {}
        if self.step_count > 0:
            for i, p in enumerate(params):
                o, n, shape = self.flat.slice_of(p)
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": self.exp_avg[o:o + n].view(shape).detach().cpu().clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + n].view(shape).detach().cpu().clone()}
        if self.groups is None:
            return {"state": state,
                    "param_groups": [self._torch_group(self.param_groups[0],
                                                       list(range(len(params))))]}
        out, first = [], 0
        for gi, g in enumerate(self.param_groups):
            n = len(self.groups.members(gi))
            out.append(self._torch_group(g, list(range(first, first + n))))
            first += n
        return {"state": state, "param_groups": out}

    def load_state_dict(self, sd):
        """Accepts the flat form and torch's AdamW layout (a Lightning checkpoint of the
        reference: one param group, indices in registration order)."""
        if "state" in sd:
            params = self._ordered_params()
            groups = sd["param_groups"]
            n_idx = sum(len(g["params"]) for g in groups)
            if n_idx != len(params):
                raise ValueError(f"optimizer state holds {n_idx} parameters, model has {len(params)}")
            if self.groups is not None and len(groups) != len(self.param_groups):
                raise ValueError(f"optimizer state has {len(groups)} param groups, this optimizer "
                                 f"{len(self.param_groups)}")
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            step = 0
            for i, p in enumerate(params):
                st = sd["state"].get(i, sd["state"].get(str(i)))
                if not st:
                    continue
                o, n, shape = self.flat.slice_of(p)
                if tuple(st["exp_avg"].shape) != tuple(shape):
                    raise ValueError(f"optimizer state {i}: shape {tuple(st['exp_avg'].shape)} "
                                     f"!= parameter shape {tuple(shape)}")
                self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                step = max(step, int(float(st["step"])))
            self.step_count = step
            n_own = len(self.param_groups) if self.groups is not None else 1
            self.param_groups = [self._own_group(g) for g in groups[:n_own]]
            return
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        if self.groups is not None and len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError(f"optimizer state has {len(sd['param_groups'])} param groups, this "
                             f"optimizer {len(self.param_groups)}")
        self.param_groups = [{k: v for k, v in g.items() if k != "params"} for g in sd["param_groups"]]


class LinearLRSchedulerWarmup:
    """Linear warmup from warmup_lr_init to the base lr over warmup_t steps, then linear decay to
    lr_min over t_initial steps (schedulers.py:113-132), applied to optimizer.param_groups."""

    def __init__(self, optimizer, t_initial, warmup_t=0, warmup_lr_init=0.0, lr_min=0.0,
                 t_in_epochs=False, cycle_limit=None, cycle_decay=1.0, **unused):
        self.optimizer = optimizer
        self.t_initial = t_initial
        self.warmup_t = warmup_t
        self.warmup_lr_init = warmup_lr_init
        self.lr_min = lr_min
        self.t_in_epochs = t_in_epochs
        self.cycle_limit = cycle_limit
        self.cycle_decay = cycle_decay
        self.base_values = [g.get("initial_lr", g["lr"]) for g in optimizer.param_groups]
        self._last_epoch = 0
        self.step(epoch=0)

    def _get_lr(self, t):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * (lr - self.warmup_lr_init) / self.warmup_t
                    for lr in self.base_values]
        if self.cycle_limit is not None and t >= self.cycle_limit * self.t_initial:
            return [self.lr_min for _ in self.base_values]
        cycle = math.floor(1 + (t - self.warmup_t) / self.t_initial)
        t_curr = t - self.warmup_t - (cycle - 1) * self.t_initial
        gamma = self.cycle_decay ** cycle
        return [self.lr_min + (lr * gamma - self.lr_min) * (1 - t_curr / self.t_initial)
                for lr in self.base_values]

    def step(self, epoch=None):
        self._last_epoch = self._last_epoch + 1 if epoch is None else epoch
        for g, lr in zip(self.optimizer.param_groups, self._get_lr(self._last_epoch)):
            g["lr"] = lr

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        """timm Scheduler.state_dict keys (the instance __dict__ minus the optimizer)."""
        return {"_last_epoch": self._last_epoch, "t_initial": self.t_initial,
                "warmup_t": self.warmup_t, "warmup_lr_init": self.warmup_lr_init,
                "lr_min": self.lr_min, "t_in_epochs": self.t_in_epochs,
                "cycle_limit": self.cycle_limit, "cycle_decay": self.cycle_decay,
                "base_values": list(self.base_values)}

    def load_state_dict(self, sd):
        """Resumes the step counter; accepts the reference's timm layout (`_last_epoch`) and the
        round-1 form of this file (`last_epoch`)."""
        t = sd["_last_epoch"] if "_last_epoch" in sd else sd["last_epoch"]
        self.step(epoch=int(t))


class TimmCosineLRScheduler:
    """Registry scheduler "cosine_warmup_timm": timm.scheduler.CosineLRScheduler restated with its
    defaults (cycle_mul = cycle_decay = k_decay = 1, cycle_limit = 1, warmup_prefix False),
    stepped per optimizer step (t_in_epochs False), each group scaled from its own initial_lr:

        t <  warmup_t              lr = warmup_lr_init + t (base - warmup_lr_init) / warmup_t
        warmup_t <= t < t_initial  lr = lr_min + 0.5 (base - lr_min) (1 + cos(pi t / t_initial))
        t >= t_initial             lr = lr_min

    Same interface as LinearLRSchedulerWarmup. Options that would leave that form are refused."""

    def __init__(self, optimizer, t_initial, lr_min=0.0, warmup_t=0, warmup_lr_init=0.0,
                 t_in_epochs=False, cycle_mul=1.0, cycle_decay=1.0, cycle_limit=1,
                 warmup_prefix=False, k_decay=1.0, **unused):
        if (float(cycle_mul), float(cycle_decay), int(cycle_limit), bool(warmup_prefix),
                float(k_decay)) != (1.0, 1.0, 1, False, 1.0):
            raise NotImplementedError("cosine_warmup_timm: cycle_mul, cycle_decay, k_decay = 1, "
                                      "cycle_limit = 1, warmup_prefix = False only")
        if t_initial <= 0:
            raise ValueError(f"cosine_warmup_timm: t_initial must be > 0 (got {t_initial})")
        self.optimizer = optimizer
        self.t_initial = t_initial
        self.lr_min = float(lr_min)
        self.warmup_t = warmup_t  # the reference configs compute it as a float (1 % of the run)
        self.warmup_lr_init = float(warmup_lr_init)
        self.t_in_epochs = t_in_epochs
        self.base_values = [g.get("initial_lr", g["lr"]) for g in optimizer.param_groups]
        self._last_epoch = 0
        self.step(epoch=0)

    def _get_lr(self, t):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * (lr - self.warmup_lr_init) / self.warmup_t
                    for lr in self.base_values]
        if t >= self.t_initial:
            return [self.lr_min for _ in self.base_values]
        c = 0.5 * (1.0 + math.cos(math.pi * t / self.t_initial))
        return [self.lr_min + (lr - self.lr_min) * c for lr in self.base_values]

    def step(self, epoch=None):
        self._last_epoch = self._last_epoch + 1 if epoch is None else epoch
        for g, lr in zip(self.optimizer.param_groups, self._get_lr(self._last_epoch)):
            g["lr"] = lr

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        """timm Scheduler.state_dict keys (the instance __dict__ minus the optimizer)."""
        return {"_last_epoch": self._last_epoch, "t_initial": self.t_initial,
                "lr_min": self.lr_min, "warmup_t": self.warmup_t,
                "warmup_lr_init": self.warmup_lr_init, "t_in_epochs": self.t_in_epochs,
                "cycle_mul": 1.0, "cycle_decay": 1.0, "cycle_limit": 1, "warmup_prefix": False,
                "k_decay": 1.0, "base_values": list(self.base_values)}

    def load_state_dict(self, sd):
        self.step(epoch=int(sd["_last_epoch"]))


SCHEDULERS = {"linear_warmup": LinearLRSchedulerWarmup, "cosine_warmup_timm": TimmCosineLRScheduler}
