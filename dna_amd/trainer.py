"""Training step engine for DNABERT-2 MLM pretraining (replaces the Lightning fit loop's
per-batch work: SequenceLightningModule._shared_step/training_step, train.py:339-440, plus
Lightning's backward, DDP gradient all-reduce, clip_grad_norm_ and AdamW/scheduler steps).

One step = embedding/encoder/head forward on HIP kernels -> fused masked-CE loss -> backward
(gradient buckets all-reduced over RCCL as they complete) -> global-norm clip + AdamW on the
flat buffers -> LR schedule. No host synchronisation inside a step: the batch's row indices
(MLMIndex) are computed on the host while it is collated.

ModuleTrainer holds that step and the construction of what it needs, once. The named trainers
add what is their own: the loss of a micro-batch, the public `step` signature, the seed and the
RNG state kept in checkpoints.
"""
import contextlib
from dataclasses import dataclass

import torch
import torch.distributed as dist

from .bert_layers import BertForMaskedLM, BertForSequenceClassification, MLMIndex
from .ddp import GradBucketReducer, broadcast_
from .flat import ALIGN, FlatParams
from .functional import LNFromYGuard
from .optim import SCHEDULERS, FusedAdamW, LinearLRSchedulerWarmup, ParamGroups


@dataclass
class DeviceBatch:
    masked_ids: torch.Tensor  # [b, S] int64 on device
    mask: torch.Tensor        # [b, S] bool
    labels: torch.Tensor      # [b, S] int64
    target: torch.Tensor      # [b, S] int64 (original ids)
    index: MLMIndex           # on device
    n_mask: int
    n_unk_masked: int

    @staticmethod
    def from_host(masked_ids, mask, labels, target, device, pad_token_id=3):
        """Collated CPU tensors -> device batch; row bookkeeping done on the host (no GPU sync)."""
        idx = MLMIndex.build(masked_ids, labels, pad_token_id)
        n_mask = int(mask.sum())
        n_unk = n_mask - int(idx.target.numel())
        pin = lambda t: t.pin_memory() if torch.cuda.is_available() else t
        dev = lambda t: pin(t).to(device, non_blocking=True)
        return DeviceBatch(dev(masked_ids), dev(mask), dev(labels), dev(target),
                           MLMIndex(*(dev(t) for t in (idx.subset_idx, idx.head_idx, idx.target,
                                                       idx.flat_masked))), n_mask, n_unk)


def _sync_shadow(flat, versions):
    """Re-derive the bf16 parameter copy when a parameter was changed in place outside the fused
    AdamW step (load_state_dict, a manual edit): torch bumps the tensor's version counter then, the
    AdamW kernel (raw pointers) does not. Returns the versions to compare against next step."""
    if flat.shadow is None:
        return None
    v = [p._version for p in flat.params]
    if v != versions:
        flat.refresh_shadow()
        # the version the copy stands for: a reader outside the trainer (functional._shadow) takes
        # the copy only while the parameter still has it, and casts the parameter otherwise
        for p, pv in zip(flat.params, v):
            p._dna_lp_version = pv
    return v


def _rank():
    return dist.get_rank() if dist.is_initialized() else 0


def _single_gpu_only(name):
    if dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f"{name}: single-GPU fine-tuning only")


def _micro_batches(batch, accum):
    """step(batch | [micro-batches], accum) of the pretraining trainers -> (micro-batches,
    divisor): a list or tuple is micro-batches, and the divisor defaults to their number."""
    micro = batch if isinstance(batch, (list, tuple)) else [batch]
    return micro, len(micro) if accum is None else int(accum)


def _mlm_loss(model, mb):
    return model.mlm_loss(mb.masked_ids, mb.mask, mb.index, mb.n_mask, mb.n_unk_masked)[0]


class _DropoutStreamState:
    """RNG state of the BERT trainers, whose models draw dropout from their own counter-based
    stream (functional.DropoutRNG): its (seed, offset)."""

    def _seed_stream(self, seed, rank=0):
        """The stream's seed: derived from train.seed when given, and distinct per rank."""
        base = self.model.dropout_rng.seed if seed is None else int(seed) + 0x5EED
        self.model.dropout_rng.seed = (base * 1000003 + rank) & (2 ** 63 - 1)

    def rng_state(self):
        """Dropout stream position, saved in checkpoints so a resume does not replay masks."""
        r = self.model.dropout_rng
        return {"seed": int(r.seed), "offset": int(r.offset)}

    def load_rng_state(self, st, rank=0):
        """rank: added to the saved seed (a checkpoint holds rank 0's stream; every rank draws
        its own, as _seed_stream derives them)."""
        self.model.dropout_rng.seed = (int(st["seed"]) + int(rank)) & (2 ** 63 - 1)
        self.model.dropout_rng.offset = int(st["offset"])


class _TorchGeneratorState:
    """RNG state of the trainers whose models draw dropout from torch's generators: the CPU's and
    the device's."""

    def rng_state(self):
        st = {"cpu": torch.get_rng_state()}
        if self.device.type == "cuda":
            st["cuda"] = torch.cuda.get_rng_state(self.device)
        return st

    def load_rng_state(self, st, rank=0):
        """A checkpoint holds rank 0's generator states; the other ranks keep the streams their
        own seed gave them (distinct per rank, not replayed)."""
        if rank:
            return
        torch.set_rng_state(st["cpu"])
        if "cuda" in st and self.device.type == "cuda":
            torch.cuda.set_rng_state(st["cuda"], self.device)


class ModuleTrainer:
    """The same data-parallel step for any model (BASELINE configs D / E: HyenaDNA, Caduceus):
    parameters and gradients in one flat buffer (FlatParams), gradient buckets all-reduced over
    RCCL as they complete in the backward (GradBucketReducer, fp32 or bf16 wire), global-norm clip
    + AdamW in one fused launch (FusedAdamW), the 1/world average folded into it. `loss_fn(model,
    batch)` returns the scalar loss; with `autocast` set it runs under torch.autocast (the configs'
    bf16 mixed precision: fp32 master weights, bf16 compute)."""

    # the schedule steps before the LayerNorm guard's check is launched (see SeqClsTrainer)
    _sched_before_guard = True

    def __init__(self, model, device, loss_fn, lr=1e-3, weight_decay=0.0, betas=(0.9, 0.999),
                 eps=1e-8, max_grad_norm=1.0, bucket_mb=25.0, wire_dtype="fp32",
                 autocast=torch.bfloat16, groups=None, lp_tags=True):
        """groups: an optim.ParamGroups of `model` (opt-in): the flat buffers are laid out by it
        and AdamW steps each `_optim` group with its own hyperparameters.
        lp_tags: who finds the bf16 copy of the parameters. True: the kernels, through `_dna_lp`
        on each parameter, and the copy exists only under bf16 autocast on a GPU. False: the model,
        through FlatParams' `_lp_provider` and its own precision setting (the BERT models); the
        copy is then always built."""
        self.model = model.to(device).train()
        self.device = torch.device(device)
        self.loss_fn = loss_fn
        self.autocast = autocast
        # bf16 autocast: a persistent bf16 copy of every parameter, rewritten by the fused AdamW
        # step, stands in for autocast's per-forward weight casts where the kernels read it
        # (mamba._lowp: `_dna_lp` on the parameter)
        lowp = not lp_tags or (autocast == torch.bfloat16 and self.device.type == "cuda")
        self.flat = FlatParams(self.model, device, shadow_dtype=torch.bfloat16 if lowp else None,
                               group_of=groups)
        if lowp and lp_tags:
            for p in self.flat.params:
                p._dna_lp = self.flat.lp(p)
        # weight gradients the hand-written kernels can write into the flat buffer go there
        # directly (no returned dW, no AccumulateGrad add); others return theirs as before
        self.flat.enable_direct_grad(True)
        self.opt = FusedAdamW(self.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                              max_grad_norm=max_grad_norm, groups=groups)
        self.ln_guard = LNFromYGuard(self.flat, self.opt)
        self.sched = None
        self.reducer = GradBucketReducer(self.flat, bucket_mb=bucket_mb, wire_dtype=wire_dtype)
        self.world = self.reducer.world
        if self.reducer.enabled:  # DDP construction broadcast (C2 in SURVEY §2.2)
            broadcast_(self.flat.flat, src=0)
        self._versions = _sync_shadow(self.flat, None)  # bf16 copy of the (broadcast) weights
        self.global_step = 0
        self.micro_losses = []  # undivided loss of each micro-batch of the last step (metrics)

    def _autocast(self):
        if self.autocast is None:
            return contextlib.nullcontext()
        return torch.autocast(self.device.type, dtype=self.autocast)

    def _loss(self, batch):
        """The scalar loss of one micro-batch."""
        with self._autocast():
            return self.loss_fn(self.model, batch)

    def _run(self, micro_batches, div):
        """One optimizer step over the micro-batches (accumulate_grad_batches: each loss is
        divided by `div` like Lightning, which divides by accumulate_grad_batches even in an
        epoch's short last window; gradients are all-reduced only during the last micro-batch's
        backward, like DDP no_sync). -> the sum of the divided losses."""
        self._versions = _sync_shadow(self.flat, self._versions)
        self.ln_guard.poll()
        self.opt.zero_grad()
        total = None
        self.micro_losses = []
        for i, mb in enumerate(micro_batches):
            self.reducer.prepare(sync=i == len(micro_batches) - 1)
            loss = self._loss(mb)
            self.micro_losses.append(loss.detach())
            if div > 1:
                loss = loss / div
            loss.backward()
            total = loss.detach() if total is None else total + loss.detach()
        self.reducer.finish()
        self.opt.step(grad_scale=self.reducer.grad_scale)
        if self.sched is not None and self._sched_before_guard:
            self.sched.step()
        self.ln_guard.launch()
        if self.sched is not None and not self._sched_before_guard:
            self.sched.step()
        self.global_step += 1
        return total

    def step(self, batch) -> torch.Tensor:
        """One optimizer step on one batch, which goes to loss_fn as it is (a tuple too)."""
        return self._run([batch], 1)


class MLMTrainer(_DropoutStreamState, ModuleTrainer):
    def __init__(self, model: BertForMaskedLM, device, lr=5e-4, weight_decay=1e-5,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, scheduler=None,
                 bucket_mb=25.0, seed=None, wire_dtype="fp32"):
        super().__init__(model, device, _mlm_loss, lr=lr, weight_decay=weight_decay, betas=betas,
                         eps=eps, max_grad_norm=max_grad_norm, bucket_mb=bucket_mb,
                         wire_dtype=wire_dtype, autocast=None, lp_tags=False)
        if scheduler is not None:
            self.sched = LinearLRSchedulerWarmup(self.opt, **scheduler)
        self._seed_stream(seed, _rank())

    def device_batch(self, masked_ids, mask, labels, target, pad_token_id=3):
        """Collated CPU tensors -> the batch `step` and the model's mlm_loss take."""
        return DeviceBatch.from_host(masked_ids, mask, labels, target, self.device, pad_token_id)

    def step(self, batch, accum=None) -> torch.Tensor:
        """One optimizer step over one micro-batch or a list of them, each loss divided by
        `accum` (default their number)."""
        return self._run(*_micro_batches(batch, accum))


def strip_model_prefix(state_dict):
    """A checkpoint's state dict without the "model." prefix that train.py's and finetune.py's
    checkpoints (Lightning's layout) put on every key."""
    return {(k[len("model."):] if k.startswith("model.") else k): v for k, v in state_dict.items()}


def load_backbone(model, path, strict=False):
    """Load a Lightning-layout MLM checkpoint (train.py save_checkpoint: {"state_dict":
    {"model.<key>": ...}}; a bare state dict works too) into a BertForSequenceClassification,
    non-strictly. -> (missing keys, unexpected keys): for an MLM checkpoint the pooler and
    classifier keys (they keep their initialisation) and the `cls.*` MLM-head keys."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    missing, unexpected = model.load_state_dict(strip_model_prefix(ck.get("state_dict", ck)),
                                                strict=strict)
    return list(missing), list(unexpected)


class _ClsSteps(ModuleTrainer):
    """What the two fine-tuning trainers share: a model with `cls_logits(input_ids, labels) ->
    (logits, loss, pred)`, step(input_ids, labels), last_logits / last_pred, evaluate, a
    schedule (scheduler_name: linear_warmup, or cosine_warmup_timm with optim's refusals). Single
    GPU (multi-rank fine-tuning is not built)."""

    def __init__(self, model, device, scheduler, scheduler_name="linear_warmup", **kw):
        if scheduler_name not in SCHEDULERS:
            raise NotImplementedError(f"scheduler {scheduler_name!r}: one of {sorted(SCHEDULERS)}")
        super().__init__(model, device, self._cls_loss, **kw)
        self.sched = self._make_sched(self.opt, scheduler, scheduler_name)
        self.last_logits = None
        self.last_pred = None

    @staticmethod
    def _make_sched(opt, scheduler, scheduler_name="linear_warmup"):
        """The schedule the constructor attaches to its optimizer: `scheduler` (keyword
        arguments, None: no schedule) on the class `scheduler_name` names in optim.SCHEDULERS."""
        return SCHEDULERS[scheduler_name](opt, **scheduler) if scheduler else None

    def _cls_loss(self, model, batch):
        input_ids, labels, packed = batch
        # the index goes on as a keyword only when there is one: a model without a packed path
        # (SeqClsTrainer's) rejects the unknown argument itself
        kw = {} if packed is None else {"packed": packed}
        logits, loss, pred = model.cls_logits(input_ids, labels, **kw)
        self.last_logits, self.last_pred = logits.detach(), pred
        return loss

    def step(self, input_ids, labels, packed=None) -> torch.Tensor:
        """One optimizer step on one batch (ids [b, S] and labels on the device: int64 [b] for a
        single-label head, fp32 [b, C] for a regression or multi-label one). The logits and
        (single-label; None otherwise) predictions of the step stay in last_logits / last_pred;
        no host sync. packed: the batch's PackedIndex on the device (BertForSequenceClassification
        only): the encoder runs on the real tokens instead of the padded rectangle."""
        return self._run([(input_ids, labels, packed)], 1)

    @torch.no_grad()
    def evaluate(self, input_ids, labels=None, packed=None):
        """Eval-mode forward -> (logits, loss | None, pred | None); restores the training mode."""
        was = self.model.training
        self.model.eval()
        try:
            self._versions = _sync_shadow(self.flat, self._versions)
            with self._autocast():
                kw = {} if packed is None else {"packed": packed}
                return self.model.cls_logits(input_ids, labels, **kw)
        finally:
            self.model.train(was)


class ClsTrainer(_DropoutStreamState, _ClsSteps):
    """Fine-tuning step engine for BertForSequenceClassification, next to MLMTrainer: flat fp32
    parameters / gradients with the bf16 shadow, the fused head kernels writing their parameter
    gradients straight into the flat buffer, global-norm clip + AdamW in one launch, LR schedule,
    dropout-stream state for checkpoints. Single GPU."""

    def __init__(self, model: BertForSequenceClassification, device, lr=3e-5, weight_decay=0.01,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, scheduler=None, seed=None,
                 scheduler_name="linear_warmup"):
        _single_gpu_only("ClsTrainer")
        super().__init__(model, device, scheduler, scheduler_name, lr=lr,
                         weight_decay=weight_decay, betas=betas,
                         eps=eps, max_grad_norm=max_grad_norm, autocast=None, lp_tags=False)
        self._seed_stream(seed)


class SeqClsTrainer(_TorchGeneratorState, _ClsSteps):
    """Fine-tuning step engine for the pooling-head classifiers (decoders.SequenceClassifier over
    DNAEmbeddingModel, CaduceusForSequenceClassification; any model with
    `cls_logits(input_ids, labels) -> (logits, loss, pred)`): ModuleTrainer's step -- flat fp32
    parameters with the bf16 shadow under bf16 autocast, the head's dW / dbias added straight
    into the flat gradient, clip + AdamW in one launch -- plus ClsTrainer's interface: LR
    schedule, last_logits / last_pred, evaluate, RNG state for checkpoints. These models draw
    their dropout from torch's generators, so that is the state kept. Single GPU."""

    # The schedule steps after the guard's check is launched. The check's margin is MAX_AGE steps
    # at max(lr, initial_lr) of group 0: while the schedule stays at or under the base lr the order
    # makes no difference, but one that goes over it (warmup_lr_init or lr_min above lr,
    # cycle_decay > 1, all of which finetune.py passes on from the config) hands the check another
    # lr in the other order, and with it possibly another LayerNorm backward path. The same holds
    # for cosine_warmup_timm: warmup rises from warmup_lr_init to the base lr, the cosine falls
    # from it to lr_min, so with warmup_lr_init and lr_min at or under lr (the Nucleotide
    # Transformer experiments: 1e-6 and 0.1 lr) it never exceeds the base lr either.
    _sched_before_guard = False

    def __init__(self, model, device, lr=6e-4, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=1.0, scheduler=None, seed=None, autocast=torch.bfloat16,
                 scheduler_name="linear_warmup"):
        _single_gpu_only("SeqClsTrainer")
        if seed is not None:
            torch.manual_seed(int(seed) + 0x5EED)
        super().__init__(model, device, scheduler, scheduler_name, lr=lr,
                         weight_decay=weight_decay, betas=betas,
                         eps=eps, max_grad_norm=max_grad_norm, autocast=autocast)
        self.opt.numel = self._trainable_extent()

    def _trainable_extent(self):
        """How far into the flat buffers the optimizer steps. Frozen parameters (requires_grad
        False: hyena_lm.load_backbone(freeze_backbone=True)) must get no update and no weight
        decay. FlatParams lays parameters out in reverse registration order, so a frozen model
        under a trainable decoder is the tail of the buffer and the step simply stops before it;
        any other pattern of frozen parameters is refused."""
        flat = self.flat
        end = 0
        for p, (o, n, _) in zip(flat.params, flat.slices):
            if p.requires_grad:
                end = max(end, o + n)
        if end == 0:
            raise ValueError("SeqClsTrainer: no parameter requires a gradient")
        inside = [n for p, (o, n, _) in zip(flat.params, flat.slices)
                  if not p.requires_grad and o < end]
        if inside:
            raise NotImplementedError(
                f"SeqClsTrainer: {len(inside)} frozen parameters are registered after trainable "
                "ones; only a frozen leading sub-module (the backbone under its head) is built")
        return min((end + ALIGN - 1) // ALIGN * ALIGN, flat.numel)  # slices start ALIGN-aligned


class BlmTrainer(_TorchGeneratorState, ModuleTrainer):
    """Masked-LM pretraining step engine for hyena_lm.BertLMHeadModel (registry model "blm") and
    caduceus.CaduceusForMaskedLM (registry model "caduceus") -- any model with `mlm_loss(...)`
    and `lm_head.weight`: ModuleTrainer's step -- flat fp32 parameters with the bf16 shadow under
    bf16 autocast,
    gradient buckets all-reduced as the backward completes them, clip + AdamW fused -- with
    MLMTrainer's interface, which train.py drives: step(batch | [micro-batches], accum), sched,
    micro_losses, rng_state / load_rng_state, device_batch. The Hyena filter's parameters
    (`_optim`: their own lr, no weight decay) step in AdamW groups of their own
    (optim.ParamGroups). These models draw dropout from torch's generators, so that is the RNG
    state kept; it is seeded with seed + rank. precision: autocast=torch.bfloat16 or None (fp32)."""

    def __init__(self, model, device, lr=6e-4, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=1.0, scheduler=None, scheduler_name="cosine_warmup_timm",
                 bucket_mb=25.0, seed=None, wire_dtype="fp32", autocast=torch.bfloat16):
        if seed is not None:
            torch.manual_seed(int(seed) + _rank())
        super().__init__(model, device, _mlm_loss, lr=lr, weight_decay=weight_decay, betas=betas,
                         eps=eps, max_grad_norm=max_grad_norm, bucket_mb=bucket_mb,
                         wire_dtype=wire_dtype, autocast=autocast, groups=ParamGroups(model))
        self.sched = SCHEDULERS[scheduler_name](self.opt, **scheduler) if scheduler else None
        self.vocab_size = int(self.model.lm_head.weight.shape[0])

    def device_batch(self, masked_ids, mask, labels, target, pad_token_id=None):
        """Collated CPU tensors -> device batch; the head's labels (the original id at masked
        positions, -100 elsewhere) and the masked rows are found on the host, where the targets
        are also checked against the vocabulary (no GPU sync)."""
        from .hyena_lm import BlmIndex
        idx = BlmIndex.build(mask, target, self.vocab_size)
        pin = lambda t: t.pin_memory() if torch.cuda.is_available() else t
        dev = lambda t: pin(t).to(self.device, non_blocking=True)
        return DeviceBatch(dev(masked_ids), dev(mask), dev(labels), dev(target),
                           BlmIndex(dev(idx.labels), dev(idx.flat_masked), dev(idx.target)),
                           int(idx.flat_masked.numel()), 0)

    def step(self, batch, accum=None) -> torch.Tensor:
        """One optimizer step over one micro-batch or a list of them; MLMTrainer.step's
        contract."""
        return self._run(*_micro_batches(batch, accum))
