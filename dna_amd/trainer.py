"""Training step engine for DNABERT-2 MLM pretraining (replaces the Lightning fit loop's
per-batch work: SequenceLightningModule._shared_step/training_step, train.py:339-440, plus
Lightning's backward, DDP gradient all-reduce, clip_grad_norm_ and AdamW/scheduler steps).

One step = embedding/encoder/head forward on HIP kernels -> fused masked-CE loss -> backward
(gradient buckets all-reduced over RCCL as they complete) -> global-norm clip + AdamW on the
flat buffers -> LR schedule. No host synchronisation inside a step: the batch's row indices
(MLMIndex) are computed on the host while it is collated.
"""
import math
from dataclasses import dataclass

import torch
import torch.distributed as dist

from .bert_layers import BertForMaskedLM, BertForSequenceClassification, MLMIndex
from .ddp import GradBucketReducer, broadcast_
from .flat import FlatParams
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
    return v


class ModuleTrainer:
    """The same data-parallel step for any model (BASELINE configs D / E: HyenaDNA, Caduceus):
    parameters and gradients in one flat buffer (FlatParams), gradient buckets all-reduced over
    RCCL as they complete in the backward (GradBucketReducer, fp32 or bf16 wire), global-norm clip
    + AdamW in one fused launch (FusedAdamW), the 1/world average folded into it. `loss_fn(model,
    batch)` returns the scalar loss; with `autocast` set it runs under torch.autocast (the configs'
    bf16 mixed precision: fp32 master weights, bf16 compute)."""

    def __init__(self, model, device, loss_fn, lr=1e-3, weight_decay=0.0, betas=(0.9, 0.999),
                 eps=1e-8, max_grad_norm=1.0, bucket_mb=25.0, wire_dtype="fp32",
                 autocast=torch.bfloat16, groups=None):
        """groups: an optim.ParamGroups of `model` (opt-in): the flat buffers are laid out by it
        and AdamW steps each `_optim` group with its own hyperparameters."""
        self.model = model.to(device).train()
        self.device = torch.device(device)
        self.loss_fn = loss_fn
        self.autocast = autocast
        # bf16 autocast: a persistent bf16 copy of every parameter, rewritten by the fused AdamW
        # step, stands in for autocast's per-forward weight casts where the kernels read it
        # (mamba._lowp: `_dna_lp` on the parameter)
        lowp = autocast == torch.bfloat16 and torch.device(device).type == "cuda"
        self.flat = FlatParams(self.model, device, shadow_dtype=torch.bfloat16 if lowp else None,
                               group_of=groups)
        if lowp:
            for p in self.flat.params:
                p._dna_lp = self.flat.lp(p)
        # weight gradients the hand-written kernels can write into the flat buffer go there
        # directly (no returned dW, no AccumulateGrad add); others return theirs as before
        self.flat.enable_direct_grad(True)
        self.opt = FusedAdamW(self.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                              max_grad_norm=max_grad_norm, groups=groups)
        self.ln_guard = LNFromYGuard(self.flat, self.opt)
        self.reducer = GradBucketReducer(self.flat, bucket_mb=bucket_mb, wire_dtype=wire_dtype)
        self.world = self.reducer.world
        if self.reducer.enabled:  # DDP construction broadcast
            broadcast_(self.flat.flat, src=0)
        self._versions = _sync_shadow(self.flat, None)  # bf16 copy of the (broadcast) weights
        self.global_step = 0

    def step(self, batch) -> torch.Tensor:
        self._versions = _sync_shadow(self.flat, self._versions)
        self.ln_guard.poll()
        self.opt.zero_grad()
        self.reducer.prepare(sync=True)
        if self.autocast is not None:
            with torch.autocast(self.device.type, dtype=self.autocast):
                loss = self.loss_fn(self.model, batch)
        else:
            loss = self.loss_fn(self.model, batch)
        loss.backward()
        self.reducer.finish()
        self.opt.step(grad_scale=self.reducer.grad_scale)
        self.ln_guard.launch()
        self.global_step += 1
        return loss.detach()


class MLMTrainer:
    def __init__(self, model: BertForMaskedLM, device, lr=5e-4, weight_decay=1e-5,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, scheduler=None,
                 bucket_mb=25.0, seed=None, wire_dtype="fp32"):
        self.model = model.to(device).train()
        self.device = device
        self.flat = FlatParams(self.model, device)
        self.flat.enable_direct_grad(True)
        self.opt = FusedAdamW(self.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                              max_grad_norm=max_grad_norm)
        self.ln_guard = LNFromYGuard(self.flat, self.opt)
        self.sched = None
        if scheduler is not None:
            self.sched = LinearLRSchedulerWarmup(self.opt, **scheduler)
        self.reducer = GradBucketReducer(self.flat, bucket_mb=bucket_mb, wire_dtype=wire_dtype)
        self.world = self.reducer.world
        if self.reducer.enabled:  # DDP construction broadcast (C2 in SURVEY §2.2)
            broadcast_(self.flat.flat, src=0)
        # dropout stream: derived from train.seed when given, and distinct per rank
        rank = dist.get_rank() if dist.is_initialized() else 0
        base = self.model.dropout_rng.seed if seed is None else int(seed) + 0x5EED
        self.model.dropout_rng.seed = (base * 1000003 + rank) & (2 ** 63 - 1)
        self.global_step = 0
        self._versions = _sync_shadow(self.flat, None)
        self.micro_losses = []  # undivided loss of each micro-batch of the last step (metrics)

    def rng_state(self):
        """Dropout stream position, saved in checkpoints so a resume does not replay masks."""
        r = self.model.dropout_rng
        return {"seed": int(r.seed), "offset": int(r.offset)}

    def load_rng_state(self, st, rank=0):
        """rank: added to the saved seed (a checkpoint holds rank 0's stream; every rank draws
        its own, as __init__ derives them)."""
        self.model.dropout_rng.seed = (int(st["seed"]) + int(rank)) & (2 ** 63 - 1)
        self.model.dropout_rng.offset = int(st["offset"])

    def device_batch(self, masked_ids, mask, labels, target, pad_token_id=3):
        """Collated CPU tensors -> the batch `step` and the model's mlm_loss take."""
        return DeviceBatch.from_host(masked_ids, mask, labels, target, self.device, pad_token_id)

    def step(self, batch, accum=None) -> torch.Tensor:
        """One optimizer step over one micro-batch or a list of them (accumulate_grad_batches:
        each micro-batch loss is divided by `accum` -- default their number -- like Lightning,
        which divides by accumulate_grad_batches even in an epoch's short last window;
        gradients are all-reduced only during the last micro-batch's backward, like DDP
        no_sync)."""
        micro = batch if isinstance(batch, (list, tuple)) else [batch]
        div = len(micro) if accum is None else int(accum)
        self._versions = _sync_shadow(self.flat, self._versions)
        self.ln_guard.poll()
        self.opt.zero_grad()
        total = None
        self.micro_losses = []
        for i, mb in enumerate(micro):
            last = i == len(micro) - 1
            self.reducer.prepare(sync=last)
            loss, _ = self.model.mlm_loss(mb.masked_ids, mb.mask, mb.index, mb.n_mask,
                                          mb.n_unk_masked)
            self.micro_losses.append(loss.detach())
            if div > 1:
                loss = loss / div
            loss.backward()
            total = loss.detach() if total is None else total + loss.detach()
        self.reducer.finish()
        self.opt.step(grad_scale=self.reducer.grad_scale)
        if self.sched is not None:
            self.sched.step()
        self.ln_guard.launch()
        self.global_step += 1
        return total


def load_backbone(model, path):
    """Load a Lightning-layout MLM checkpoint (train.py save_checkpoint: {"state_dict":
    {"model.<key>": ...}}; a bare state dict works too) into a BertForSequenceClassification,
    non-strictly. -> (missing keys, unexpected keys): for an MLM checkpoint the pooler and
    classifier keys (they keep their initialisation) and the `cls.*` MLM-head keys."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = ck.get("state_dict", ck)
    sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    return list(missing), list(unexpected)


class ClsTrainer:
    """Fine-tuning step engine for BertForSequenceClassification, next to MLMTrainer: flat fp32
    parameters / gradients with the bf16 shadow, the fused head kernels writing their parameter
    gradients straight into the flat buffer, global-norm clip + AdamW in one launch, LR schedule,
    dropout-stream state for checkpoints. Single GPU (multi-rank fine-tuning is not built)."""

    def __init__(self, model: BertForSequenceClassification, device, lr=3e-5, weight_decay=0.01,
                 betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, scheduler=None, seed=None):
        if dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("ClsTrainer: single-GPU fine-tuning only")
        self.model = model.to(device).train()
        self.device = device
        self.flat = FlatParams(self.model, device)
        self.flat.enable_direct_grad(True)
        self.opt = FusedAdamW(self.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                              max_grad_norm=max_grad_norm)
        self.ln_guard = LNFromYGuard(self.flat, self.opt)
        self.sched = LinearLRSchedulerWarmup(self.opt, **scheduler) if scheduler else None
        base = self.model.dropout_rng.seed if seed is None else int(seed) + 0x5EED
        self.model.dropout_rng.seed = (base * 1000003) & (2 ** 63 - 1)
        self.global_step = 0
        self._versions = _sync_shadow(self.flat, None)
        self.last_logits = None
        self.last_pred = None

    def rng_state(self):
        r = self.model.dropout_rng
        return {"seed": int(r.seed), "offset": int(r.offset)}

    def load_rng_state(self, st):
        self.model.dropout_rng.seed = int(st["seed"])
        self.model.dropout_rng.offset = int(st["offset"])

    def step(self, input_ids, labels) -> torch.Tensor:
        """One optimizer step on one batch (ids [b, S] and labels on the device). The logits and
        (single-label) predictions of the step stay in last_logits / last_pred; no host sync."""
        self._versions = _sync_shadow(self.flat, self._versions)
        self.ln_guard.poll()
        self.opt.zero_grad()
        logits, loss, pred = self.model.cls_logits(input_ids, labels)
        loss.backward()
        self.opt.step()
        if self.sched is not None:
            self.sched.step()
        self.ln_guard.launch()
        self.global_step += 1
        self.last_logits, self.last_pred = logits.detach(), pred
        return loss.detach()

    @torch.no_grad()
    def evaluate(self, input_ids, labels=None):
        """Eval-mode forward -> (logits, loss | None, pred | None); restores the training mode."""
        was = self.model.training
        self.model.eval()
        try:
            self._versions = _sync_shadow(self.flat, self._versions)
            return self.model.cls_logits(input_ids, labels)
        finally:
            self.model.train(was)


class SeqClsTrainer(ModuleTrainer):
    """Fine-tuning step engine for the pooling-head classifiers (decoders.SequenceClassifier over
    DNAEmbeddingModel, CaduceusForSequenceClassification; any model with
    `cls_logits(input_ids, labels) -> (logits, loss, pred)`): ModuleTrainer's step -- flat fp32
    parameters with the bf16 shadow under bf16 autocast, the head's dW / dbias added straight
    into the flat gradient, clip + AdamW in one launch -- plus ClsTrainer's interface: LR
    schedule, last_logits / last_pred, evaluate, RNG state for checkpoints. These models draw
    their dropout from torch's generators, so that is the state kept. Single GPU."""

    def __init__(self, model, device, lr=6e-4, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=1.0, scheduler=None, seed=None, autocast=torch.bfloat16):
        if dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("SeqClsTrainer: single-GPU fine-tuning only")
        if seed is not None:
            torch.manual_seed(int(seed) + 0x5EED)
        super().__init__(model, device, self._loss, lr=lr, weight_decay=weight_decay, betas=betas,
                         eps=eps, max_grad_norm=max_grad_norm, autocast=autocast)
        self.sched = LinearLRSchedulerWarmup(self.opt, **scheduler) if scheduler else None
        self.opt.numel = self._trainable_extent()
        self.last_logits = None
        self.last_pred = None

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
        from .flat import ALIGN
        return min((end + ALIGN - 1) // ALIGN * ALIGN, flat.numel)  # slices start ALIGN-aligned

    def _loss(self, model, batch):
        logits, loss, pred = model.cls_logits(*batch)
        self.last_logits, self.last_pred = logits.detach(), pred
        return loss

    def rng_state(self):
        st = {"cpu": torch.get_rng_state()}
        if self.device.type == "cuda":
            st["cuda"] = torch.cuda.get_rng_state(self.device)
        return st

    def load_rng_state(self, st):
        torch.set_rng_state(st["cpu"])
        if "cuda" in st and self.device.type == "cuda":
            torch.cuda.set_rng_state(st["cuda"], self.device)

    def step(self, input_ids, labels) -> torch.Tensor:
        """One optimizer step on one batch (ids and labels on the device); no host sync."""
        loss = super().step((input_ids, labels))
        if self.sched is not None:
            self.sched.step()
        return loss

    @torch.no_grad()
    def evaluate(self, input_ids, labels=None):
        """Eval-mode forward -> (logits, loss | None, pred | None); restores the training mode."""
        was = self.model.training
        self.model.eval()
        try:
            self._versions = _sync_shadow(self.flat, self._versions)
            if self.autocast is not None:
                with torch.autocast(self.device.type, dtype=self.autocast):
                    return self.model.cls_logits(input_ids, labels)
            return self.model.cls_logits(input_ids, labels)
        finally:
            self.model.train(was)


class BlmTrainer(ModuleTrainer):
    """Masked-LM pretraining step engine for hyena_lm.BertLMHeadModel (registry model "blm"):
    ModuleTrainer's step -- flat fp32 parameters with the bf16 shadow under bf16 autocast,
    gradient buckets all-reduced as the backward completes them, clip + AdamW fused -- with
    MLMTrainer's interface, which train.py drives: step(batch | [micro-batches], accum), sched,
    micro_losses, rng_state / load_rng_state, device_batch. The Hyena filter's parameters
    (`_optim`: their own lr, no weight decay) step in AdamW groups of their own
    (optim.ParamGroups). These models draw dropout from torch's generators, so that is the RNG
    state kept; it is seeded with seed + rank. precision: autocast=torch.bfloat16 or None (fp32)."""

    def __init__(self, model, device, lr=6e-4, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=1.0, scheduler=None, scheduler_name="cosine_warmup_timm",
                 bucket_mb=25.0, seed=None, wire_dtype="fp32", autocast=torch.bfloat16):
        rank = dist.get_rank() if dist.is_initialized() else 0
        if seed is not None:
            torch.manual_seed(int(seed) + rank)
        super().__init__(model, device, None, lr=lr, weight_decay=weight_decay, betas=betas,
                         eps=eps, max_grad_norm=max_grad_norm, bucket_mb=bucket_mb,
                         wire_dtype=wire_dtype, autocast=autocast, groups=ParamGroups(model))
        self.sched = SCHEDULERS[scheduler_name](self.opt, **scheduler) if scheduler else None
        self.vocab_size = int(self.model.lm_head.weight.shape[0])
        self.micro_losses = []  # undivided loss of each micro-batch of the last step (metrics)

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

    def _loss(self, mb):
        if self.autocast is not None:
            with torch.autocast(self.device.type, dtype=self.autocast):
                return self.model.mlm_loss(mb.masked_ids, mb.mask, mb.index, mb.n_mask,
                                           mb.n_unk_masked)[0]
        return self.model.mlm_loss(mb.masked_ids, mb.mask, mb.index, mb.n_mask,
                                   mb.n_unk_masked)[0]

    def step(self, batch, accum=None) -> torch.Tensor:
        """One optimizer step over one micro-batch or a list of them; MLMTrainer.step's
        contract: each micro-batch loss is divided by `accum` (default their number), gradients
        are all-reduced only during the last micro-batch's backward."""
        micro = batch if isinstance(batch, (list, tuple)) else [batch]
        div = len(micro) if accum is None else int(accum)
        self._versions = _sync_shadow(self.flat, self._versions)
        self.ln_guard.poll()
        self.opt.zero_grad()
        total = None
        self.micro_losses = []
        for i, mb in enumerate(micro):
            self.reducer.prepare(sync=i == len(micro) - 1)
            loss = self._loss(mb)
            self.micro_losses.append(loss.detach())
            if div > 1:
                loss = loss / div
            loss.backward()
            total = loss.detach() if total is None else total + loss.detach()
        self.reducer.finish()
        self.opt.step(grad_scale=self.reducer.grad_scale)
        if self.sched is not None:
            self.sched.step()
        self.ln_guard.launch()
        self.global_step += 1
        return total
