"""DNABERT-2 (MosaicBERT) masked-LM model on dna_amd HIP kernels.

Drop-in for the reference's registry.model["dnabert2"] =
src.models.DNABERT2.bert_layers.BertForMaskedLM (src/utils/registry.py:39):
  * same constructor (`cls(config=<dict-like model.config>)`, bert_layers.py:693-716),
  * same module tree and state_dict keys (tied decoder weight),
  * same forward protocol (`forward(batch, state=None)` with batch = (masked_ids, mask, labels)
    -> (MaskedLMOutput(loss, logits=(scores [b,S,V] zero at labels<=0 rows, mask)), None),
    bert_layers.py:756-843), including the last-layer subset computation (:469-488), the
    zero logit rows for masked [UNK] tokens, and the -10000 key-pad bias.
Differences by design (documented in DESIGN.md): the pad mask comes from `ids != pad_token`
without reloading the tokenizer each forward (reference :786-787); by default the batch stays in
padded layout (no unpad/pad round trips) because pad keys are excluded inside the attention
kernel. With `packed=` (a PackedIndex built on the host) the encoder runs the reference's unpadded
layout instead: the real tokens only, attention per sequence from cu_seqlens.

Compute precision: "bf16" (default; MFMA bf16 kernels, fp32 master weights / LayerNorm /
residual stream, like PL `precision: bf16` autocast) or "fp32" (exact-fp32 kernels; the 1e-3
logit-parity mode).
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import functional as DF
from .config import BertConfig, alibi_slopes

try:  # the reference returns transformers' MaskedLMOutput (bert_layers.py:838-843)
    from transformers.modeling_outputs import MaskedLMOutput
except Exception:  # pragma: no cover - transformers is part of the image; keep a twin anyway
    @dataclass
    class MaskedLMOutput:
        loss: Optional[torch.Tensor] = None
        logits: Optional[object] = None
        hidden_states: Optional[object] = None
        attentions: Optional[object] = None

        def __getitem__(self, i):
            return (self.loss, self.logits)[i]

try:  # BertForSequenceClassification returns transformers' SequenceClassifierOutput (:1004-1009)
    from transformers.modeling_outputs import SequenceClassifierOutput
except Exception:  # pragma: no cover
    @dataclass
    class SequenceClassifierOutput:
        loss: Optional[torch.Tensor] = None
        logits: Optional[torch.Tensor] = None
        hidden_states: Optional[object] = None
        attentions: Optional[object] = None

        def __getitem__(self, i):
            return tuple(v for v in (self.loss, self.logits) if v is not None)[i]

PAD_TOKEN_ID = 3  # DNABERT-2 tokenizer [PAD] (tokenizer.json added_tokens)


class BertEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size,
                                            padding_idx=config.pad_token_id)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)


class BertUnpadSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        if config.hidden_size % config.num_attention_heads != 0:
            raise ValueError(f"The hidden size ({config.hidden_size}) is not a multiple of the "
                             f"number of attention heads ({config.num_attention_heads})")
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = config.hidden_size // config.num_attention_heads
        self.p_dropout = config.attention_probs_dropout_prob
        self.Wqkv = nn.Linear(config.hidden_size, 3 * config.hidden_size)


class BertSelfOutput(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)


class BertUnpadAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self = BertUnpadSelfAttention(config)
        self.output = BertSelfOutput(config)


class BertGatedLinearUnitMLP(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.gated_layers = nn.Linear(config.hidden_size, config.intermediate_size * 2, bias=False)
        self.wo = nn.Linear(config.intermediate_size, config.hidden_size)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.layernorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)


class BertLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = BertUnpadAttention(config)
        self.mlp = BertGatedLinearUnitMLP(config)


class BertEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(config) for _ in range(config.num_hidden_layers)])
        self.num_attention_heads = config.num_attention_heads
        # ALiBi slopes (bert_layers.py:378-396); the [H,S,S] bias itself is never materialised
        self.register_buffer("alibi_slopes",
                             torch.tensor(alibi_slopes(config.num_attention_heads),
                                          dtype=torch.float32), persistent=False)


class BertPooler(nn.Module):
    """tanh(dense(hidden[:, 0])) (reference bert_layers.py:495-510); runs inside the fused head
    kernel (DF.ClsHead / DF.pooler), which reads dense.weight / dense.bias in fp32."""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.activation = nn.Tanh()


def _init_bert_weights(module, std):
    """BertPreTrainedModel._init_weights semantics: N(0, initializer_range) for Linear and
    Embedding weights, zero biases, LayerNorm (1, 0), zero padding_idx row."""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, mean=0.0, std=std)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, mean=0.0, std=std)
            if m.padding_idx is not None:
                with torch.no_grad():
                    m.weight[m.padding_idx].zero_()
        elif isinstance(m, nn.LayerNorm):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)


def _tag_projections(root, skip=()):
    """Projection weights keep a W^T copy for the data gradient dx = dy . W^T^T, where the MFMA
    kernel wants the reduction (out features) % 64 and the output (in features) % 8, as
    dna_transpose_bf16 does; other shapes keep the library dgrad. `skip`: Linear modules whose
    weights only the head kernel reads (pooler.dense, classifier)."""
    for m in root.modules():
        if (isinstance(m, nn.Linear) and m.out_features % 64 == 0 and m.in_features % 8 == 0
                and not any(m is q for q in skip)):
            m.weight._dna_transpose = True


class _HipEncoder:
    """Mixin of the models that run the encoder on the HIP kernels: compute precision, the
    dropout stream, the compute-dtype weight views (FlatParams) and the encoder loop itself.
    `self._bert_model()` is the BertModel holding embeddings and encoder."""

    def _init_hip_encoder(self, precision):
        assert precision in ("bf16", "fp32")
        self.precision = precision
        self.dropout_rng = DF.DropoutRNG()
        self._lp_provider = None  # set by dna_amd.flat.FlatParams for a persistent bf16 copy
        self._lpt_provider = None  # ... and for the transposed bf16 projection weights

    def _bert_model(self):
        return self.bert

    def set_precision(self, precision: str):
        assert precision in ("bf16", "fp32")
        self.precision = precision
        return self

    @property
    def compute_dtype(self):
        return torch.bfloat16 if self.precision == "bf16" else torch.float32

    def _lp(self, p: torch.Tensor) -> torch.Tensor:
        """Compute-dtype view of master weight `p` (persistent shadow if a FlatParams owns it)."""
        if self.precision == "fp32":
            return p
        if self._lp_provider is not None:
            return self._lp_provider(p)
        return p.detach().to(torch.bfloat16)

    def _lp_t(self, p: torch.Tensor):
        """Transposed bf16 copy of projection weight `p` (None: the data gradient falls back)."""
        if self.precision == "fp32" or self._lpt_provider is None:
            return None
        return self._lpt_provider(p)

    def _linear(self, x, w, b=None, geglu=None):
        return DF.linear(x, w, self._lp(w), b, w_lpt=self._lp_t(w), geglu=geglu)

    def _check_inputs(self, input_ids, token_type_ids, attention_mask):
        if input_ids is None:
            raise ValueError("Must specify input_ids (inputs_embeds is not supported)")
        if token_type_ids is not None and bool((token_type_ids != 0).any()):
            raise NotImplementedError("token_type_ids other than 0 (the MLM path never sets them)")
        if attention_mask is not None:
            if not torch.equal(attention_mask.bool(), input_ids != self.config.pad_token_id_mask):
                raise NotImplementedError("attention_mask must equal input_ids != [PAD]")

    def encode(self, input_ids: torch.Tensor, last_rows: Optional[torch.Tensor] = None,
               packed: Optional["PackedIndex"] = None):
        """Embeddings + encoder -> (x fp32, x compute dtype) of the last layer, rows flattened
        over (b, s). last_rows (flattened row indices): the last layer's output projection, MLP
        and LayerNorms run on those rows only and the result holds just them (reference
        :469-488 `subset_mask`). bf16 mode with S % 64 != 0 (the attention kernel's tile): the ids
        are padded with [PAD] to the next multiple of 64 and the outputs sliced back -- pad keys
        are excluded in the kernel and ALiBi depends on i - j only, so valid rows are unchanged.
        packed (a PackedIndex of input_ids, on its device): the reference's unpadded layout
        (unpad_input after the embeddings' gather). Only the T = packed.total real tokens have
        rows: the ids are gathered with packed.indices, every row-wise op runs on T rows, attention
        is the packed kernel, and neither key_valid nor the pad-to-64 step exists. last_rows stays
        in flattened (b, s) coordinates, names real tokens only (a [PAD] has no packed row) and is
        mapped through packed.row_of on the device; the result holds the T packed rows (or the
        subset rows). Dropout draws T * width counters, so its stream
        differs from the padded run's."""
        cfg = self.config
        bert = self._bert_model()
        b, S0 = input_ids.shape
        bf16 = self.precision == "bf16"
        S = S0
        if packed is not None:
            packed.check(input_ids)
            input_ids = input_ids.reshape(-1).index_select(0, packed.indices)
            if last_rows is not None:
                last_rows = packed.row_of.index_select(0, last_rows)
        elif bf16 and S0 % 64:
            S = (S0 + 63) // 64 * 64
            input_ids = torch.nn.functional.pad(input_ids, (0, S - S0), value=cfg.pad_token_id_mask)
            if last_rows is not None:
                last_rows = torch.div(last_rows, S0, rounding_mode="floor") * S + last_rows % S0
        T = b * S if packed is None else packed.total
        H = cfg.num_attention_heads
        train = self.training
        rng = self.dropout_rng
        p_hidden = cfg.hidden_dropout_prob if train else 0.0
        if cfg.attention_probs_dropout_prob and train:
            raise NotImplementedError("attention-probability dropout (reference default 0.0)")
        eps = cfg.layer_norm_eps
        ids = input_ids.reshape(-1)
        key_valid = None if packed is not None else (ids != cfg.pad_token_id_mask).to(torch.uint8)

        emb = bert.embeddings
        seed, off = rng.take(T * cfg.hidden_size) if p_hidden else (0, 0)
        x32, xb = DF.EmbeddingLN.apply(ids, emb.word_embeddings.weight,
                                       emb.token_type_embeddings.weight, emb.LayerNorm.weight,
                                       emb.LayerNorm.bias, eps, p_hidden, seed, off, True, bf16)
        xin = xb if bf16 else x32
        slopes = bert.encoder.alibi_slopes
        L = len(bert.encoder.layer)
        for i, layer in enumerate(bert.encoder.layer):
            att = layer.attention
            qkv = self._linear(xin, att.self.Wqkv.weight, att.self.Wqkv.bias)
            if packed is not None:
                ctx = DF.alibi_attention_varlen(qkv, packed, slopes, H)
            else:
                ctx = DF.alibi_attention(qkv, key_valid, slopes, b, S, H,
                                         bias_grad=att.self.Wqkv.bias is not None)
            res = x32
            if i == L - 1 and last_rows is not None:  # output + MLP on the subset rows (:480-488)
                ctx = ctx.index_select(0, last_rows)
                res = x32.index_select(0, last_rows)
            n = ctx.shape[0]
            out = att.output
            h = self._linear(ctx, out.dense.weight)
            seed, off = rng.take(n * cfg.hidden_size) if p_hidden else (0, 0)
            y32, yb = DF.FusedLayerNorm.apply(h, out.dense.bias, res, out.LayerNorm.weight,
                                              out.LayerNorm.bias, eps, 0, p_hidden, seed, off,
                                              True, bf16)
            mlp = layer.mlp
            seed, off = rng.take(n * cfg.intermediate_size) if p_hidden else (0, 0)
            # the GeGLU forward runs in the gated_layers GEMM's epilogue where the kernel allows
            g = self._linear(yb if bf16 else y32, mlp.gated_layers.weight,
                             geglu=(p_hidden, seed, off))
            wo_lp, wo_lpt = self._lp(mlp.wo.weight), self._lp_t(mlp.wo.weight)
            if DF.geglu_out_fused_ok(g, wo_lp, wo_lpt):
                # GeGLU + wo as one node: backward = wo's data gradient with the GeGLU backward
                # in its epilogue (da never in memory), then wo's weight gradient
                o = DF.geglu_out(g, p_hidden, seed, off, mlp.wo.weight, wo_lp, wo_lpt)
            else:
                a = DF.GeGLU.apply(g, p_hidden, seed, off)
                o = DF.linear(a, mlp.wo.weight, wo_lp, None, w_lpt=wo_lpt)
            x32, xb = DF.FusedLayerNorm.apply(o, mlp.wo.bias, y32, mlp.layernorm.weight,
                                              mlp.layernorm.bias, eps, 0, 0.0, 0, 0, True, bf16)
            xin = xb if bf16 else x32
        if L == 0 and last_rows is not None:
            x32, xin = x32.index_select(0, last_rows), xin.index_select(0, last_rows)
        if packed is None and last_rows is None and S != S0:
            d = x32.shape[1]
            x32 = x32.view(b, S, d)[:, :S0].reshape(b * S0, d)
            xin = xin.view(b, S, d)[:, :S0].reshape(b * S0, d)
        return x32, xin


class BertModel(nn.Module, _HipEncoder):
    """Embeddings + encoder (+ pooler). Inside BertForMaskedLM / BertForSequenceClassification it
    is the parameter container and the owning model runs `encode`; on its own, `forward` is the
    embedding-extraction path (reference bert_layers.py:587-644 without masked_tokens_mask)."""

    def __init__(self, config, add_pooling_layer=False, precision: str = "bf16",
                 init_weights: bool = True):
        super().__init__()
        config = BertConfig.from_any(config)
        self.config = config
        self.embeddings = BertEmbeddings(config)
        self.encoder = BertEncoder(config)
        self.pooler = BertPooler(config) if add_pooling_layer else None
        self._init_hip_encoder(precision)
        if init_weights:  # an owning model initialises the whole tree once instead
            _init_bert_weights(self, config.initializer_range)
            _tag_projections(self.encoder)

    def _bert_model(self):
        return self

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, position_ids=None,
                output_all_encoded_layers=False, masked_tokens_mask=None, packed=None, **kwargs):
        """-> (sequence_output [b, S, hidden] fp32 with zero rows at [PAD] positions, like the
        reference's pad_input, pooled_output [b, hidden] fp32 or None). packed (a PackedIndex of
        input_ids): the encoder runs on the real tokens only and the rows are scattered back
        through packed.indices into zeros -- the same outputs."""
        if output_all_encoded_layers or masked_tokens_mask is not None:
            raise NotImplementedError("BertModel.forward: last layer only, no masked_tokens_mask "
                                      "(the MLM subset path is BertForMaskedLM.mlm_logits)")
        self._check_inputs(input_ids, token_type_ids, attention_mask)
        b, S = input_ids.shape
        if packed is not None:
            x32, xin = self.encode(input_ids, packed=packed)
            seq = torch.zeros(b * S, x32.shape[1], device=x32.device, dtype=x32.dtype)
            seq = seq.index_copy(0, packed.indices, x32).view(b, S, -1)
            pooled = None
            if self.pooler is not None:
                pooled = DF.pooler(xin.index_select(0, packed.cls_rows()),
                                   self.pooler.dense.weight, self.pooler.dense.bias)
            return seq, pooled
        x32, xin = self.encode(input_ids)
        valid = (input_ids != self.config.pad_token_id_mask).unsqueeze(-1)
        seq = x32.view(b, S, -1) * valid
        pooled = None
        if self.pooler is not None:
            pooled = DF.pooler(xin.view(b, S, -1)[:, 0], self.pooler.dense.weight,
                               self.pooler.dense.bias)
        return seq, pooled


class BertPredictionHeadTransform(nn.Module):
    def __init__(self, config):
        super().__init__()
        if config.hidden_act not in ("gelu", "gelu_python"):
            raise NotImplementedError(f"head activation {config.hidden_act!r} (gelu only)")
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=1e-12)


class BertLMPredictionHead(nn.Module):
    def __init__(self, config, bert_model_embedding_weights):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(bert_model_embedding_weights.size(1),
                                 bert_model_embedding_weights.size(0))
        self.decoder.weight = bert_model_embedding_weights


class BertOnlyMLMHead(nn.Module):
    def __init__(self, config, bert_model_embedding_weights):
        super().__init__()
        self.predictions = BertLMPredictionHead(config, bert_model_embedding_weights)


@dataclass
class MLMIndex:
    """Row bookkeeping of one batch, computable on the host before the batch reaches the GPU.

    subset_idx   rows (flattened b*S) entering the last layer's output/MLP: (masked | col 0) & valid
    head_idx     positions inside the subset rows that are masked (labels > 0)   (:626-630)
    target       labels of those rows; flat_masked: their flattened positions
    """
    subset_idx: torch.Tensor
    head_idx: torch.Tensor
    target: torch.Tensor
    flat_masked: torch.Tensor

    @staticmethod
    def build(input_ids, labels, pad_token_id=PAD_TOKEN_ID):
        valid = input_ids != pad_token_id
        masked = labels > 0
        subset = masked.clone()
        subset[:, 0] = True
        subset &= valid
        flat_subset = subset.reshape(-1)
        subset_idx = torch.nonzero(flat_subset).flatten()
        head_idx = torch.nonzero(masked.reshape(-1)[flat_subset]).flatten()
        flat_masked = torch.nonzero(masked.reshape(-1)).flatten()
        target = labels.reshape(-1)[flat_masked]
        return MLMIndex(subset_idx, head_idx, target, flat_masked)

    def to(self, device, non_blocking=False):
        return MLMIndex(*(t.to(device, non_blocking=non_blocking) for t in
                          (self.subset_idx, self.head_idx, self.target, self.flat_masked)))


@dataclass
class PackedIndex:
    """Where the real tokens of a padded batch [b, S] sit, computable on the host while the
    batch is collated (`.to(device, non_blocking=True)` afterwards: the step has no device sync).
    It is what the reference's bert_padding.unpad_input returns, plus the columns ALiBi needs.

    indices      [T] int64  flattened (b, s) positions of the non-pad tokens, row-major
    cu_seqlens   [b+1] int32  cumulative sequence lengths
    positions    [T] int32  the column s of each kept token (ALiBi's |i - j| is taken in padded
                 coordinates: a [PAD] inside a row is not a shift, so the kernel is given the
                 columns instead of recomputing them from cu_seqlens)
    row_of       [b*S] int64  packed row of each flattened position, -1 at pads
    max_seqlen, total (= T), batch, seqlen: ints; first_valid: column 0 of every row is a token;
    sq_sum: sum of the squared lengths (the attention FLOP count of the op timer)
    """
    indices: torch.Tensor
    cu_seqlens: torch.Tensor
    positions: torch.Tensor
    row_of: torch.Tensor
    max_seqlen: int
    total: int
    batch: int
    seqlen: int
    first_valid: bool
    sq_sum: int = 0

    @staticmethod
    def build(input_ids, pad_token_id=PAD_TOKEN_ID):
        if input_ids.dim() != 2:
            raise ValueError(f"PackedIndex.build: input_ids must be [b, S], got "
                             f"{tuple(input_ids.shape)}")
        b, S = input_ids.shape
        valid = input_ids != pad_token_id
        lens = valid.sum(1)
        empty = torch.nonzero(lens == 0).flatten()
        if empty.numel():
            raise ValueError(f"PackedIndex.build: row {int(empty[0])} has no real token (a "
                             "sequence of [PAD] only has no query and no [CLS] row)")
        indices = torch.nonzero(valid.reshape(-1)).flatten()
        total = int(indices.numel())
        cu = torch.zeros(b + 1, dtype=torch.int32, device=input_ids.device)
        cu[1:] = torch.cumsum(lens, 0)
        row_of = torch.full((b * S,), -1, dtype=torch.int64, device=input_ids.device)
        row_of[indices] = torch.arange(total, device=input_ids.device)
        lens_l = lens.tolist()
        return PackedIndex(indices, cu, (indices % S).to(torch.int32), row_of, max(lens_l), total,
                           b, S, bool(valid[:, 0].all()), sum(n * n for n in lens_l))

    def to(self, device, non_blocking=False):
        t = [x.to(device, non_blocking=non_blocking)
             for x in (self.indices, self.cu_seqlens, self.positions, self.row_of)]
        return PackedIndex(*t, self.max_seqlen, self.total, self.batch, self.seqlen,
                           self.first_valid, self.sq_sum)

    def check(self, input_ids):
        if tuple(input_ids.shape) != (self.batch, self.seqlen):
            raise ValueError(f"PackedIndex of a [{self.batch}, {self.seqlen}] batch used with "
                             f"input_ids {tuple(input_ids.shape)}")

    def cls_rows(self):
        """Packed rows of column 0 of every sequence (the [CLS] rows), on the index's device."""
        if not self.first_valid:
            raise ValueError("packed batch: a row starts with [PAD]; the reference reads column 0 "
                             "of every sequence, and a pad there has no packed row")
        return self.row_of[::self.seqlen]


class BertForMaskedLM(nn.Module, _HipEncoder):
    """Registry "dnabert2" model (reference bert_layers.py:691-850)."""

    def __init__(self, config, precision: str = "bf16", **kwargs):
        super().__init__()
        config = BertConfig.from_any(config)
        if config.is_decoder:
            raise ValueError("BertForMaskedLM needs config.is_decoder=False")
        self.config = config
        self.bert = BertModel(config, add_pooling_layer=False, init_weights=False)
        self.cls = BertOnlyMLMHead(config, self.bert.embeddings.word_embeddings.weight)
        self.hyena_framework = config.hyena_framework
        self._init_hip_encoder(precision)
        self._init_weights()
        _tag_projections(self)

    # -- reference-compatible utilities ------------------------------------------------------
    def _init_weights(self):
        _init_bert_weights(self, self.config.initializer_range)

    def get_output_embeddings(self):
        return self.cls.predictions.decoder

    # -- the hot path ------------------------------------------------------------------------
    def mlm_logits(self, input_ids: torch.Tensor, index: MLMIndex,
                   packed: Optional["PackedIndex"] = None) -> torch.Tensor:
        """Compact logits [M, V] of the masked rows (row-major over (b, s)), compute dtype.
        packed: run the encoder on the real tokens only (index.subset_idx holds valid positions
        only, so each has a packed row)."""
        bf16 = self.precision == "bf16"
        _, xin = self.encode(input_ids, index.subset_idx, packed=packed)
        seq = xin.index_select(0, index.head_idx)
        tr = self.cls.predictions.transform
        t = self._linear(seq, tr.dense.weight)
        t32, tb = DF.FusedLayerNorm.apply(t, tr.dense.bias, None, tr.LayerNorm.weight,
                                          tr.LayerNorm.bias, 1e-12, 1, 0.0, 0, 0, not bf16, bf16)
        dec = self.cls.predictions.decoder
        return self._linear(tb if bf16 else t32, dec.weight, dec.bias)

    def mlm_loss(self, input_ids, mask, index: MLMIndex, n_mask: Optional[int] = None,
                 n_unk_masked: Optional[int] = None, packed: Optional["PackedIndex"] = None):
        """Task loss bert_cross_entropy (src/tasks/metrics.py:268-273) without dense logits:
        masked rows with label 0 ([UNK]) have all-zero logits in the reference (no gradient,
        loss ln V each); they are added as a constant."""
        logits = self.mlm_logits(input_ids, index, packed=packed)
        if n_mask is None:
            n_mask = int(mask.sum())
        if n_unk_masked is None:
            n_unk_masked = n_mask - int(index.target.numel())
        loss = DF.MaskedCrossEntropy.apply(logits, index.target, max(n_mask, 1))
        if n_unk_masked:
            loss = loss + n_unk_masked * math.log(self.config.vocab_size) / max(n_mask, 1)
        return loss, logits

    # -- reference forward protocol ----------------------------------------------------------
    def forward(self, batch=None, input_ids=None, attention_mask=None, token_type_ids=None,
                position_ids=None, head_mask=None, inputs_embeds=None, encoder_hidden_states=None,
                encoder_attention_mask=None, labels=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, state=None, mlm_index=None, **kwargs):
        if self.hyena_framework:
            input_ids, labels = batch[0], batch[2]
        if input_ids is None:
            raise ValueError("Must specify input_ids (inputs_embeds is not supported)")
        if token_type_ids is not None and bool((token_type_ids != 0).any()):
            raise NotImplementedError("token_type_ids other than 0 (the MLM path never sets them)")
        if attention_mask is not None and not self.hyena_framework:
            if not torch.equal(attention_mask.bool(), input_ids != self.config.pad_token_id_mask):
                raise NotImplementedError("attention_mask must equal input_ids != [PAD]")
        if labels is None:
            raise NotImplementedError("forward without labels (encoder-only inference)")
        b, S = input_ids.shape
        index = mlm_index if mlm_index is not None else \
            MLMIndex.build(input_ids, labels, self.config.pad_token_id_mask)
        logits = self.mlm_logits(input_ids, index)
        # internal loss over labels > 0 rows (bert_layers.py:818-824)
        loss = DF.MaskedCrossEntropy.apply(logits, index.target, max(index.target.numel(), 1))
        V = logits.shape[-1]
        scores = torch.zeros(b * S, V, device=logits.device, dtype=logits.dtype)
        scores = scores.index_put((index.flat_masked,), logits).view(b, S, V)  # :828-831
        if self.hyena_framework:
            return MaskedLMOutput(loss=loss, logits=(scores, batch[1]), hidden_states=None,
                                  attentions=None), None
        return MaskedLMOutput(loss=loss, logits=scores, hidden_states=None, attentions=None)


class BertForSequenceClassification(nn.Module, _HipEncoder):
    """DNABERT-2 with the sequence classification / regression head (reference
    bert_layers.py:881-1009; every DNABERT-2 experiment config maps
    AutoModelForSequenceClassification to it). Same module tree and state_dict keys: `bert.*`
    with `bert.pooler.dense.*`, `classifier.*`, no `cls.*`.

    Only the [CLS] row reaches the head, so the last layer's output projection, MLP and
    LayerNorms run on the b first-column rows alone; pooler, dropout, classifier and loss are
    the fused head kernels (DF.ClsHead) on the fp32 parameters in both precisions."""

    def __init__(self, config, precision: str = "bf16", **kwargs):
        super().__init__()
        config = BertConfig.from_any(config)
        if config.is_decoder:
            raise ValueError("BertForSequenceClassification needs config.is_decoder=False")
        self.config = config
        self.num_labels = int(config.num_labels)
        self.bert = BertModel(config, add_pooling_layer=True, init_weights=False)
        self.classifier_dropout = (config.classifier_dropout if config.classifier_dropout
                                   is not None else config.hidden_dropout_prob)
        self.dropout = nn.Dropout(self.classifier_dropout)
        self.classifier = nn.Linear(config.hidden_size, self.num_labels)
        self._init_hip_encoder(precision)
        _init_bert_weights(self, config.initializer_range)
        _tag_projections(self, skip=(self.classifier, self.bert.pooler.dense))
        self.last_pred = None  # argmax of the last single-label forward with labels (metrics)

    @classmethod
    def from_composer(cls, pretrained_checkpoint, state_dict=None, cache_dir=None, from_tf=False,
                      config=None, *inputs, **kwargs):
        """Load from a pre-trained checkpoint, non-strictly, with a `model.` prefix stripped
        (reference :903-933)."""
        model = cls(config, *inputs, **kwargs)
        if from_tf:
            raise ValueError("Mosaic BERT does not support loading TensorFlow weights.")
        sd = torch.load(pretrained_checkpoint, map_location="cpu", weights_only=True)
        sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
        missing, unexpected = model.load_state_dict(sd, strict=False)
        model.missing_keys, model.unexpected_keys = list(missing), list(unexpected)
        return model

    def _problem_type(self, labels):
        cfg = self.config
        if cfg.problem_type is None:  # reference :977-984
            if self.num_labels == 1:
                cfg.problem_type = "regression"
            elif self.num_labels > 1 and labels.dtype in (torch.long, torch.int):
                cfg.problem_type = "single_label_classification"
            else:
                cfg.problem_type = "multi_label_classification"
        return cfg.problem_type

    def cls_logits(self, input_ids, labels=None, full_last_layer=False, packed=None):
        """(logits [b, num_labels] fp32, loss | None, pred | None). full_last_layer: run the last
        layer on every row and read the [CLS] rows of its output in place (the reference's
        computation; the default restricts the last layer to those rows). packed (a PackedIndex
        of input_ids): the encoder runs on the real tokens only; ValueError if a row starts with
        [PAD], whose column 0 has no packed row."""
        b, S = input_ids.shape
        rows = torch.arange(b, device=input_ids.device) * S
        if packed is not None:
            cls_rows = packed.cls_rows()  # raises unless every row starts with a real token
            if full_last_layer:
                _, xin = self.encode(input_ids, packed=packed)
                x = xin.index_select(0, cls_rows)
            else:
                _, x = self.encode(input_ids, rows, packed=packed)
        elif full_last_layer:
            _, xin = self.encode(input_ids)
            x = xin.view(b, S, -1)[:, 0]
        else:
            _, x = self.encode(input_ids, rows)
        p = float(self.classifier_dropout) if self.training else 0.0
        pool = self.bert.pooler.dense
        return DF.cls_head(x, pool.weight, pool.bias, self.classifier.weight, self.classifier.bias,
                           p, self.dropout_rng, labels,
                           None if labels is None else self._problem_type(labels))

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None,
                head_mask=None, inputs_embeds=None, labels=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, packed=None):
        self._check_inputs(input_ids, token_type_ids, attention_mask)
        logits, loss, self.last_pred = self.cls_logits(input_ids, labels, packed=packed)
        if return_dict is not None and not return_dict:
            return ((loss, logits) if loss is not None else (logits,))
        return SequenceClassifierOutput(loss=loss, logits=logits, hidden_states=None,
                                        attentions=None)
