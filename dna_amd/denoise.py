"""The gated dilated-CNN backbone (reference registry model "denoise_cnn":
src/models/sequence/denoise.py CNNModel, src/utils/registry.py:32) on the HIP dilated
convolution (csrc/dilated_conv.hip).

Built: `args.mode == "dilation"` as the reference's fine-tuning experiments use the model --
`pretrain=False, for_representation=True, use_outlinear=False, args.clean_data=False` -- and as
its masked-LM pretraining (configs/experiment/hg38/hg38_bert.yaml) does -- `pretrain=True,
for_representation=False`, which adds `out_linear` (see "Pretraining" below); both with
forget / use_comp / mlp / final_conv either way, num_cnn_stacks >= 1, num_conv1d 1..5, odd
kernel_size <= 9, any dilation >= 1, hidden_dim a multiple of 64 up to 512. The constructor keys,
the module tree and the state-dict keys are the reference's (`linear`, `rc_linear`, `convs.i`,
`gates.i`, `norms.i`, `rc_norms.i`, `milinear.{0,2,3,4,6,7}`, `final_conv.{0,2}`), so one of its
checkpoints of this configuration loads with strict=True. Every other mode and option raises
NotImplementedError naming it.

    forward(input_ids [B, L], ids 0..4 = A C G T N) -> (feat [B, L, D], None)

What runs where: the two input layers Conv1d(5, D, 9) on a one-hot input are table lookups
(functional.onehot_conv; rc_linear on the complemented ids when use_comp); each of the
num_conv1d * num_cnn_stacks layers is two LayerNorms (hyena_lm.LayerNorm) and one
functional.GatedDilatedConv node (gate conv + main conv with the combine in their epilogues);
milinear and final_conv (k = 1: a per-position linear) run on HipLinear's kernels. The nn.Conv1d
modules only hold the parameters, except under DNA_CONV_IMPL=torch (a measurement switch that
counts as a library fallback), where they run.

Pretraining (`pretrain=True, for_representation=False`): the reference's `self.pretrain` branch
of forward (denoise.py:546-677). The main stream's input layer runs under ReLU (rc_linear stays
GELU), the layers are the same, and out_linear = Linear(D, alphabet_size) with a bias follows.

    forward((input_ids, mask)) -> (CausalLMOutput(logits=(logits [B, L, V], mask)), None)
    mlm_loss(input_ids, mask, index: hyena_lm.BlmIndex) -> (loss, None)

mlm_loss is the task loss bert_cross_entropy (src/tasks/metrics.py:268-273) without a logits
tensor. Everything after the last gated layer is per position, so that tail -- milinear + the
residual, final_conv, out_linear -- runs on the M masked rows only (index_select with
index.flat_masked, as hyena_lm's BPE branch compacts them) and ends in the biased fused head
(functional.masked_lm_head(bias=), csrc/lm_head.hip) on [M, D] with index.target. M is any
number, so the tail's linears go through functional.strided_linear, whose kernels take any row
count. DNA_DENOISE_MLM_TAIL=dense runs the tail on all B * L rows and the fused head on [T, D]
with index.labels instead (the A/B of DESIGN §5.5). M == 0 gives loss 0 and zero gradients (the
reference's mean over an empty selection is NaN).

The one numeric deviation: under bf16 autocast the reference carries feat / rc_feat in bf16
(gelu of an autocast conv1d); here the two residual streams stay fp32 and only the convolution
operands (the LayerNorm outputs, z, g) are bf16, as the HyenaDNA block keeps its residual in fp32.
"""
import copy
import os
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as DF
from .hyena import HipLinear, hip_linear
from .hyena_lm import LayerNorm  # widths in hyena_lm._LN_COLS on HIP, others on torch's kernel


def native_linear(x, weight, bias):
    """hip_linear, kept on hand-written kernels for every shape of this model: the persistent
    GEMM's weight gradient takes sides that are multiples of 256 only and hands anything else
    (128 -> 256 at hidden_dim 128) to a library GEMM, so such a layer runs wholly on the strided
    MFMA GEMM instead, forward, data gradient and weight gradient."""
    if weight.shape[0] % 256 or weight.shape[1] % 256:
        return DF.strided_linear(x, weight, bias)
    return hip_linear(x, weight, bias)


class MlpLinear(HipLinear):
    """The Linear layers of milinear: HipLinear (same parameters / state dict) on native_linear."""

    def forward(self, x):
        return native_linear(x, self.weight, self.bias)


def _arg(args, name, default=None):
    if isinstance(args, dict):
        return args.get(name, default)
    return getattr(args, name, default)


def _not_built(what):
    raise NotImplementedError(f"denoise_cnn: {what} is not built (mode 'dilation' with "
                              "pretrain=False, for_representation=True, use_outlinear=False, "
                              "args.clean_data=False is, and the same with pretrain=True, "
                              "for_representation=False)")


CausalLMOutput = namedtuple("CausalLMOutput", ["logits"])


def mlm_tail():
    """DNA_DENOISE_MLM_TAIL: "compact" (default: the per-position tail of mlm_loss on the masked
    rows only) | "dense" (on every row; kept for the A/B measurement)."""
    v = os.environ.get("DNA_DENOISE_MLM_TAIL", "compact")
    if v not in ("compact", "dense"):
        raise ValueError(f"DNA_DENOISE_MLM_TAIL={v!r}: compact or dense")
    return v


def _rows_linear(x, weight, bias):
    """A Linear on [M, D] rows for any M: the strided MFMA GEMM (forward, data and weight
    gradient), which pads nothing onto a library for an odd row count."""
    return DF.strided_linear(x, weight, bias)


class CNNModel(nn.Module):
    def __init__(self, args, alphabet_size, num_cls, classifier=False, for_representation=False,
                 pretrain=False, dilation=2, kernel_size=9, mlp=True, out_dim=2, length=248,
                 use_outlinear=False, forget=False, num_conv1d=5, d_inner=2, final_conv=False,
                 use_comp=True, **kwargs):
        super().__init__()
        mode = _arg(args, "mode")
        if mode != "dilation":
            _not_built(f"args.mode={mode!r}")
        if pretrain and for_representation:
            _not_built("pretrain=True with for_representation=True")
        if classifier:
            _not_built("classifier=True")
        if _arg(args, "cls_free_guidance", False):
            _not_built("args.cls_free_guidance=True")
        if _arg(args, "clean_data", False):
            _not_built("args.clean_data=True")
        if use_outlinear:
            _not_built("use_outlinear=True")
        if not for_representation and not pretrain:
            _not_built("for_representation=False without pretrain=True")
        D = int(_arg(args, "hidden_dim"))
        stacks = int(_arg(args, "num_cnn_stacks", 1))
        if D % 64 or not 64 <= D <= 512:
            _not_built(f"args.hidden_dim={D} (a multiple of 64 up to 512)")
        if not 1 <= int(num_conv1d) <= 5:
            _not_built(f"num_conv1d={num_conv1d} (1..5)")
        if kernel_size % 2 == 0 or not 1 <= kernel_size <= 9:
            _not_built(f"kernel_size={kernel_size} (odd, <= 9)")
        if int(dilation) < 1 or stacks < 1:
            _not_built(f"dilation={dilation} / args.num_cnn_stacks={stacks} (both >= 1)")
        if int(alphabet_size) > 8:
            _not_built(f"alphabet_size={alphabet_size} (<= 8)")
        self.alphabet_size, self.args, self.num_cls = int(alphabet_size), args, num_cls
        self.classifier, self.pretrain = False, bool(pretrain)
        self.for_representation = not self.pretrain
        self.d_model = D
        self.mlp, self.use_outlinear, self.forget = bool(mlp), False, bool(forget)
        self.num_conv1d, self.d_inner = int(num_conv1d), int(d_inner)
        self.use_final_conv, self.use_comp = bool(final_conv), bool(use_comp)
        self.num_cnn_stacks = stacks
        self.num_layers = self.num_conv1d * stacks
        self.mode = mode

        k, pad = int(kernel_size), (int(kernel_size) - 1) // 2
        self.linear = nn.Conv1d(self.alphabet_size, D, kernel_size=9, padding=4)
        self.rc_linear = nn.Conv1d(self.alphabet_size, D, kernel_size=9, padding=4)
        dils = [1, 1, int(dilation), int(dilation) ** 2, int(dilation) ** 3][:self.num_conv1d]

        def tower():
            base = [nn.Conv1d(D, D, kernel_size=k, dilation=d, padding=pad * d) for d in dils]
            return nn.ModuleList([copy.deepcopy(layer) for layer in base for _ in range(stacks)])

        self.convs = tower()
        self.gates = tower()
        if self.mlp:
            Di = D * self.d_inner
            self.milinear = nn.Sequential(MlpLinear(D, Di), nn.GELU(), MlpLinear(Di, Di),
                                          LayerNorm(Di), MlpLinear(Di, Di), nn.GELU(),
                                          MlpLinear(Di, D), LayerNorm(D))
        self.norms = nn.ModuleList([LayerNorm(D) for _ in range(self.num_layers)])
        self.rc_norms = nn.ModuleList([LayerNorm(D) for _ in range(self.num_layers)])
        if self.use_final_conv:
            self.final_conv = nn.Sequential(nn.Conv1d(D, D, kernel_size=1), nn.GELU(),
                                            nn.Conv1d(D, D, kernel_size=1))
        if self.pretrain:
            self.out_linear = nn.Linear(D, self.alphabet_size)
        self.dropout = nn.Dropout(float(_arg(args, "dropout", 0.0) or 0.0))

    @property
    def d_output(self):
        return self.d_model

    def _complement(self, ids):
        if not self.use_comp:
            return ids
        return torch.where(ids == 4, ids, 3 - ids)  # ACGTN = 01234: A<->T, C<->G, N stays

    @property
    def lm_head(self):
        """The vocabulary projection, under the name BlmTrainer reads (`lm_head.weight.shape[0]`
        bounds the labels). A property: no state-dict key."""
        if not self.pretrain:
            raise AttributeError("denoise_cnn: lm_head exists with pretrain=True only")
        return self.out_linear

    def _forward_library(self, ids):
        """The reference's forward on torch's conv1d (DNA_CONV_IMPL=torch: measurement only)."""
        DF.library_fallback("denoise_cnn conv1d", ids.shape, (self.d_model,))
        V = self.alphabet_size
        act = F.relu if self.pretrain else F.gelu
        feat = act(self.linear(F.one_hot(ids, V).float().transpose(1, 2)))
        rc_feat = F.gelu(self.rc_linear(F.one_hot(self._complement(ids), V).float().transpose(1, 2)))
        for i in range(self.num_layers):
            h = self.norms[i](self.dropout(feat).transpose(1, 2)).transpose(1, 2)
            rc_h = self.rc_norms[i](self.dropout(rc_feat).transpose(1, 2)).transpose(1, 2)
            z_g = self.gates[i](rc_h)
            g = torch.sigmoid(z_g) if self.forget else F.gelu(z_g)
            h = F.gelu(self.convs[i](h))
            feat = h * g + feat if self.forget else h + g + feat
            rc_feat = g + rc_feat
        return feat.transpose(1, 2)

    def _layers(self, input_ids):
        """The two input layers and the gated layers -> feat [B, L, D] fp32."""
        if not input_ids.is_cuda:
            raise RuntimeError("denoise_cnn runs on the GPU only (no CPU fallback); got ids on "
                               f"{input_ids.device}")
        ids = input_ids.to(torch.int64)
        if DF.conv_impl() == "torch":
            feat = self._forward_library(ids)
        else:
            feat = DF.onehot_conv(ids, self.linear.weight, self.linear.bias, False,
                                  act=DF.N.ACT_RELU if self.pretrain else DF.N.ACT_GELU)
            rc_feat = DF.onehot_conv(ids, self.rc_linear.weight, self.rc_linear.bias,
                                     self.use_comp)
            for i in range(self.num_layers):
                h = self.norms[i](self.dropout(feat))
                rc_h = self.rc_norms[i](self.dropout(rc_feat))
                conv, gate = self.convs[i], self.gates[i]
                with torch.autocast("cuda", enabled=False):
                    feat, rc_feat = DF.GatedDilatedConv.apply(
                        h, rc_h, feat, rc_feat, conv.weight, conv.bias, gate.weight, gate.bias,
                        conv.dilation[0], self.forget)
        return feat

    def _tail(self, feat, linear=native_linear):
        """milinear + the residual, then final_conv (k = 1: two per-position linears), on
        [..., D]. linear: native_linear, or _rows_linear for a compacted [M, D] of any M."""
        if self.mlp:
            h = feat
            for layer in self.milinear:
                h = linear(h, layer.weight, layer.bias) if isinstance(layer, MlpLinear) else layer(h)
            feat = h + feat
        if self.use_final_conv:
            a, act, b = self.final_conv
            feat = linear(act(linear(feat, a.weight.squeeze(-1), a.bias)),
                          b.weight.squeeze(-1), b.bias)
        return feat

    def forward(self, input_ids, t=None, cls=None, return_embedding=False, state=None):
        if not self.pretrain:
            return self._tail(self._layers(input_ids)), None
        if not isinstance(input_ids, (tuple, list)) or len(input_ids) != 2:
            raise TypeError("denoise_cnn with pretrain=True takes the tuple (input_ids, mask), as "
                            "the reference's pretraining forward does; got "
                            f"{type(input_ids).__name__}")
        ids, mask = input_ids
        feat = self._tail(self._layers(ids))
        w, b = self.out_linear.weight, self.out_linear.bias
        B, L, D = feat.shape
        # dense logits serve parity and inference only; alphabet_size columns fit no tile of the
        # persistent GEMM, so the strided one
        logits = _rows_linear(feat.reshape(B * L, D), w, b).reshape(B, L, -1)
        return CausalLMOutput(logits=(logits, mask)), None

    def mlm_loss(self, input_ids, mask, index, n_mask=None, n_unk_masked=None):
        """bert_cross_entropy over the masked positions without a logits tensor;
        BertLMHeadModel.mlm_loss's signature with a hyena_lm.BlmIndex -> (loss, None). mask,
        n_mask and n_unk_masked are unused: the index carries the rows and every one is scored."""
        if not self.pretrain:
            raise RuntimeError("denoise_cnn: mlm_loss needs pretrain=True")
        feat = self._layers(input_ids)
        w, b = self.out_linear.weight, self.out_linear.bias
        D = feat.shape[-1]
        # no masked row: the dense tail, where the head's count == 0 contract gives loss 0 and
        # writes a zero gradient to every parameter (a compacted [0, D] has no kernel to run)
        if mlm_tail() == "dense" or int(index.flat_masked.numel()) == 0:
            loss, _ = DF.masked_lm_head(self._tail(feat), w, index.labels, bias=b)
            return loss, None
        rows = feat.reshape(-1, D).index_select(0, index.flat_masked)
        loss, _ = DF.masked_lm_head(self._tail(rows, _rows_linear), w, index.target, bias=b)
        return loss, None
