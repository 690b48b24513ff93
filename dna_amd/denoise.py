"""The gated dilated-CNN backbone (reference registry model "denoise_cnn":
src/models/sequence/denoise.py CNNModel, src/utils/registry.py:32) on the HIP dilated
convolution (csrc/dilated_conv.hip).

Built: `args.mode == "dilation"` as the reference's fine-tuning experiments use the model --
`pretrain=False, for_representation=True, use_outlinear=False, args.clean_data=False`, with
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

The one numeric deviation: under bf16 autocast the reference carries feat / rc_feat in bf16
(gelu of an autocast conv1d); here the two residual streams stay fp32 and only the convolution
operands (the LayerNorm outputs, z, g) are bf16, as the HyenaDNA block keeps its residual in fp32.
"""
import copy

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
                              "args.clean_data=False is)")


class CNNModel(nn.Module):
    def __init__(self, args, alphabet_size, num_cls, classifier=False, for_representation=False,
                 pretrain=False, dilation=2, kernel_size=9, mlp=True, out_dim=2, length=248,
                 use_outlinear=False, forget=False, num_conv1d=5, d_inner=2, final_conv=False,
                 use_comp=True, **kwargs):
        super().__init__()
        mode = _arg(args, "mode")
        if mode != "dilation":
            _not_built(f"args.mode={mode!r}")
        if pretrain:
            _not_built("pretrain=True")
        if classifier:
            _not_built("classifier=True")
        if _arg(args, "cls_free_guidance", False):
            _not_built("args.cls_free_guidance=True")
        if _arg(args, "clean_data", False):
            _not_built("args.clean_data=True")
        if use_outlinear:
            _not_built("use_outlinear=True")
        if not for_representation:
            _not_built("for_representation=False")
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
        self.classifier, self.for_representation, self.pretrain = False, True, False
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
        self.dropout = nn.Dropout(float(_arg(args, "dropout", 0.0) or 0.0))

    @property
    def d_output(self):
        return self.d_model

    def _complement(self, ids):
        if not self.use_comp:
            return ids
        return torch.where(ids == 4, ids, 3 - ids)  # ACGTN = 01234: A<->T, C<->G, N stays

    def _forward_library(self, ids):
        """The reference's forward on torch's conv1d (DNA_CONV_IMPL=torch: measurement only)."""
        DF.library_fallback("denoise_cnn conv1d", ids.shape, (self.d_model,))
        V = self.alphabet_size
        feat = F.gelu(self.linear(F.one_hot(ids, V).float().transpose(1, 2)))
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

    def forward(self, input_ids, t=None, cls=None, return_embedding=False, state=None):
        if not input_ids.is_cuda:
            raise RuntimeError("denoise_cnn runs on the GPU only (no CPU fallback); got ids on "
                               f"{input_ids.device}")
        ids = input_ids.to(torch.int64)
        if DF.conv_impl() == "torch":
            feat = self._forward_library(ids)
        else:
            feat = DF.onehot_conv(ids, self.linear.weight, self.linear.bias, False)
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
        if self.mlp:
            feat = self.milinear(feat) + feat
        if self.use_final_conv:
            a, act, b = self.final_conv
            feat = native_linear(act(native_linear(feat, a.weight.squeeze(-1), a.bias)),
                                 b.weight.squeeze(-1), b.bias)
        return feat, None
