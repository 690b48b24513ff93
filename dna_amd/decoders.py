"""Sequence-level decoder of the HyenaDNA downstream tasks (reference src/tasks/decoders.py
SequenceDecoder, :36-131, as configs/experiment/hg38/genomic_benchmark_hyena.yaml builds it:
`decoder: {_name_: sequence, mode: pool}` with l_output 0), on the fused pooling head
(functional.PoolHead, csrc/pool_head.hip): restrict over L, output_transform and the loss are
one op, and the [B, L, D] hidden state is read once.

What each supported mode pools (one vector per sequence, l_output = 0):
  pool                 the mean of the whole row (the reference's cumsum / arange at the last
                       position)
  pool + mask          the mean of the first sum(mask) positions (decoders.py:85-105 indexes the
                       running mean at sum(mask) - 1; a row whose mask is empty pools to zero here,
                       where the reference wraps around to the whole-row mean)
  pool + use_lengths   the mean of the first lengths[b] positions
  first / last         position 0 / L - 1 (with use_lengths: lengths[b] - 1)
Not built (NotImplementedError names the option): mode sum and ragged, l_output other than 0,
d_output None (no output_transform).
"""
import torch
import torch.nn as nn

from . import functional as DF

MODES = ("pool", "first", "last")


class SequenceDecoder(nn.Module):
    def __init__(self, d_model, d_output=None, l_output=None, use_lengths=False, mode="last"):
        super().__init__()
        if mode in ("sum", "ragged"):
            raise NotImplementedError(f"SequenceDecoder mode={mode!r} is not built ({MODES} are)")
        if mode not in MODES:
            raise NotImplementedError(f"SequenceDecoder mode={mode!r}: one of {MODES}")
        if d_output is None:
            raise NotImplementedError("SequenceDecoder d_output=None (identity output_transform) "
                                      "is not built: the fused head needs the linear")
        if l_output != 0:
            raise NotImplementedError(f"SequenceDecoder l_output={l_output!r} is not built: "
                                      "l_output=0 (one vector per sequence) only")
        self.output_transform = nn.Linear(d_model, d_output)
        self.d_model, self.d_output = d_model, d_output
        self.l_output, self.squeeze = 1, True
        self.use_lengths = use_lengths
        self.mode = mode

    def window(self, x, mask=None, lengths=None):
        """(start, count) int32 [B] on x's device, None where the kernel's default applies."""
        B, L = x.shape[0], x.shape[1]
        dev = x.device
        n = None
        if self.use_lengths:
            if lengths is None:
                raise ValueError("SequenceDecoder(use_lengths=True) needs lengths")
            n = torch.as_tensor(lengths, device=dev).to(torch.int32).reshape(B)
        elif self.mode == "pool" and mask is not None:
            n = mask.reshape(B, L).to(dev).sum(-1, dtype=torch.int32)
        one = torch.ones(B, device=dev, dtype=torch.int32)
        if self.mode == "pool":
            return None, n
        if self.mode == "first":
            return None, one
        last = torch.full((B,), L - 1, device=dev, dtype=torch.int32) if n is None else n - 1
        return last, one

    def head(self, x, mask=None, lengths=None, labels=None, problem_type=None):
        """-> (logits [B, d_output] fp32, loss | None, pred | None) from hidden states [B, L, D]."""
        start, count = self.window(x, mask, lengths)
        if labels is not None and problem_type is None:
            problem_type = "single_label_classification"
        return DF.pool_head(x, self.output_transform.weight, self.output_transform.bias,
                            start=start, count=count, labels=labels, problem_type=problem_type)

    def forward(self, x, state=None, lengths=None, l_output=None, mask=None):
        return self.head(x, mask=mask, lengths=lengths)[0]


def scale_loss(loss, scale):
    """The head's loss (a mean over B x C) times the task's scale (tasks.pool_loss; customMSE:
    C). Scaled here, so the head's backward receives the scale as its upstream gradient."""
    return loss if loss is None or scale == 1.0 else loss * scale


class SequenceClassifier(nn.Module):
    """An embedding model (forward(input_ids) -> (hidden_states, None), attribute d_output) and a
    SequenceDecoder on it: what the reference's SequenceLightningModule chains for a
    classification task, under its attribute names `model` and `decoder` (the decoder sits in a
    one-entry list there, hence the state-dict keys decoder.0.output_transform.*). problem_type and
    loss_scale: the task's loss as tasks.pool_loss names it; labels are int64 [B] for
    single-label and fp32 [B, d_output] otherwise."""

    def __init__(self, model, d_output, mode="pool", use_lengths=False,
                 problem_type="single_label_classification", loss_scale=1.0):
        super().__init__()
        self.model = model
        self.decoder = nn.ModuleList([SequenceDecoder(model.d_output, d_output, l_output=0,
                                                      use_lengths=use_lengths, mode=mode)])
        self.num_labels = d_output
        self.problem_type = problem_type
        self.loss_scale = float(loss_scale)

    def cls_logits(self, input_ids, labels=None, mask=None, lengths=None):
        hidden, _ = self.model(input_ids)
        logits, loss, pred = self.decoder[0].head(hidden, mask=mask, lengths=lengths,
                                                  labels=labels, problem_type=self.problem_type)
        return logits, scale_loss(loss, self.loss_scale), pred

    def forward(self, input_ids, labels=None, mask=None, lengths=None):
        logits, loss, _ = self.cls_logits(input_ids, labels, mask, lengths)
        return loss, logits
