"""Regression and multi-label heads end to end on the GPU: a SequenceClassifier on a
DNAEmbeddingModel with DeepSEA's 919 labels (the wide pooling head; fp32 and bf16 autocast), a
CaduceusForSequenceClassification with RCPS, two regression targets and customMSE, and
SeqClsTrainer on float targets.

Tolerance, the rule of tests/test_gpu_lm_head.py: no worse than twice the path the head
replaces. That path is the torch composition on the same model -- mean over L -> F.linear ->
the loss, for Caduceus the reference's stack / flip / mean / score per strand / average -- run
with the head in fp32 and in float64 on the backbone's hidden state. With err = max |x - x64|,

    err_fused <= 2 * err_fp32 + floor

for the loss, the logits and every parameter gradient. floor is what storing the compared value
costs: 2^-24 max|x64| (half an fp32 ulp) in fp32; under bf16 autocast the gradient of the hidden
state leaves either head rounded to bf16 (relative 2^-9 per element, and the two heads need not
round the same elements the same way), and every gradient behind it inherits that: 2^-9
max|g64| for the backbone's parameters there, the head's own parameters keep the fp32 floor.

Measured on MI355X (fused error / (2 x fp32 error + floor), worst value per case):
  hyena, 919 labels, fp32           0.44 .. 0.52 (a backbone parameter; two runs)
  hyena, 919 labels, bf16 autocast  0.25 (the head's bias)
  caduceus RCPS, customMSE, fp32    0.81 .. 0.93 (a backbone parameter; two runs)
"""
import pytest
import torch
import torch.nn.functional as F

from test_caduceus import CM
from test_gpu_pool_models import _perturb

pytestmark = pytest.mark.gpu
DEV = "cuda"
MULTI = "multi_label_classification"


def _compare(tag, model, fused, torch_head, bf16, head_params):
    """fused() and torch_head(dtype) -> (loss, logits) on the same model."""
    def run(fn):
        model.zero_grad(set_to_none=True)
        loss, logits = fn()
        loss.backward()
        g = {n: p.grad.detach().double().clone() for n, p in model.named_parameters()
             if p.grad is not None}
        return loss.detach().double().reshape(1), logits.detach().double(), g
    new, old, ref = run(fused), run(lambda: torch_head(torch.float32)), run(
        lambda: torch_head(torch.float64))
    assert set(new[2]) == set(ref[2]) and new[2]
    worst = (0.0, None)
    items = [("loss", new[0], old[0], ref[0], False), ("logits", new[1], old[1], ref[1], False)]
    items += [(n, new[2][n], old[2][n], r, bf16 and n not in head_params) for n, r in ref[2].items()]
    for name, a, b, r, behind_bf16 in items:
        floor = float(r.abs().max()) * (2.0 ** -9 if behind_bf16 else 2.0 ** -24)
        bound = 2 * float((b - r).abs().max()) + floor
        err = float((a - r).abs().max())
        if bound > 0 and err / bound > worst[0]:
            worst = (err / bound, name)
        assert err <= bound, (tag, name, err, bound)
    print(f"{tag}: {len(items)} tensors, worst err / bound {worst[0]:.2f} ({worst[1]})")


def _hyena(L, C, problem, scale=1.0):
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.hyena_lm import DNAEmbeddingModel
    layer = {"_name_": "hyena", "emb_dim": 5, "filter_order": 16, "short_filter_order": 3,
             "l_max": L, "modulate": True, "w": 10, "lr_pos_emb": 0.0}
    emb = DNAEmbeddingModel(d_model=64, n_layer=1, d_inner=256, vocab_size=16, embed_dropout=0.0,
                            resid_dropout=0.0, residual_in_fp32=True, layer=layer)
    m = SequenceClassifier(emb, C, mode="pool", problem_type=problem, loss_scale=scale)
    _perturb(m, 3)
    return m


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_hyena_deepsea_head_vs_torch_composition(precision):
    B, L, C = 3, 130, 919
    m = _hyena(L, C, MULTI).to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 16, (B, L), generator=g).to(DEV)
    labels = (torch.rand(B, C, generator=g) < 0.4).float().to(DEV)
    lin = m.decoder[0].output_transform
    bf16 = precision == "bf16"

    def cast():
        return torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16)

    def fused():
        with cast():
            logits, loss, pred = m.cls_logits(ids, labels)
        assert pred is None and logits.dtype == torch.float32
        return loss, logits

    def torch_head(dtype):
        with cast():
            h, _ = m.model(ids)
        lg = F.linear(h.to(dtype).mean(1), lin.weight.to(dtype), lin.bias.to(dtype))
        return F.binary_cross_entropy_with_logits(lg, labels.to(dtype)), lg

    _compare(f"hyena deepsea {precision}", m, fused, torch_head, bf16,
             ("decoder.0.output_transform.weight", "decoder.0.output_transform.bias"))


def _custom_mse(outs, y):
    """The reference's customMSE (src/tasks/metrics.py:354-356), for any number of columns."""
    y = y.reshape(outs.shape)
    return sum(torch.mean((outs[:, c] - y[:, c]) ** 2) for c in range(outs.shape[1]))


def test_caduceus_rcps_regression_custom_mse():
    from dna_amd.caduceus import CaduceusForSequenceClassification
    from dna_amd.tasks import pool_loss
    B, L, C = 2, 96, 2
    problem, scale = pool_loss("regression", "customMSE", C)
    torch.manual_seed(7)
    m = CaduceusForSequenceClassification(
        pooling_strategy="mean", num_labels=C, problem_type=problem, loss_scale=scale, d_model=64,
        n_layer=2, vocab_size=12, ssm_cfg={"d_state": 16}, fused_add_norm=True, rcps=True,
        complement_map=CM)
    _perturb(m, 9)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(7, 11, (B, L), generator=g).to(DEV)
    y = torch.randn(B, C, generator=g).to(DEV)
    d = m.config["d_model"]

    def fused():
        logits, loss, pred = m.cls_logits(ids, y)
        assert pred is None
        return loss, logits

    def torch_head(dtype):
        out = m.caduceus(ids).to(dtype)
        h = torch.stack([out[..., :d], torch.flip(out[..., d:], dims=[1, 2])], dim=-1)
        p, w = h.mean(dim=1), m.score.weight.to(dtype)
        lg = (F.linear(p[..., 0], w) + F.linear(p[..., 1], w)) / 2
        return _custom_mse(lg, y.to(dtype)), lg

    _compare("caduceus customMSE", m, fused, torch_head, False, ("score.weight",))
    loss, logits = fused()  # customMSE is the reference's formula on the head's own logits
    ref = _custom_mse(logits.detach().double(), y.double())
    assert abs(loss.item() - ref.item()) <= 4 * 2.0 ** -24 * max(1.0, abs(ref.item()))


def test_trainer_learns_float_targets():
    """30 steps on a target a linear head on a mean-pooled state can learn: the GC and the A
    fraction of the sequence."""
    from dna_amd.trainer import SeqClsTrainer
    B, L, C = 16, 64, 2
    m = _hyena(L, C, "regression", scale=float(C))
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(7, 11, (B, L), generator=g)  # A C G T of the character tokenizer
    y = torch.stack([((ids == 8) | (ids == 9)).float().mean(1), (ids == 7).float().mean(1)], 1)
    ids, y = ids.to(DEV), y.to(DEV)
    tr = SeqClsTrainer(m, torch.device(DEV), lr=2e-3, weight_decay=0.0, seed=5, autocast=None)
    losses = [tr.step(ids, y) for _ in range(30)]
    assert tr.last_pred is None and tr.last_logits.shape == (B, C)
    assert all(bool(torch.isfinite(v)) for v in losses)
    assert losses[-1].item() < losses[0].item()
    # evaluate: the loss step() would compute for the same weights (no dropout in this model)
    logits, loss, pred = tr.evaluate(ids, y)
    assert pred is None and tr.model.training
    state = tr.flat.flat.detach().clone()
    again = tr.step(ids, y)
    assert not torch.equal(state, tr.flat.flat)
    assert abs(loss.item() - again.item()) <= 1e-6 * max(1.0, abs(again.item()))
    assert abs(loss.item() - _custom_mse(logits.double(), y.double()).item()) <= 1e-6
