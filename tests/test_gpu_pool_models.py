"""The pooling-head classifiers end to end: DNAEmbeddingModel + SequenceDecoder and
CaduceusForSequenceClassification (rcps off / on, conjoining) on the GPU, fp32, eval mode.

Two checks per case, both isolating the head (the backbones have their own oracle tests):
  1. logits and loss against the float64 head on the hidden state the backbone produced (caught
     with a forward hook), under the kernel tests' rule: at most 4x the larger of CPU fp32 torch's
     error, the fp32 cumsum-form's error and 2^-24 max|ref| (tests/test_gpu_pool_head.py).
  2. every parameter gradient against the same model, same backbone kernels, with the head
     replaced by the torch composition it stands for (Hyena: mean(1) -> F.linear -> cross_entropy;
     Caduceus: the reference's stack / flip / pool / score per strand / average) on the GPU. That
     composition runs twice, with the head in fp32 and in float64 on the same hidden state; the
     difference of the two is what an fp32 head contributes to each gradient. The fused head's
     gradient may differ from the float64-head run by at most 4x that (floored at 2^-24 max|grad|,
     half an fp32 ulp of the stored gradient).

Measured on MI355X: logits 6.2e-9 .. 1.7e-8 and loss 1.2e-8 .. 6.4e-8 against the float64 head,
ratio to the yardstick 0.20 .. 1.12. Gradients, worst parameter per case (fused-vs-float64 over
fp32-vs-float64; both are a few fp32 ulps of the gradient and the backbone's last bits differ
from run to run, so the ratios are coarse and move; over four runs): hyena 1.35 .. 2.86, plain
2.00 .. 2.50, rcps_fused 1.50 .. 1.67, rcps_unfused 1.60 .. 3.81, rcps_first 1.25 .. 1.50,
rcps_last 1.25 .. 1.60, conjoin_eval 1.78 .. 2.50. The floor set the yardstick for 0 .. 1
parameters per case and never decided a verdict.
RC invariance: the two float64 heads agree exactly (the backbone is exactly equivariant at this
size); the fused logits differ by 7.5e-9 (mean) and 0 (first, last).
"""
import pytest
import torch
import torch.nn.functional as F

from test_caduceus import CM
from test_gpu_pool_head import SINGLE, _reference

gpu = pytest.mark.gpu
DEV = "cuda"


def _perturb(m, seed):
    torch.manual_seed(seed)
    with torch.no_grad():  # break the initialisation's symmetries (tied / identical weights)
        for n, p in m.named_parameters():
            if not n.endswith("freq"):
                p.add_(torch.randn_like(p) * 0.02)


def _head_check(tag, logits, loss, x, w, bias, layout, start, count, labels):
    """logits / loss of the fused head against the float64 head on the hidden state x."""
    args = (x.detach().float().cpu(), w.detach().cpu(), None if bias is None else bias.detach().cpu(),
            layout, start, count, labels.cpu(), SINGLE)
    ref = _reference(*args, torch.float64)
    cpu = _reference(*args, torch.float32)
    cum = _reference(*args, torch.float32, form="cumsum")
    got = {"logits": logits, "loss": loss.reshape(1)}
    tol = {}
    for k, g in got.items():
        r = ref[k]
        yard = max(float((cpu[k] - r).abs().max()), float((cum[k] - r).abs().max()),
                   float(r.abs().max()) * 2.0 ** -24)
        err = float((g.detach().double().cpu().reshape(r.shape) - r).abs().max())
        print(f"{tag} {k}: fused {err:.3e} yardstick {yard:.3e} ratio {err / yard:.2f}")
        assert err <= 4 * yard, (tag, k, err, yard)
        tol[k] = 4 * yard
    return ref, tol


def _grad_check(tag, model, fused_loss, torch_head):
    """fused_loss() and torch_head(dtype) -> scalar losses on the same model; compares every
    parameter gradient as the module docstring says."""
    def grads(fn):
        model.zero_grad(set_to_none=True)
        fn().backward()
        return {n: p.grad.detach().double().clone() for n, p in model.named_parameters()
                if p.grad is not None}
    g_fused = grads(fused_loss)
    g32 = grads(lambda: torch_head(torch.float32))
    g64 = grads(lambda: torch_head(torch.float64))
    assert set(g_fused) == set(g64) and g_fused
    worst, floored, needed = (0.0, None), 0, 0
    for n, r in g64.items():
        diff, floor = float((g32[n] - r).abs().max()), float(r.abs().max()) * 2.0 ** -24
        yard = max(diff, floor)
        err = float((g_fused[n] - r).abs().max())
        floored += floor > diff       # the floor, not the two torch runs, sets this yardstick
        needed += err > 4 * diff      # ... and the fused gradient passes only thanks to it
        if yard > 0 and err / yard > worst[0]:
            worst = (err / yard, n)
        assert err <= 4 * yard, (tag, n, err, yard)
    print(f"{tag} gradients: {len(g64)} parameters, worst ratio {worst[0]:.2f} ({worst[1]}); "
          f"floor binds for {floored}, decides for {needed}")


# ------------------------------------------------------------------------------------ HyenaDNA
def _hyena(L=130, d_model=64, C=2, mode="pool"):
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.hyena_lm import DNAEmbeddingModel
    layer = {"_name_": "hyena", "emb_dim": 5, "filter_order": 16, "short_filter_order": 3,
             "l_max": L, "modulate": True, "w": 10, "lr_pos_emb": 0.0}
    emb = DNAEmbeddingModel(d_model=d_model, n_layer=2, d_inner=4 * d_model, vocab_size=16,
                            embed_dropout=0.0, residual_in_fp32=True, layer=layer)
    m = SequenceClassifier(emb, C, mode=mode)
    _perturb(m, 3)
    return m


@gpu
def test_dna_embedding_decoder_vs_float64_head():
    B, L, C = 3, 130, 2
    m = _hyena(L).to(DEV).eval()
    ids = torch.randint(0, 16, (B, L), generator=torch.Generator().manual_seed(4)).to(DEV)
    labels = torch.tensor([1, 0, 1], device=DEV)
    seen = []
    hook = m.model.register_forward_hook(lambda mod, i, o: seen.append(o[0].detach()))
    logits, loss, pred = m.cls_logits(ids, labels)
    hook.remove()
    lin = m.decoder[0].output_transform
    _head_check("hyena", logits, loss, seen[0], lin.weight, lin.bias, "single", None, None, labels)
    assert torch.equal(pred, logits.argmax(-1))

    def torch_head(dtype):
        h, _ = m.model(ids)
        lg = F.linear(h.to(dtype).mean(1), lin.weight.to(dtype), lin.bias.to(dtype))
        return F.cross_entropy(lg, labels)

    _grad_check("hyena", m, lambda: m.cls_logits(ids, labels)[1], torch_head)


def _train_three_steps(m, ids, labels):
    from dna_amd.trainer import SeqClsTrainer
    tr = SeqClsTrainer(m, torch.device(DEV), lr=1e-3, weight_decay=0.0, seed=5,
                       scheduler=dict(t_in_epochs=False, t_initial=100, warmup_t=2,
                                      warmup_lr_init=1e-6, lr_min=0.0))
    before = tr.flat.flat.detach().clone()
    shadow = tr.flat.shadow.detach().clone()
    for _ in range(3):
        loss = tr.step(ids, labels)
        assert bool(torch.isfinite(loss))
    assert tr.global_step == 3 and tr.last_pred.shape == labels.shape
    assert not torch.equal(before, tr.flat.flat) and not torch.equal(shadow, tr.flat.shadow)
    lg, ls, pr = tr.evaluate(ids, labels)
    assert bool(torch.isfinite(ls)) and lg.shape[0] == ids.shape[0] and tr.model.training
    st = tr.rng_state()
    tr.load_rng_state(st)


@gpu
def test_dna_embedding_trains_under_bf16_autocast():
    B, L = 3, 130
    m = _hyena(L)
    ids = torch.randint(0, 16, (B, L), generator=torch.Generator().manual_seed(4)).to(DEV)
    _train_three_steps(m, ids, torch.tensor([1, 0, 1], device=DEV))


@gpu
def test_frozen_backbone_is_bit_identical_after_steps():
    """load_backbone(freeze_backbone=True): the backbone gets no update and no weight decay (the
    fused AdamW stops before it), the decoder trains, and the head's backward writes no dx."""
    from dna_amd.hyena_lm import load_backbone
    from dna_amd.trainer import SeqClsTrainer
    B, L = 3, 130
    m = _hyena(L)
    load_backbone(m.model, {k: v.clone() for k, v in m.model.state_dict().items()},
                  freeze_backbone=True)
    assert not any(p.requires_grad for p in m.model.parameters())
    tr = SeqClsTrainer(m, torch.device(DEV), lr=1e-2, weight_decay=0.1, seed=5)
    assert 0 < tr.opt.numel < tr.flat.numel
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    shadow = tr.flat.shadow.detach().clone()
    ids = torch.randint(0, 16, (B, L), generator=torch.Generator().manual_seed(4)).to(DEV)
    labels = torch.tensor([1, 0, 1], device=DEV)
    for _ in range(3):
        assert bool(torch.isfinite(tr.step(ids, labels)))
    for n, p in m.named_parameters():
        if n.startswith("model."):
            assert torch.equal(p, before[n]), n
        else:
            assert not torch.equal(p, before[n]), n
    assert torch.equal(tr.flat.shadow[tr.opt.numel:], shadow[tr.opt.numel:])
    assert not torch.equal(tr.flat.shadow[:tr.opt.numel], shadow[:tr.opt.numel])
    # frozen parameters in the middle of trainable ones are refused, not decayed
    m2 = _hyena(L)
    m2.decoder[0].output_transform.bias.requires_grad = False
    with pytest.raises(NotImplementedError, match="frozen"):
        SeqClsTrainer(m2, torch.device(DEV))


@gpu
def test_head_backward_without_dx():
    """x without a gradient: dW / dbias as with one, and no dx is made."""
    from dna_amd import functional as DF
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 300, 64, generator=g).to(DEV)
    labels = torch.tensor([1, 0], device=DEV)
    grads = []
    for need in (True, False):
        w = torch.randn(2, 64, generator=torch.Generator().manual_seed(3)) * 0.1
        w = w.to(DEV).requires_grad_(True)
        b = torch.zeros(2, device=DEV, requires_grad=True)
        xi = x.clone().requires_grad_(need)
        DF.pool_head(xi, w, b, labels=labels, problem_type=SINGLE)[1].backward()
        assert (xi.grad is not None) == need
        grads.append((w.grad, b.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


# ------------------------------------------------------------------------------------ Caduceus
def _caduceus(rcps=False, fused_add_norm=True, C=3, pooling="mean", **kw):
    from dna_amd.caduceus import CaduceusForSequenceClassification
    torch.manual_seed(7)
    cfg = dict(d_model=64, n_layer=2, vocab_size=12, ssm_cfg={"d_state": 16},
               fused_add_norm=fused_add_norm)
    if rcps:
        cfg.update(rcps=True, complement_map=CM)
    m = CaduceusForSequenceClassification(pooling_strategy=pooling, num_labels=C, **kw, **cfg)
    _perturb(m, 9)
    return m


def _reference_pool(h, pooling):
    if pooling == "mean":
        return h.mean(dim=1)
    return h[:, 0] if pooling == "first" else h[:, -1]


def _caduceus_torch_head(m, ids, labels, dtype, conjoin):
    """The reference's forward after the backbone (modeling_caduceus.py:543-610), in `dtype`."""
    d, w = m.config["d_model"], m.score.weight.to(dtype)
    if m.config["rcps"]:
        out = m.caduceus(ids).to(dtype)
        h = torch.stack([out[..., :d], torch.flip(out[..., d:], dims=[1, 2])], dim=-1)
    elif conjoin:
        h = torch.stack([m.caduceus(ids[..., 0]).to(dtype), m.caduceus(ids[..., 1]).to(dtype)],
                        dim=-1)
    else:
        h = m.caduceus(ids).to(dtype)
    p = _reference_pool(h, m.pooling_strategy)
    if h.dim() == 4:
        lg = (F.linear(p[..., 0], w) + F.linear(p[..., 1], w)) / 2
    else:
        lg = F.linear(p, w)
    return F.cross_entropy(lg, labels)


CADUCEUS_CASES = {
    "plain": dict(rcps=False),
    "rcps_fused": dict(rcps=True, fused_add_norm=True),
    "rcps_unfused": dict(rcps=True, fused_add_norm=False),
    "rcps_first": dict(rcps=True, pooling="first"),
    "rcps_last": dict(rcps=True, pooling="last"),
    "conjoin_eval": dict(rcps=False, conjoin_eval=True),
}


def _rc_ids(ids):
    cm = torch.tensor([CM[i] for i in range(12)], device=ids.device)
    return cm[ids].flip(-1)


@gpu
@pytest.mark.parametrize("case", list(CADUCEUS_CASES))
def test_caduceus_classifier_vs_float64_head(case):
    B, L, C = 2, 96, 3
    kw = CADUCEUS_CASES[case]
    m = _caduceus(C=C, **kw).to(DEV).eval()
    conjoin = bool(kw.get("conjoin_eval"))
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(3)).to(DEV)
    if conjoin:
        ids = torch.stack([ids, _rc_ids(ids)], dim=-1)
    labels = torch.tensor([2, 0], device=DEV)
    seen = []
    hook = m.caduceus.register_forward_hook(lambda mod, i, o: seen.append(o.detach()))
    logits, loss, pred = m.cls_logits(ids, labels)
    hook.remove()
    pooling = m.pooling_strategy
    start = {"mean": None, "first": None, "last": [L - 1] * B}[pooling]
    count = None if pooling == "mean" else [1] * B
    if kw["rcps"]:
        x, layout = seen[0], "rcps_mirror"
    elif conjoin:
        x, layout = torch.cat(seen, dim=-1), "two"
    else:
        x, layout = seen[0], "single"
    assert len(seen) == (2 if conjoin else 1)
    _head_check(case, logits, loss, x, m.score.weight, None, layout, start, count, labels)
    assert torch.equal(pred, logits.argmax(-1))
    _grad_check(case, m, lambda: m.cls_logits(ids, labels)[1],
                lambda dtype: _caduceus_torch_head(m, ids, labels, dtype, conjoin))


@gpu
@pytest.mark.parametrize("pooling", ["mean", "first", "last"])
def test_caduceus_rcps_logits_are_rc_invariant(pooling):
    """Logits on a sequence and on its reverse complement: the float64 head on the two hidden
    states shows the backbone's own gap; the fused head may add its tolerance on each side."""
    B, L, C = 2, 96, 3
    m = _caduceus(rcps=True, C=C, pooling=pooling).to(DEV).eval()
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(3)).to(DEV)
    labels = torch.tensor([2, 0], device=DEV)
    start = {"mean": None, "first": None, "last": [L - 1] * B}[pooling]
    count = None if pooling == "mean" else [1] * B
    out = []
    for x in (ids, _rc_ids(ids)):
        seen = []
        hook = m.caduceus.register_forward_hook(lambda mod, i, o: seen.append(o.detach()))
        logits, loss, _ = m.cls_logits(x, labels)
        hook.remove()
        ref, tol = _head_check(f"rc {pooling}", logits, loss, seen[0], m.score.weight, None,
                               "rcps_mirror", start, count, labels)
        out.append((logits.detach().double().cpu(), ref["logits"], tol["logits"]))
    (l1, r1, t1), (l2, r2, t2) = out
    backbone_gap = float((r1 - r2).abs().max())
    fused_gap = float((l1 - l2).abs().max())
    print(f"rc {pooling}: fused gap {fused_gap:.3e} backbone gap {backbone_gap:.3e}")
    assert fused_gap <= backbone_gap + t1 + t2


@gpu
def test_caduceus_classifier_trains_under_bf16_autocast():
    B, L = 2, 96
    m = _caduceus(rcps=True, C=3)
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(3)).to(DEV)
    _train_three_steps(m, ids, torch.tensor([2, 0], device=DEV))


# ---------------------------------------------------------------------------------- state dicts
def test_lm_checkpoint_loads_into_dna_embedding_model():
    from dna_amd.hyena_lm import BertLMHeadModel, DNAEmbeddingModel, load_backbone
    layer = {"_name_": "hyena", "emb_dim": 5, "filter_order": 16, "short_filter_order": 3,
             "l_max": 66, "modulate": True, "w": 10, "lr_pos_emb": 0.0}
    kw = dict(d_model=32, n_layer=1, d_inner=64, vocab_size=12, pad_vocab_size_multiple=8,
              layer=layer)
    lm = BertLMHeadModel(**kw)
    _perturb(lm, 1)
    emb = DNAEmbeddingModel(**kw)
    assert set(emb.state_dict()) == set(lm.state_dict())
    emb.load_state_dict(lm.state_dict())  # the plain load
    sd = {"model." + k: v.clone() for k, v in lm.state_dict().items()}
    emb2 = DNAEmbeddingModel(**kw)
    kept = load_backbone(emb2, sd, freeze_backbone=True)
    assert kept == ["lm_head.weight"]
    for (n, a), (_, b) in zip(sorted(emb2.state_dict().items()), sorted(lm.state_dict().items())):
        assert torch.equal(a, b), n
    assert emb2.lm_head.weight is emb2.backbone.embeddings.word_embeddings.weight
    assert not any(p.requires_grad for p in emb2.parameters())
    assert emb2.d_output == 32
    with pytest.raises(KeyError, match="missing"):
        load_backbone(DNAEmbeddingModel(**kw), {"model.lm_head.weight": sd["model.lm_head.weight"]})


def test_masked_lm_backbone_loads_into_caduceus_classifier():
    from dna_amd.caduceus import CaduceusForMaskedLM, CaduceusForSequenceClassification
    cfg = dict(d_model=32, n_layer=1, vocab_size=12, ssm_cfg={"d_state": 8}, rcps=True,
               complement_map=CM)
    lm = CaduceusForMaskedLM(**cfg)
    clf = CaduceusForSequenceClassification(num_labels=4, **cfg)
    backbone = {k: v for k, v in lm.state_dict().items() if k.startswith("caduceus.")}
    missing, unexpected = clf.load_state_dict(backbone, strict=False)
    assert list(missing) == ["score.weight"] and not unexpected
    assert clf.score.weight.shape == (4, 32) and clf.score.bias is None
