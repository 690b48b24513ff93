"""GPU: HyenaDNA (registry model blm) masked-LM pretraining, end to end.

* BertLMHeadModel.mlm_loss on the fused small-vocabulary head (vocab 12 padded to 16) against
  the task loss bert_cross_entropy on the float64 backbone oracle's logits
  (oracle/hyena_lm_ref.py), loss and every parameter gradient; the relative measure and limits
  of tests/test_gpu_hyena_lm.py for this model: `_rel`, forward 1e-4, gradients 2e-3.
* the compact path (vocab 4096) against the dense forward() -> bert_cross_entropy -> autograd.
* FusedAdamW with `_optim` groups against torch.optim.AdamW grouped by the reference's rule.
* BlmTrainer: bf16 steps train; accum = 2 over two half-batches = one step over the batch (fp32).
* train.train(cfg) on a synthetic FASTA / BED: logs, last.ckpt, resume, and the checkpoint
  loading into DNAEmbeddingModel through hyena_lm.load_backbone.
"""
import copy
import io
import json
import math
import os

import pytest
import torch

from oracle import hyena_lm_ref as LM
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _layer(L, lr=None, filter_order=16):
    layer = {"_name_": "hyena", "emb_dim": 5, "filter_order": filter_order, "short_filter_order": 3,
             "l_max": L, "modulate": True, "w": 10, "lr_pos_emb": 0.0, "bidirectional": True,
             "wd": 0.0}
    if lr is not None:
        layer["lr"] = lr
    return layer


def _tiny(L, vocab=12, lr=None, dropout=0.0, perturb=True):
    from dna_amd.hyena_lm import BertLMHeadModel
    m = BertLMHeadModel(d_model=64, n_layer=2, d_inner=256, vocab_size=vocab,
                        pad_vocab_size_multiple=8, embed_dropout=dropout, residual_in_fp32=True,
                        layer=_layer(L, lr))
    if perturb:  # break the reference init's identical-weights symmetry (test_gpu_hyena_lm.py)
        torch.manual_seed(3)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if not n.endswith("freq"):
                    p.add_(torch.randn_like(p) * 0.02)
    return m


def _batch(B, L, vocab, seed=4, per_row=None):
    """(masked_ids, mask, target): ids over the whole vocabulary, about 15 % of the positions
    masked (per_row: exactly that many in every row), 80 % of them replaced by the mask token."""
    g = torch.Generator().manual_seed(seed)
    target = torch.randint(0, vocab, (B, L), generator=g)
    if per_row is None:
        mask = torch.rand(B, L, generator=g) < 0.15
    else:
        mask = torch.zeros(B, L, dtype=torch.bool)
        for b in range(B):
            mask[b, torch.randperm(L, generator=g)[:per_row]] = True
    masked = torch.where(mask & (torch.rand(B, L, generator=g) < 0.8), torch.full_like(target, 3),
                         target)
    return masked, mask, target


def _labels(mask, target):
    return torch.where(mask, target, torch.full_like(target, -100))


def _index(mask, target, V):
    from dna_amd.hyena_lm import BlmIndex
    return BlmIndex.build(mask, target, V).to(DEV)


@pytest.mark.parametrize("L", [256, 130])
def test_mlm_loss_fused_head_vs_oracle(L):
    from dna_amd.tasks import bert_cross_entropy
    m = _tiny(L)
    V = m.lm_head.weight.shape[0]
    assert V == 16
    buffers = {n for n, _ in m.named_buffers()}
    sd = {k: v.detach().double().clone().requires_grad_(k not in buffers)
          for k, v in m.state_dict().items()}
    sd["lm_head.weight"] = sd["backbone.embeddings.word_embeddings.weight"]  # tied
    masked, mask, target = _batch(3, L, 12)
    ref_logits = LM.lm_logits(sd, masked, 64, 2, l_max=L, bidirectional=True)
    ref = bert_cross_entropy((ref_logits.reshape(-1, V), mask), target.reshape(-1))
    ref.backward()
    m = m.to(DEV).eval()
    loss, logits = m.mlm_loss(masked.to(DEV), mask.to(DEV), _index(mask, target, V),
                              int(mask.sum()), 0)
    assert logits is None and type(loss.grad_fn).__name__ == "MaskedLMHeadBackward"
    assert _rel(loss, ref) < 1e-4
    loss.backward()
    for n, p in m.named_parameters():
        r = sd[n].grad
        if n.endswith("freq"):
            pre = n[: n.index("implicit_filter.")]
            r = sum(sd[k].grad for k in sd if k.startswith(pre) and k.endswith("freq"))
        assert _rel(p.grad, r) < 2e-3, n


def test_mlm_loss_compact_path_vs_dense_forward():
    """Vocabulary 4096: index_select of the masked rows -> tied head -> MaskedCrossEntropy,
    against forward()'s dense logits -> bert_cross_entropy -> autograd."""
    from dna_amd.tasks import bert_cross_entropy
    L, V = 128, 4096
    m = _tiny(L, vocab=V).to(DEV).eval()
    masked, mask, target = _batch(3, L, V)
    (out, _) = m((masked.to(DEV), mask.to(DEV)))
    dense = bert_cross_entropy((out.logits[0].reshape(-1, V), mask.to(DEV)),
                               target.reshape(-1).to(DEV))
    dense.backward()
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    loss, logits = m.mlm_loss(masked.to(DEV), mask.to(DEV), _index(mask, target, V),
                              int(mask.sum()), 0)
    assert tuple(logits.shape) == (int(mask.sum()), V)
    assert type(loss.grad_fn).__name__ == "MaskedCrossEntropyBackward"
    assert _rel(loss, dense) < 1e-4
    loss.backward()
    for n, p in m.named_parameters():
        assert _rel(p.grad, want[n]) < 2e-3, n
    # nothing masked: loss 0 and zero gradients (the reference's empty mean is NaN)
    m.zero_grad(set_to_none=True)
    none = torch.zeros_like(mask)
    loss, _ = m.mlm_loss(masked.to(DEV), none.to(DEV), _index(none, target, V), 0, 0)
    loss.backward()
    assert float(loss) == 0.0
    assert all(p.grad is None or not p.grad.any() for p in m.parameters())


def _torch_adamw(params_by_name, model, lr, wd, decay_all=False):
    """torch.optim.AdamW over fp32 copies, grouped by the reference's rule: the parameters
    without `_optim` with the optimizer config, one more group per distinct `_optim` dict."""
    named = list(model.named_parameters())
    normal = [params_by_name[n] for n, p in named if not hasattr(p, "_optim")]
    opt = torch.optim.AdamW(normal, lr=lr, weight_decay=wd)
    hps = sorted(dict.fromkeys(frozenset(p._optim.items()) for _, p in named if hasattr(p, "_optim")))
    for hp in hps:
        ps = [params_by_name[n] for n, p in named if getattr(p, "_optim", None) == dict(hp)]
        g = dict({"params": ps, "lr": lr, "weight_decay": wd}, **dict(hp))
        if decay_all:  # the group's own lr, but decayed like everything else
            g["weight_decay"] = wd
        opt.add_param_group(g)
    return opt


def test_fused_adamw_param_groups_match_torch():
    """Three steps with weight_decay 0.1 and the filter group at wd 0.0 / its own lr, against
    torch.optim.AdamW on fp32 copies with the same gradients. Agreement as
    test_gpu_kernels.py::test_fused_adamw_matches_torch asks of the one-group step: 1e-6 (there
    absolute on parameters below 1; here times max(1, |p|), the Sin frequencies being 10). The
    filter parameters carry no weight-decay term: a decay-all reference is far outside that."""
    from dna_amd.flat import FlatParams
    from dna_amd.optim import FusedAdamW, ParamGroups
    lr, wd, flr = 5e-3, 0.1, 2e-3
    m = _tiny(64, lr=flr).to(DEV)
    names = [n for n, _ in m.named_parameters()]
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    allwd = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    pg = ParamGroups(m)
    assert len(pg) == 2
    flat = FlatParams(m, DEV, shadow_dtype=None, group_of=pg)
    opt = FusedAdamW(flat, lr=lr, weight_decay=wd, max_grad_norm=1.0, groups=pg)
    assert [g["weight_decay"] for g in opt.param_groups] == [wd, 0.0]
    assert [g["lr"] for g in opt.param_groups] == [lr, flr]
    topt, aopt = _torch_adamw(ref, m, lr, wd), _torch_adamw(allwd, m, lr, wd, decay_all=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    params = dict(m.named_parameters())
    for step in range(3):
        flat.zero_grad()
        for n in names:
            g = torch.randn(params[n].shape, device=DEV, generator=gen) * 2
            params[n].grad.copy_(g)
            ref[n].grad, allwd[n].grad = g.clone(), g.clone()
        torch.nn.utils.clip_grad_norm_(list(ref.values()), 1.0)
        torch.nn.utils.clip_grad_norm_(list(allwd.values()), 1.0)
        topt.step()
        aopt.step()
        opt.step()
        for n in names:
            tol = 1e-6 * max(1.0, float(ref[n].detach().abs().max()))
            assert float((params[n].detach() - ref[n].detach()).abs().max()) < tol, (step, n)
    filt = [n for n in names if hasattr(params[n], "_optim") and not n.endswith("freq")]
    assert filt
    for n in filt:  # lr * wd * |p| per step would show
        tol = 1e-6 * max(1.0, float(ref[n].detach().abs().max()))
        assert float((params[n].detach() - allwd[n].detach()).abs().max()) > 10 * tol, n
    # state_dict round trip through torch's layout: both groups come back
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 2
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(pg.members(0)), len(pg.members(1))]
    assert sd["param_groups"][1]["weight_decay"] == 0.0 and sd["param_groups"][1]["lr"] == flr
    tsd = topt.state_dict()
    for i in range(len(names)):  # index for index torch's own state
        torch.testing.assert_close(sd["state"][i]["exp_avg"], tsd["state"][i]["exp_avg"].cpu(),
                                   rtol=1e-5, atol=1e-7)
        assert float(sd["state"][i]["step"]) == 3.0
    topt.load_state_dict(sd)  # torch accepts it
    m2 = _tiny(64, lr=flr).to(DEV)
    pg2 = ParamGroups(m2)
    flat2 = FlatParams(m2, DEV, shadow_dtype=None, group_of=pg2)
    opt2 = FusedAdamW(flat2, lr=1.0, weight_decay=0.5, groups=pg2)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 3
    assert [(g["lr"], g["weight_decay"]) for g in opt2.param_groups] == [(lr, wd), (flr, 0.0)]
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    opt3 = FusedAdamW(flat2, lr=1.0, groups=pg2)
    opt3.load_state_dict(opt.state_dict(torch_layout=False))
    assert [(g["lr"], g["weight_decay"]) for g in opt3.param_groups] == [(lr, wd), (flr, 0.0)]
    assert torch.equal(opt3.exp_avg, opt.exp_avg)


def test_blm_trainer_bf16_trains():
    from dna_amd.trainer import BlmTrainer
    L = 256
    m = _tiny(L, lr=2e-3, dropout=0.1, perturb=False)
    tr = BlmTrainer(m, torch.device(DEV), lr=2e-3, weight_decay=0.1, seed=5,
                    scheduler={"t_initial": 20, "warmup_t": 1, "warmup_lr_init": 1e-4,
                               "lr_min": 6e-5, "t_in_epochs": False})
    assert len(tr.opt.param_groups) == 2 and tr.flat.shadow is not None
    masked, mask, target = _batch(3, L, 12)
    db = tr.device_batch(masked, mask, _labels(mask, target), target)
    assert db.n_mask == int(mask.sum())
    losses = [float(tr.step(db)) for _ in range(4)]
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    assert torch.isfinite(tr.flat.flat).all()
    assert tr.global_step == 4 and tr.sched._last_epoch == 4 and len(tr.micro_losses) == 1
    st = tr.rng_state()
    a = torch.rand(3, device=DEV)
    tr.load_rng_state(st)
    assert torch.equal(a, torch.rand(3, device=DEV))


def test_blm_trainer_accumulation_equals_one_step():
    """fp32, dropout 0: accum = 2 over two half-batches with equally many masked positions is the
    step over the whole batch. The two gradients are the same fp32 sums in another order, so they
    agree to this model's fp32 forward limit (1e-4, max-norm relative); the first AdamW step then
    moves every parameter with a gradient that is not tiny by the same +-lr."""
    from dna_amd.trainer import BlmTrainer
    L, lr = 256, 1e-3
    base = _tiny(L, lr=lr)
    masked, mask, target = _batch(4, L, 12, per_row=38)
    out = []
    for split in (False, True):
        tr = BlmTrainer(copy.deepcopy(base), torch.device(DEV), lr=lr, weight_decay=0.1,
                        autocast=None, seed=1)
        assert tr.flat.shadow is None
        before = tr.flat.flat.clone()
        if split:
            mbs = [tr.device_batch(masked[i:i + 2], mask[i:i + 2],
                                   _labels(mask[i:i + 2], target[i:i + 2]), target[i:i + 2])
                   for i in (0, 2)]
            loss = tr.step(mbs, accum=2)
            assert len(tr.micro_losses) == 2
        else:
            loss = tr.step(tr.device_batch(masked, mask, _labels(mask, target), target))
        out.append((float(loss), tr.flat.grad.clone(), tr.flat.flat - before))
    (la, ga, da), (lb, gb, db) = out
    assert abs(la - lb) <= 1e-4 * abs(la)
    assert _rel(gb, ga) < 1e-4
    big = ga.abs() > 1e-3 * ga.abs().max()
    assert big.any() and float((da - db)[big].abs().max()) < 1e-2 * lr


# ------------------------------------------------------------------------------ train.train(cfg)
@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    """A synthetic hg38: FASTA + .fai + BED with train / valid / test windows of 256 bases."""
    from dna_amd.synthetic import write_hg38
    root = tmp_path_factory.mktemp("blm_hg38")
    write_hg38(str(root), n_chroms=2, chrom_len=60_000, max_length=256)
    return str(root)


TINY = ["experiment=hyena/bert_hg38_hyena", "dataset.max_length=256", "dataset.batch_size=4",
        "dataset.num_workers=0", "model.d_model=64", "model.d_inner=256", "model.n_layer=2",
        "model.layer.filter_order=16", "trainer.devices=1", "trainer.max_epochs=1",
        "trainer.limit_train_batches=4", "trainer.limit_val_batches=2",
        "trainer.log_every_n_steps=1", "scheduler.t_initial=20", "scheduler.warmup_t=2",
        "wandb=null"]


def test_train_blm_runs_checkpoints_resumes_and_feeds_finetuning(data_root, monkeypatch, tmp_path):
    import train
    from dna_amd.compose import compose
    from dna_amd.hyena_lm import DNAEmbeddingModel, load_backbone
    from dna_amd.optim import TimmCosineLRScheduler
    monkeypatch.setenv("DATA_PATH", data_root)
    monkeypatch.chdir(tmp_path)
    cfg = compose(os.path.join(ROOT, "configs"), "config", TINY)
    buf = io.StringIO()
    tr = train.train(cfg, out=buf)
    logs = [json.loads(l) for l in buf.getvalue().splitlines()]
    assert type(tr).__name__ == "BlmTrainer" and isinstance(tr.sched, TimmCosineLRScheduler)
    assert tr.global_step == 4 and len(tr.opt.param_groups) == 2
    tl = [l for l in logs if "train/loss" in l]
    assert [l["step"] for l in tl] == [1, 2, 3, 4]
    assert all(math.isfinite(l["train/loss"]) and math.isfinite(l["train/perplexity"]) for l in tl)
    ev = [l for l in logs if "val/loss" in l]
    assert len(ev) == 1 and ev[0]["step"] == 4
    for k in ("val/loss", "val/perplexity", "test/loss", "test/perplexity"):
        assert math.isfinite(ev[0][k]), k
    assert ev[0]["val/loss"] < math.log(16) + 0.5  # around a uniform guess over 16 entries
    last = tmp_path / "checkpoints" / "last.ckpt"
    assert os.path.exists(last)
    ck = torch.load(last, map_location="cpu", weights_only=True)
    assert ck["global_step"] == 4 and len(ck["optimizer_states"][0]["param_groups"]) == 2
    assert ck["lr_schedulers"][0]["_last_epoch"] == 4
    # resume: step, schedule and both optimizer groups come back (max_epochs reached: no step)
    cfg2 = compose(os.path.join(ROOT, "configs"), "config",
                   TINY + [f"trainer.resume_from_checkpoint={last}"])
    tr2 = train.train(cfg2, out=io.StringIO())
    assert tr2.global_step == 4 and tr2.sched._last_epoch == 4 and tr2.opt.step_count == 4
    assert tr2.sched.get_last_lr() == tr.sched.get_last_lr()
    assert [(g["lr"], g["weight_decay"], g["initial_lr"]) for g in tr2.opt.param_groups] == \
        [(g["lr"], g["weight_decay"], g["initial_lr"]) for g in tr.opt.param_groups]
    assert tr2.opt.param_groups[1]["weight_decay"] == 0.0
    for a, b in zip(tr.model.parameters(), tr2.model.parameters()):
        assert torch.equal(a, b)
    for pa, pb in zip(tr.model.parameters(), tr2.model.parameters()):
        oa, na, _ = tr.flat.slice_of(pa)
        ob, nb, _ = tr2.flat.slice_of(pb)
        assert torch.equal(tr.opt.exp_avg[oa:oa + na], tr2.opt.exp_avg[ob:ob + nb])
        assert torch.equal(tr.opt.exp_avg_sq[oa:oa + na], tr2.opt.exp_avg_sq[ob:ob + nb])
    # and trains on: one more epoch from the checkpoint
    cfg3 = compose(os.path.join(ROOT, "configs"), "config",
                   TINY + [f"trainer.resume_from_checkpoint={last}", "trainer.max_epochs=2"])
    tr3 = train.train(cfg3, out=io.StringIO())
    assert tr3.global_step == 8 and tr3.sched._last_epoch == 8
    # the checkpoint is what finetune.py's load_backbone hook takes
    kw = {k: v for k, v in cfg.model.to_container().items() if k != "_name_"}
    emb = DNAEmbeddingModel(**kw)
    kept = load_backbone(emb, ck["state_dict"])
    assert kept and all("head" in k for k in kept), kept
    ids = torch.randint(7, 11, (2, 256), generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():
        got = emb.to(DEV).eval()(ids)[0]
        want = tr.model.eval().backbone(ids)
    assert torch.equal(got, want)
