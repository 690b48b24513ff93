"""GPU: Caduceus (registry model caduceus) masked-LM pretraining, end to end.

* CaduceusForMaskedLM.mlm_loss on the fused small-vocabulary head (vocab 12 padded to 16), plain
  for rcps=False and RC-equivariant for rcps=True, against the float64 oracle's logits
  (oracle/caduceus_ref.mlm_logits) + float64 cross entropy over the masked positions: the loss and
  every parameter gradient; the relative measure and limits of tests/test_gpu_caduceus.py for this
  model: `_rel`, forward 1e-4, gradients 2e-3.
* the compact path (vocab 4096) against the dense forward(input_ids, labels).
* a batch without a masked position: loss 0, zero gradients.
* add_optimizer_hooks + FusedAdamW(groups=) against torch.optim.AdamW grouped by the same rule.
* BlmTrainer: bf16 steps train; accum = 2 over two half-batches = one step over the batch (fp32).
* train.train(cfg) on a synthetic FASTA / BED with the new experiment: logs, last.ckpt, resume,
  and the checkpoint loading into CaduceusForSequenceClassification through
  finetune.load_pretrained.
* two ranks (one device each) = one process on the concatenated batch.
"""
import copy
import io
import json
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from oracle import caduceus_ref as CR
from test_caduceus import CM, _rcps_sd
from test_gpu_blm_pretrain import _batch, _index, _labels, _torch_adamw
from test_gpu_caduceus import _rel
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, L = 2, 300


def _tiny(rcps, vocab=12, perturb=True, seed=7, **kw):
    from dna_amd.caduceus import CaduceusForMaskedLM
    torch.manual_seed(seed)
    if rcps:
        kw.update(rcps=True, complement_map=CM)
    m = CaduceusForMaskedLM(d_model=64, n_layer=2, vocab_size=vocab, ssm_cfg={"d_state": 16}, **kw)
    if perturb:  # as tests/test_gpu_caduceus.py: break the init's symmetry
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * 0.02)
    return m


def _oracle_sd(m, rcps):
    if rcps:
        return _rcps_sd(m)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    sd["lm_head.weight"] = sd["caduceus.backbone.embeddings.word_embeddings.weight"]  # tied
    for i in range(m.config["n_layer"]):
        p = f"caduceus.backbone.layers.{i}.mixer."
        for k in ("in_proj.weight", "out_proj.weight"):
            sd[p + "mamba_rev." + k] = sd[p + "mamba_fwd." + k]
    return sd


def _dt_rank(m, rcps):
    mixer = m.caduceus.backbone.layers[0].mixer
    return (mixer.submodule if rcps else mixer).mamba_fwd.dt_rank


@pytest.mark.parametrize("rcps", [False, True], ids=["ph", "rcps"])
def test_mlm_loss_fused_head_vs_oracle(rcps):
    m = _tiny(rcps)
    V = m.lm_head.weight.shape[0]
    assert V == 16
    sd = _oracle_sd(m, rcps)
    masked, mask, target = _batch(B, L, 12)
    ref_logits = CR.mlm_logits(sd, masked, 2, 16, 4, _dt_rank(m, rcps), rcps=rcps)
    keep = mask.reshape(-1)
    ref = F.cross_entropy(ref_logits.reshape(-1, V)[keep], target.reshape(-1)[keep])
    ref.backward()
    m = m.to(DEV)
    loss, logits = m.mlm_loss(masked.to(DEV), mask.to(DEV), _index(mask, target, V),
                              int(mask.sum()), 0)
    assert logits is None and type(loss.grad_fn).__name__ == "MaskedLMHeadBackward"
    print(f"caduceus mlm_loss rcps={rcps}: loss {float(loss.detach()):.6f} ref {float(ref.detach()):.6f} "
          f"rel {_rel(loss, ref):.3e}")
    assert _rel(loss, ref) < 1e-4
    loss.backward()
    for n, p in m.named_parameters():
        assert _rel(p.grad, sd[n].grad) < 2e-3, n


def test_mlm_loss_untied_head_reads_its_own_weight():
    m = _tiny(False, tie_word_embeddings=False).to(DEV)
    emb = m.caduceus.backbone.embeddings.word_embeddings
    assert m.lm_head.weight is not emb.weight
    masked, mask, target = _batch(B, L, 12)
    labels = _labels(mask, target).to(DEV)
    dense, _ = m(masked.to(DEV), labels)
    dense.backward()
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    loss, logits = m.mlm_loss(masked.to(DEV), mask.to(DEV), _index(mask, target, 16))
    assert logits is None and _rel(loss, dense) < 1e-4
    loss.backward()
    assert "lm_head.weight" in want
    for n, p in m.named_parameters():
        assert _rel(p.grad, want[n]) < 2e-3, n


def test_mlm_loss_compact_path_vs_dense_forward():
    """Vocabulary 4096: index_select of the masked rows -> the head -> MaskedCrossEntropy, against
    forward(input_ids, labels): dense logits -> F.cross_entropy(ignore_index) -> autograd."""
    V = 4096
    m = _tiny(False, vocab=V).to(DEV)
    masked, mask, target = _batch(B, L, V)
    dense, dlogits = m(masked.to(DEV), _labels(mask, target).to(DEV))
    assert tuple(dlogits.shape) == (B, L, V)
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
    # nothing masked: loss 0 and zero gradients
    m.zero_grad(set_to_none=True)
    none = torch.zeros_like(mask)
    loss, _ = m.mlm_loss(masked.to(DEV), none.to(DEV), _index(none, target, V), 0, 0)
    loss.backward()
    assert float(loss) == 0.0
    assert all(p.grad is None or not p.grad.any() for p in m.parameters())


@pytest.mark.parametrize("rcps", [False, True], ids=["ph", "rcps"])
def test_mlm_loss_empty_mask_batch(rcps):
    m = _tiny(rcps).to(DEV)
    masked, mask, target = _batch(B, L, 12)
    none = torch.zeros_like(mask)
    loss, logits = m.mlm_loss(target.to(DEV), none.to(DEV), _index(none, target, 16), 0, 0)
    assert logits is None and float(loss) == 0.0
    loss.backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() and not g.any() for g in grads)


def test_optimizer_hooks_fused_adamw_matches_torch():
    """Three steps with weight_decay 0.1 and the hooks' group at weight_decay 0, against
    torch.optim.AdamW on fp32 copies grouped by the same rule, with the same gradients; agreement
    as tests/test_gpu_blm_pretrain.py asks: 1e-6 times max(1, |p|). A_log and D carry no
    weight-decay term: a decay-all reference is far outside that."""
    from dna_amd.flat import FlatParams
    from dna_amd.optim import FusedAdamW, ParamGroups, add_optimizer_hooks
    lr, wd = 5e-3, 0.1
    m = _tiny(True).to(DEV)
    add_optimizer_hooks(m)
    names = [n for n, _ in m.named_parameters()]
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    allwd = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    pg = ParamGroups(m)
    assert len(pg) == 2
    flat = FlatParams(m, DEV, shadow_dtype=None, group_of=pg)
    opt = FusedAdamW(flat, lr=lr, weight_decay=wd, max_grad_norm=1.0, groups=pg)
    assert [g["weight_decay"] for g in opt.param_groups] == [wd, 0.0]
    assert [g["lr"] for g in opt.param_groups] == [lr, lr]
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
    ssm = [n for n in names if n.endswith(".A_log") or n.endswith(".D")]
    assert ssm and all(hasattr(params[n], "_optim") for n in ssm)
    for n in ssm:  # lr * wd * |p| per step would show
        tol = 1e-6 * max(1.0, float(ref[n].detach().abs().max()))
        assert float((params[n].detach() - allwd[n].detach()).abs().max()) > 10 * tol, n
    sd = opt.state_dict()
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(pg.members(0)), len(pg.members(1))]
    assert sd["param_groups"][1]["weight_decay"] == 0.0
    topt.load_state_dict(sd)  # torch accepts it


def _trainer(m, **kw):
    from dna_amd.optim import add_optimizer_hooks
    from dna_amd.trainer import BlmTrainer
    add_optimizer_hooks(m)
    return BlmTrainer(m, torch.device(DEV), weight_decay=0.1, **kw)


def test_blm_trainer_bf16_trains_caduceus():
    m = _tiny(True, perturb=False)
    tr = _trainer(m, lr=2e-3, seed=5,
                  scheduler={"t_initial": 20, "warmup_t": 1, "warmup_lr_init": 1e-4,
                             "lr_min": 6e-5, "t_in_epochs": False})
    assert len(tr.opt.param_groups) == 2 and tr.flat.shadow is not None
    assert tr.opt.param_groups[1]["weight_decay"] == 0.0 and tr.vocab_size == 16
    masked, mask, target = _batch(B, L, 12)
    db = tr.device_batch(masked, mask, _labels(mask, target), target)
    assert db.n_mask == int(mask.sum())
    losses = [float(tr.step(db)) for _ in range(4)]
    print("caduceus bf16 losses", losses)
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    assert torch.isfinite(tr.flat.flat).all()
    assert tr.global_step == 4 and tr.sched._last_epoch == 4 and len(tr.micro_losses) == 1


def test_blm_trainer_accumulation_equals_one_step_caduceus():
    """fp32: accum = 2 over two half-batches with equally many masked positions is the step over
    the whole batch, to this model's fp32 forward limit (1e-4, max-norm relative; the scan
    backward adds dA / dB / dC with atomics, the head and its fold do not); the first AdamW step
    then moves every parameter with a gradient that is not tiny by the same +-lr."""
    lr = 1e-3
    base = _tiny(True)
    masked, mask, target = _batch(4, L, 12, per_row=45)
    out = []
    for split in (False, True):
        tr = _trainer(copy.deepcopy(base), lr=lr, autocast=None, seed=1)
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
    from dna_amd.synthetic import write_hg38
    root = tmp_path_factory.mktemp("caduceus_hg38")
    write_hg38(str(root), n_chroms=2, chrom_len=60_000, max_length=256)
    return str(root)


TINY = ["experiment=caduceus/bert_hg38_caduceus", "dataset.max_length=256", "dataset.batch_size=4",
        "dataset.num_workers=0", "model.config.d_model=64", "model.config.n_layer=2",
        "optimizer.lr=2e-3", "trainer.devices=1", "trainer.max_epochs=1",
        "trainer.limit_train_batches=4", "trainer.limit_val_batches=2",
        "trainer.log_every_n_steps=1", "scheduler.t_initial=20", "scheduler.warmup_t=2",
        "scheduler.lr_min=2e-4", "wandb=null"]


def test_train_caduceus_runs_checkpoints_resumes_and_feeds_finetuning(data_root, monkeypatch, tmp_path):
    import finetune
    import train
    from dna_amd.caduceus import CaduceusForSequenceClassification
    from dna_amd.compose import compose
    from dna_amd.optim import TimmCosineLRScheduler
    monkeypatch.setenv("DATA_PATH", data_root)
    monkeypatch.chdir(tmp_path)
    cfg = compose(os.path.join(ROOT, "configs"), "config", TINY)
    buf = io.StringIO()
    tr = train.train(cfg, out=buf)
    logs = [json.loads(l) for l in buf.getvalue().splitlines()]
    assert type(tr).__name__ == "BlmTrainer" and isinstance(tr.sched, TimmCosineLRScheduler)
    assert type(tr.model).__name__ == "CaduceusForMaskedLM" and tr.model.config["rcps"]
    assert tr.global_step == 4 and len(tr.opt.param_groups) == 2
    assert [g["weight_decay"] for g in tr.opt.param_groups] == [0.1, 0.0]
    tl = [l for l in logs if "train/loss" in l]
    assert [l["step"] for l in tl] == [1, 2, 3, 4]
    assert all(math.isfinite(l["train/loss"]) and math.isfinite(l["train/perplexity"]) for l in tl)
    # the first step sees the initial weights: the tied embedding has std 0.02, so the logits of
    # the 2 x 64 normalised channels have a std of about 0.02 sqrt(128) = 0.23 and the loss is
    # log(16) up to a few hundredths
    assert abs(tl[0]["train/loss"] - math.log(16)) < 0.25
    ev = [l for l in logs if "val/loss" in l]
    assert len(ev) == 1 and ev[0]["step"] == 4
    for k in ("val/loss", "val/perplexity", "test/loss", "test/perplexity"):
        assert math.isfinite(ev[0][k]) and ev[0][k] > 0, k
    last = tmp_path / "checkpoints" / "last.ckpt"
    assert os.path.exists(last)
    ck = torch.load(last, map_location="cpu", weights_only=True)
    assert ck["global_step"] == 4 and len(ck["optimizer_states"][0]["param_groups"]) == 2
    assert ck["lr_schedulers"][0]["_last_epoch"] == 4
    assert "model.lm_head.complement_map" in ck["state_dict"]
    # resume: step, schedule and both optimizer groups come back (max_epochs reached: no step)
    cfg2 = compose(os.path.join(ROOT, "configs"), "config",
                   TINY + [f"trainer.resume_from_checkpoint={last}"])
    tr2 = train.train(cfg2, out=io.StringIO())
    assert tr2.global_step == 4 and tr2.sched._last_epoch == 4 and tr2.opt.step_count == 4
    assert tr2.sched.get_last_lr() == tr.sched.get_last_lr()
    assert [(g["lr"], g["weight_decay"], g["initial_lr"]) for g in tr2.opt.param_groups] == \
        [(g["lr"], g["weight_decay"], g["initial_lr"]) for g in tr.opt.param_groups]
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
    # the checkpoint is what finetune.py's train.pretrained_model_path takes
    config = cfg.model.config.to_container()
    config["complement_map"] = tr.model.config["complement_map"]
    cls = CaduceusForSequenceClassification(num_labels=2, **config)
    info = finetune.load_pretrained(cls, ck["state_dict"])
    assert info["missing"] == ["score.weight"], info  # every backbone key matched
    assert info["unexpected"] == 2  # lm_head.lm_head.weight, lm_head.complement_map
    want = {k: v for k, v in tr.model.state_dict().items() if k.startswith("caduceus.")}
    got = cls.state_dict()
    assert want and all(torch.equal(got[k].cpu(), v.cpu()) for k, v in want.items())
    ids = torch.randint(7, 11, (2, 256), generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():
        assert torch.equal(cls.to(DEV).eval().caduceus(ids), tr.model.eval().caduceus(ids))


# ----------------------------------------------------------------------------------- two ranks
def _ddp_batch(seed, b):
    """Exactly 45 masked positions per sequence: every rank's masked-token mean then weighs its
    tokens as the concatenated batch's mean does, so the mean of rank means is that mean."""
    return _batch(b, L, 12, seed=seed, per_row=45)


def _ddp_trainer(seed, device):
    from dna_amd.optim import add_optimizer_hooks
    from dna_amd.trainer import BlmTrainer
    m = _tiny(True, seed=seed)
    add_optimizer_hooks(m)
    return BlmTrainer(m, torch.device(device), lr=2e-3, weight_decay=0.1, autocast=None,
                      bucket_mb=0.05, seed=0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = rank % torch.cuda.device_count()
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr = _ddp_trainer(seed=rank, device=f"cuda:{dev}")  # the broadcast fixes the init
        for step in range(2):
            masked, mask, target = _ddp_batch(10 * step + rank, 2)
            tr.step(tr.device_batch(masked, mask, _labels(mask, target), target))
            torch.cuda.synchronize()
        q.put((rank, dict(flat=tr.flat.flat.cpu().numpy(), scale=tr.reducer.grad_scale,
                          groups=len(tr.opt.param_groups))))
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 visible devices")
def test_caduceus_pretrain_two_ranks_equal_single_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    tr = _ddp_trainer(seed=0, device="cuda:0")
    p0 = tr.flat.flat.clone()
    for step in range(2):
        a, b = _ddp_batch(10 * step, 2), _ddp_batch(10 * step + 1, 2)
        masked, mask, target = (torch.cat([x, y]) for x, y in zip(a, b))
        tr.step(tr.device_batch(masked, mask, _labels(mask, target), target))
    torch.cuda.synchronize()
    ref = tr.flat.flat.cpu()
    r0, r1 = (torch.from_numpy(res[r]["flat"]) for r in (0, 1))
    assert torch.equal(r0, r1)  # replicas identical
    assert res[0]["scale"] == 0.5 and res[0]["groups"] == 2
    assert (ref - p0.cpu()).abs().max().item() > 0.5 * 2e-3  # two AdamW steps moved the parameters
    assert (r0 - ref).abs().max().item() < 2e-5  # tests/test_gpu_caduceus_ddp.py's fp32 limit
