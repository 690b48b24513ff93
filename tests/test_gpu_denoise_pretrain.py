"""GPU: denoise_cnn (registry model denoise_cnn, CNNModel(pretrain=True)) masked-LM pretraining,
end to end.

* the model against the reference's pretraining forward + bert_cross_entropy, as recorded by
  tests/golden/make_denoise_pretrain_golden.py (denoise_pretrain.npz: configurations P -- D 64,
  k 9, dilations 1, 1, 2, 4, 8 at L 96, forget -- and Q -- D 128, k 5, dilations 1, 1, 3 at L 200,
  add, final_conv), with the weights rebuilt from the same hash. The bounds are
  tests/test_gpu_denoise_model.py's:
    fp32   masked logits and loss within 1e-3; per parameter the sampled gradient elements within
           1e-3 relative L2 and the gradient norm within 1e-3 (the gradients are mlm_loss's: the
           compacted tail and the fused head), with every library GEMM / convolution banned.
    bf16   through BlmTrainer under autocast: logits max / rms error <= 2x the reference's own
           bf16-vs-fp32 error, gradients <= 2x its error + 5e-3, loss <= 2x its error + 1e-3.
* mlm_loss (compact tail, and the dense one behind DNA_DENOISE_MLM_TAIL=dense) against
  F.cross_entropy on forward's dense logits, fp32: the loss and every parameter gradient within
  the fp32 bound above; an empty mask gives loss 0 and finite all-zero gradients.
* BlmTrainer: bf16 steps train at D 64, L 128; accum = 2 over two half-batches = one step (fp32);
  one full bf16 step with an odd M under DNA_STRICT_NATIVE=1 and every library entry banned.
* train.train(cfg) on a synthetic FASTA / BED with the new experiment: logs, last.ckpt, resume;
  finetune.finetune(cfg) of denoise/genomic_benchmark_denoise loads that checkpoint and steps.
* two ranks (one device each) = one process on the concatenated batch.
"""
import copy
import importlib.util
import io
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from test_gpu_blm_pretrain import _index, _labels
from test_gpu_denoise_model import _ban_libraries, _toy_folder
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _maker():
    spec = importlib.util.spec_from_file_location(
        "make_denoise_pretrain_golden", os.path.join(GOLDEN, "make_denoise_pretrain_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _maker()
Z = np.load(os.path.join(GOLDEN, "denoise_pretrain.npz"))


def _model(tag):
    """CNNModel(pretrain=True) of configuration `tag` with the fixture's hashed weights, and the
    fixture's batch (ids already masked to 4, mask, target) on the host."""
    from dna_amd.denoise import CNNModel
    keys = json.loads(Z[f"{tag}/keys"].tobytes().decode())
    m = CNNModel(**MK.model_kwargs(MK.CONFIGS[tag]))
    m.load_state_dict(MK.denoise_state(keys), strict=True)
    ids = torch.as_tensor(Z[f"{tag}/ids"].astype(np.int64))
    mask = torch.as_tensor(Z[f"{tag}/mask"])
    target = torch.as_tensor(Z[f"{tag}/target"].astype(np.int64))
    assert int(mask.sum()) % 64 and bool(mask[:, 0].all()) and bool(mask[:, -1].all())
    assert bool((ids[mask] == 4).all()) and int(target[mask].max()) <= 3
    return m, ids, mask, target


def _rel_l2(a, b):
    a, b = a.detach().double().reshape(-1).cpu(), b.detach().double().reshape(-1).cpu()
    return float((a - b).norm() / b.norm())


def _assert_grads_close(got, want, tol=1e-3):
    """Per parameter: relative L2 of the difference and the norms, both within tol."""
    worst = (0.0, None)
    for n, g in got.items():
        assert g is not None and want[n] is not None, n
        rel = _rel_l2(g, want[n])
        worst = max(worst, (rel, n))
        assert rel <= tol, (n, rel)
        gn, rn = float(g.double().norm()), float(want[n].double().norm())
        assert abs(gn - rn) <= tol * rn, (n, gn, rn)
    return worst


# --------------------------------------------------------------------------- against the fixture
@pytest.mark.parametrize("tag", ["P", "Q"])
def test_fp32_logits_loss_and_gradients_vs_reference_fixture(tag, monkeypatch):
    m, ids, mask, target = _model(tag)
    m = m.to(DEV).eval()
    V = 5
    with monkeypatch.context() as mp_:
        _ban_libraries(mp_)
        md = mask.to(DEV)
        out, none = m((ids.to(DEV), md))
        logits, mask_out = out.logits
        loss, compact = m.mlm_loss(ids.to(DEV), md, _index(mask, target, V))
        loss.backward()
    assert none is None and compact is None and mask_out is md  # the reference's return value
    assert type(loss.grad_fn).__name__ == "MaskedLMHeadBackward"
    assert tuple(logits.shape) == (*ids.shape, V) and logits.dtype == torch.float32
    l32 = Z[f"{tag}/logits32"]
    rows = logits.detach()[mask.to(DEV)].float().cpu().numpy()
    lerr = float(np.abs(rows - l32).max())
    print(f"denoise pretrain {tag} fp32: masked logits err {lerr:.3e} (max |logit| "
          f"{np.abs(l32).max():.3f}), loss {loss.item():.6f} vs {float(Z[f'{tag}/loss32']):.6f}")
    assert lerr <= 1e-3
    assert abs(loss.item() - float(Z[f"{tag}/loss32"])) <= 1e-3
    worst = (0.0, None)
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        g = p.grad.detach().reshape(-1).cpu().numpy().astype(np.float64)
        g32 = Z[f"{tag}/gs32/{n}"].astype(np.float64)
        rel = np.linalg.norm(g[Z[f"{tag}/gidx/{n}"].astype(np.int64)] - g32) / np.linalg.norm(g32)
        worst = max(worst, (float(rel), n))
        assert rel <= 1e-3, (n, rel)
        gn, rn = float(np.linalg.norm(g)), float(Z[f"{tag}/gradnorm32/{n}"])
        assert abs(gn - rn) <= 1e-3 * rn, (n, gn, rn)
    print(f"denoise pretrain {tag} fp32: worst sampled-gradient relative L2 {worst[0]:.3e} "
          f"({worst[1]})")


@pytest.mark.parametrize("tag", ["P", "Q"])
def test_bf16_train_step_vs_reference_fixture(tag):
    from dna_amd.trainer import BlmTrainer
    m, ids, mask, target = _model(tag)
    tr = BlmTrainer(m, torch.device(DEV), lr=1e-3, weight_decay=0.0, max_grad_norm=1.0,
                    autocast=torch.bfloat16)
    m.eval()  # the fixture is eval mode (no dropout)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out, _ = m((ids.to(DEV), mask.to(DEV)))
    rows = out.logits[0][mask.to(DEV)].float().cpu().numpy()
    l32, l16 = Z[f"{tag}/logits32"], Z[f"{tag}/logitsbf16"]
    ref_max, ref_rms = np.abs(l16 - l32).max(), np.sqrt(((l16 - l32) ** 2).mean())
    our_max, our_rms = np.abs(rows - l32).max(), np.sqrt(((rows - l32) ** 2).mean())
    print(f"denoise pretrain {tag} bf16: logits max {our_max:.3e} (reference {ref_max:.3e}), rms "
          f"{our_rms:.3e} ({ref_rms:.3e})")
    assert our_max <= 2 * ref_max, (our_max, ref_max)
    assert our_rms <= 2 * ref_rms, (our_rms, ref_rms)
    loss = tr.step(tr.device_batch(ids, mask, _labels(mask, target), target))
    torch.cuda.synchronize()
    ref_loss_err = abs(float(Z[f"{tag}/lossbf16"]) - float(Z[f"{tag}/loss32"]))
    print(f"denoise pretrain {tag} bf16: loss {loss.item():.6f} vs fp32 record "
          f"{float(Z[f'{tag}/loss32']):.6f} (reference's bf16 error {ref_loss_err:.3e})")
    assert abs(loss.item() - float(Z[f"{tag}/loss32"])) <= 2 * ref_loss_err + 1e-3
    worst = (-math.inf, None, 0.0)
    for n, p in m.named_parameters():
        g = p.grad.detach().reshape(-1).cpu().numpy()
        g32, g16 = Z[f"{tag}/gs32/{n}"], Z[f"{tag}/gsbf16/{n}"]
        nref = np.linalg.norm(g32)
        err = np.linalg.norm(g[Z[f"{tag}/gidx/{n}"].astype(np.int64)] - g32) / nref
        ref_err = np.linalg.norm(g16 - g32) / nref
        worst = max(worst, (float(err - 2 * ref_err), n, float(err)))
        assert err <= 2 * ref_err + 5e-3, (n, err, ref_err)
    print(f"denoise pretrain {tag} bf16: largest (err - 2 ref_err) {worst[0]:.3e} at {worst[1]} "
          f"(err {worst[2]:.3e})")


# ------------------------------------------------------------- mlm_loss against the dense forward
@pytest.fixture(scope="module")
def dense_reference():
    """Per configuration, once: F.cross_entropy on forward's dense logits at the masked
    positions, and autograd's gradient of every parameter."""
    res = {}
    for tag in ("P", "Q"):
        m, ids, mask, target = _model(tag)
        m = m.to(DEV).eval()
        out, _ = m((ids.to(DEV), mask.to(DEV)))
        logits, mk = out.logits
        loss = F.cross_entropy(logits[mk].float(), target.to(DEV)[mk])
        loss.backward()
        res[tag] = (float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters()})
    return res


@pytest.mark.parametrize("tail", ["compact", "dense"])
@pytest.mark.parametrize("tag", ["P", "Q"])
def test_mlm_loss_equals_cross_entropy_on_the_dense_logits(tag, tail, dense_reference, monkeypatch):
    monkeypatch.setenv("DNA_DENOISE_MLM_TAIL", tail)
    want_loss, want = dense_reference[tag]
    m, ids, mask, target = _model(tag)
    m = m.to(DEV).eval()
    loss, logits = m.mlm_loss(ids.to(DEV), mask.to(DEV), _index(mask, target, 5),
                              int(mask.sum()), 0)
    assert logits is None
    loss.backward()
    assert abs(float(loss.detach()) - want_loss) <= 1e-3
    worst = _assert_grads_close({n: p.grad for n, p in m.named_parameters()}, want)
    print(f"denoise pretrain {tag} {tail} tail vs dense logits: loss {float(loss.detach()):.6f} / "
          f"{want_loss:.6f}, worst gradient relative L2 {worst[0]:.3e} ({worst[1]})")


@pytest.mark.parametrize("tail", ["compact", "dense"])
def test_mlm_loss_empty_mask_batch(tail, monkeypatch):
    monkeypatch.setenv("DNA_DENOISE_MLM_TAIL", tail)
    m, ids, mask, target = _model("Q")
    m = m.to(DEV).eval()
    none = torch.zeros_like(mask)
    loss, logits = m.mlm_loss(target.to(DEV), none.to(DEV), _index(none, target, 5), 0, 0)
    assert logits is None and float(loss.detach()) == 0.0
    loss.backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and not bool(p.grad.any()), n


def test_bad_tail_switch_is_refused(monkeypatch):
    monkeypatch.setenv("DNA_DENOISE_MLM_TAIL", "sparse")
    m, ids, mask, target = _model("P")
    with pytest.raises(ValueError, match="DNA_DENOISE_MLM_TAIL"):
        m.to(DEV).mlm_loss(ids.to(DEV), mask.to(DEV), _index(mask, target, 5))


# ------------------------------------------------------------------------------------- trainer
B, L = 4, 128


def _tiny(seed=7, **kw):
    """D 64, three gated layers (k 5, dilations 1, 1, 2), torch's default init."""
    from dna_amd.denoise import CNNModel
    c = dict(MK.CONFIGS["P"], num_conv1d=3, k=5, dilation=2)
    torch.manual_seed(seed)
    return CNNModel(**dict(MK.model_kwargs(c), **kw))


def _batch(b, seed=4, per_row=19):
    """(ids, mask, target) in the one-hot id space as objective stdmlm_onehot builds them: bases
    0..3 with an N run and a trailing N (the end-of-sequence position), exactly per_row masked
    bases per row (N never), 80 % of them shown as 4, the rest unchanged."""
    g = torch.Generator().manual_seed(seed)
    target = torch.randint(0, 4, (b, L), generator=g)
    target[:, 40:46] = 4
    target[:, -1] = 4
    mask = torch.zeros(b, L, dtype=torch.bool)
    for r in range(b):
        ok = torch.nonzero(target[r] != 4).flatten()
        mask[r, ok[torch.randperm(ok.numel(), generator=g)[:per_row]]] = True
    ids = torch.where(mask & (torch.rand(b, L, generator=g) < 0.8), torch.full_like(target, 4), target)
    return ids, mask, target


def _trainer(m, **kw):
    from dna_amd.trainer import BlmTrainer
    return BlmTrainer(m, torch.device(DEV), weight_decay=0.0, **kw)


def test_blm_trainer_bf16_trains_denoise_cnn():
    tr = _trainer(_tiny(), lr=2e-3, seed=5,
                  scheduler={"t_initial": 20, "warmup_t": 1, "warmup_lr_init": 1e-4,
                             "lr_min": 2e-4, "t_in_epochs": False})
    assert tr.flat.shadow is not None and tr.vocab_size == 5 and len(tr.opt.param_groups) == 1
    ids, mask, target = _batch(B)
    db = tr.device_batch(ids, mask, _labels(mask, target), target)
    assert db.n_mask == int(mask.sum()) == B * 19
    losses = [float(tr.step(db)) for _ in range(6)]
    print("denoise_cnn bf16 losses", losses)
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    assert torch.isfinite(tr.flat.flat).all()
    assert tr.global_step == 6 and tr.sched._last_epoch == 6


def test_blm_trainer_accumulation_equals_one_step_denoise_cnn():
    """fp32: accum = 2 over two half-batches with equally many masked positions is the step over
    the whole batch, to the fp32 bound of this file (1e-3 relative L2 of the flat gradient; no
    kernel of this model adds with atomics, what differs is the order of the partial sums), and
    the first AdamW step moves every parameter with a gradient that is not tiny by the same
    +-lr."""
    lr = 1e-3
    base = _tiny()
    ids, mask, target = _batch(B)
    out = []
    for split in (False, True):
        tr = _trainer(copy.deepcopy(base), lr=lr, autocast=None, seed=1)
        assert tr.flat.shadow is None
        before = tr.flat.flat.clone()
        if split:
            mbs = [tr.device_batch(ids[i:i + 2], mask[i:i + 2],
                                   _labels(mask[i:i + 2], target[i:i + 2]), target[i:i + 2])
                   for i in (0, 2)]
            loss = tr.step(mbs, accum=2)
            assert len(tr.micro_losses) == 2
        else:
            loss = tr.step(tr.device_batch(ids, mask, _labels(mask, target), target))
        out.append((float(loss), tr.flat.grad.clone(), tr.flat.flat - before))
    (la, ga, da), (lb, gb, db) = out
    assert abs(la - lb) <= 1e-3 * abs(la)
    assert _rel_l2(gb, ga) <= 1e-3
    big = ga.abs() > 1e-3 * ga.abs().max()
    assert big.any() and float((da - db)[big].abs().max()) < 1e-2 * lr


@pytest.mark.parametrize("final_conv", [False, True], ids=["mlp", "mlp+final_conv"])
def test_full_step_is_native_for_an_odd_number_of_masked_rows(final_conv, monkeypatch):
    """M = 4 * 19 + 1 = 77 rows through the compacted tail: no library GEMM, no counted
    fallback, in a whole bf16 trainer step."""
    tr = _trainer(_tiny(final_conv=final_conv), lr=1e-3, seed=2)
    ids, mask, target = _batch(B)
    free = torch.nonzero((target[0] != 4) & ~mask[0]).flatten()
    mask[0, free[0]] = True
    assert int(mask.sum()) == 77
    db = tr.device_batch(ids, mask, _labels(mask, target), target)
    before = tr.flat.flat.clone()
    with monkeypatch.context() as mp_:
        _ban_libraries(mp_)
        loss = tr.step(db)
        torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and abs(float(loss) - math.log(5)) < 1.0
    assert torch.isfinite(tr.flat.flat).all() and not torch.equal(tr.flat.flat, before)
    for n, p in tr.model.named_parameters():
        assert bool(p.grad.any()), n  # every parameter, out_linear.bias included, got a gradient


# ------------------------------------------------------------------------------ train.train(cfg)
@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    from dna_amd.synthetic import write_hg38
    root = tmp_path_factory.mktemp("denoise_hg38")
    write_hg38(str(root), n_chroms=2, chrom_len=60_000, max_length=256)
    return str(root)


SMALL = ["model.args.hidden_dim=64", "model.d_model=64", "model.num_conv1d=3", "model.kernel_size=5",
         "model.dilation=2"]
TINY = ["experiment=denoise/bert_hg38_denoise", "dataset.max_length=256", "dataset.batch_size=4",
        "dataset.num_workers=0", "optimizer.lr=2e-3", "trainer.devices=1", "trainer.max_epochs=1",
        "trainer.limit_train_batches=4", "trainer.limit_val_batches=2",
        "trainer.log_every_n_steps=1", "scheduler.t_initial=20", "scheduler.warmup_t=2",
        "scheduler.lr_min=2e-4", "wandb=null"] + SMALL


def test_train_denoise_cnn_runs_checkpoints_resumes_and_feeds_finetuning(data_root, monkeypatch,
                                                                         tmp_path):
    import finetune
    import train
    from dna_amd.compose import compose
    from dna_amd.optim import TimmCosineLRScheduler
    monkeypatch.setenv("DATA_PATH", data_root)
    monkeypatch.chdir(tmp_path)
    configs = os.path.join(ROOT, "configs")
    cfg = compose(configs, "config", TINY)
    buf = io.StringIO()
    tr = train.train(cfg, out=buf)
    logs = [json.loads(l) for l in buf.getvalue().splitlines()]
    assert type(tr).__name__ == "BlmTrainer" and isinstance(tr.sched, TimmCosineLRScheduler)
    assert type(tr.model).__name__ == "CNNModel" and tr.model.pretrain and tr.vocab_size == 5
    assert tr.global_step == 4 and len(tr.opt.param_groups) == 1
    tl = [l for l in logs if "train/loss" in l]
    assert [l["step"] for l in tl] == [1, 2, 3, 4]
    assert all(math.isfinite(l["train/loss"]) and math.isfinite(l["train/perplexity"]) for l in tl)
    # four balanced classes are scored (N is never a label): the first loss is near log(4..5)
    assert abs(tl[0]["train/loss"] - math.log(5)) < 1.0
    ev = [l for l in logs if "val/loss" in l]
    assert len(ev) == 1 and ev[0]["step"] == 4
    for k in ("val/loss", "val/perplexity", "test/loss", "test/perplexity"):
        assert math.isfinite(ev[0][k]) and ev[0][k] > 0, k
    last = tmp_path / "checkpoints" / "last.ckpt"
    assert os.path.exists(last)
    ck = torch.load(last, map_location="cpu", weights_only=True)
    assert ck["global_step"] == 4 and ck["lr_schedulers"][0]["_last_epoch"] == 4
    assert "model.out_linear.weight" in ck["state_dict"] and "model.out_linear.bias" in ck["state_dict"]
    assert not any("lm_head" in k for k in ck["state_dict"])
    # resume: step, schedule and optimizer state come back (max_epochs reached: no step)
    cfg2 = compose(configs, "config", TINY + [f"trainer.resume_from_checkpoint={last}"])
    tr2 = train.train(cfg2, out=io.StringIO())
    assert tr2.global_step == 4 and tr2.sched._last_epoch == 4 and tr2.opt.step_count == 4
    assert tr2.sched.get_last_lr() == tr.sched.get_last_lr()
    for a, b in zip(tr.model.parameters(), tr2.model.parameters()):
        assert torch.equal(a, b)
    for pa, pb in zip(tr.model.parameters(), tr2.model.parameters()):
        oa, na, _ = tr.flat.slice_of(pa)
        ob, nb, _ = tr2.flat.slice_of(pb)
        assert torch.equal(tr.opt.exp_avg[oa:oa + na], tr2.opt.exp_avg[ob:ob + nb])
        assert torch.equal(tr.opt.exp_avg_sq[oa:oa + na], tr2.opt.exp_avg_sq[ob:ob + nb])
    # and trains on: one more epoch from the checkpoint
    cfg3 = compose(configs, "config", TINY + [f"trainer.resume_from_checkpoint={last}",
                                              "trainer.max_epochs=2"])
    tr3 = train.train(cfg3, out=io.StringIO())
    assert tr3.global_step == 8 and tr3.sched._last_epoch == 8
    # the first run's checkpoint (tr3 has overwritten last.ckpt) feeds finetune.py
    pre = tmp_path / "pretrained.ckpt"
    torch.save(ck, pre)
    _toy_folder(str(tmp_path / "gb"))
    ft = compose(configs, "config",
                 ["experiment=denoise/genomic_benchmark_denoise", f"dataset.dest_path={tmp_path / 'gb'}",
                  "dataset.dataset_name=toy", "dataset.max_length=48", "dataset.batch_size=16",
                  "dataset.eval_batch_size=16", "trainer.max_epochs=1", "train.max_steps=1",
                  "trainer.log_every_n_steps=1", f"train.pretrained_model_path={pre}",
                  "callbacks.model_checkpoint.dirpath=" + str(tmp_path / "ft_ckpt"),
                  "wandb=null"] + SMALL)
    fbuf = io.StringIO()
    metrics = finetune.finetune(ft, out=fbuf)
    events = [json.loads(l) for l in fbuf.getvalue().splitlines()]
    load = [e for e in events if e.get("event") == "load_backbone"]
    assert load and load[0]["loaded"] == "backbone"
    steps = [e for e in events if e.get("event") == "train"]
    assert steps and steps[0]["step"] == 1 and math.isfinite(steps[0]["trainer/loss"])
    assert math.isfinite(metrics["val/loss"])
    # the loaded backbone is the pretrained one: the fine-tuning checkpoint's untouched input
    # layer of the reverse-complement stream differs from it by one AdamW step at most
    fck = torch.load(tmp_path / "ft_ckpt" / "last.ckpt", map_location="cpu", weights_only=True)
    a, b = fck["state_dict"]["model.model.rc_linear.weight"], ck["state_dict"]["model.rc_linear.weight"]
    assert float((a - b).abs().max()) <= 2 * 1e-3


# ----------------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_trainer(seed, device):
    from dna_amd.trainer import BlmTrainer
    return BlmTrainer(_tiny(seed=seed), torch.device(device), lr=2e-3, weight_decay=0.0,
                      autocast=None, bucket_mb=0.05, seed=0)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = rank % torch.cuda.device_count()
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr = _ddp_trainer(seed=rank, device=f"cuda:{dev}")  # the broadcast fixes the init
        for step in range(2):
            ids, mask, target = _batch(2, seed=10 * step + rank)
            tr.step(tr.device_batch(ids, mask, _labels(mask, target), target))
            torch.cuda.synchronize()
        q.put((rank, dict(flat=tr.flat.flat.cpu().numpy(), scale=tr.reducer.grad_scale)))
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 visible devices")
def test_denoise_pretrain_two_ranks_equal_single_process():
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
        a, b = _batch(2, seed=10 * step), _batch(2, seed=10 * step + 1)
        ids, mask, target = (torch.cat([x, y]) for x, y in zip(a, b))
        tr.step(tr.device_batch(ids, mask, _labels(mask, target), target))
    torch.cuda.synchronize()
    ref = tr.flat.flat.cpu()
    r0, r1 = (torch.from_numpy(res[r]["flat"]) for r in (0, 1))
    assert torch.equal(r0, r1)  # replicas identical
    assert res[0]["scale"] == 0.5
    assert (ref - p0.cpu()).abs().max().item() > 0.5 * 2e-3  # two AdamW steps moved the parameters
    assert (r0 - ref).abs().max().item() < 2e-5  # tests/test_gpu_caduceus_ddp.py's fp32 limit
