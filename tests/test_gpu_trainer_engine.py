"""What the trainers share through ModuleTrainer's one step (GPU): the fine-tuning trainers step
their schedule exactly once per step, their RNG state replays a run bit for bit, and a tuple
batch reaches ModuleTrainer's loss_fn as that tuple."""
import math

import pytest
import torch

from oracle import optim_ref
from oracle.hashinit import hash_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE_LR = 1e-3
SCHED = dict(t_in_epochs=False, t_initial=100, warmup_t=5, warmup_lr_init=1e-6, lr_min=1e-5)


def _cls_trainer():
    """ClsTrainer on a 2-layer d = 64 BERT classifier with dropout 0.1; b = 5, S = 72."""
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import ClsTrainer
    cfg = dict(vocab_size=4096, hidden_size=64, num_hidden_layers=2, num_attention_heads=1,
               intermediate_size=128, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0,
               layer_norm_eps=1e-12, type_vocab_size=2, pad_token_id=0, num_labels=3)
    m = BertForSequenceClassification(cfg)
    m.load_state_dict({k: torch.from_numpy(hash_tensor(k, tuple(v.shape)))
                       for k, v in m.state_dict().items()}, strict=True)
    tr = ClsTrainer(m, DEV, lr=BASE_LR, scheduler=SCHED, seed=1)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(5, 4096, (5, 72), generator=g)
    ids[::2, 40:] = 3
    return tr, ids.to(DEV), torch.randint(0, 3, (5,), generator=g).to(DEV)


def _seqcls_trainer():
    """SeqClsTrainer on a 2-layer HyenaDNA classifier with embedding dropout 0.1; b = 3, L = 130."""
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.hyena_lm import DNAEmbeddingModel
    from dna_amd.trainer import SeqClsTrainer
    L = 130
    layer = {"_name_": "hyena", "emb_dim": 5, "filter_order": 16, "short_filter_order": 3,
             "l_max": L, "modulate": True, "w": 10, "lr_pos_emb": 0.0}
    torch.manual_seed(11)
    emb = DNAEmbeddingModel(d_model=64, n_layer=2, d_inner=256, vocab_size=16, embed_dropout=0.1,
                            residual_in_fp32=True, layer=layer)
    tr = SeqClsTrainer(SequenceClassifier(emb, 2, mode="pool"), torch.device(DEV), lr=BASE_LR,
                       weight_decay=0.1, seed=5, scheduler=SCHED)
    ids = torch.randint(0, 16, (3, L), generator=torch.Generator().manual_seed(4)).to(DEV)
    return tr, ids, torch.tensor([1, 0, 1], device=DEV)


def _snapshot(tr):
    return (tr.flat.flat.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone(),
            tr.opt.step_count, tr.sched._last_epoch, tr.rng_state())


def _restore(tr, snap):
    flat, m1, m2, count, epoch, rng = snap
    with torch.no_grad():
        for p, (o, n, shape) in zip(tr.flat.params, tr.flat.slices):
            p.copy_(flat[o:o + n].view(shape))  # in place through torch: the trainer sees it
    tr.opt.exp_avg.copy_(m1)
    tr.opt.exp_avg_sq.copy_(m2)
    tr.opt.step_count = count
    tr.sched.step(epoch=epoch)
    tr.load_rng_state(rng)


@pytest.mark.parametrize("make", [_cls_trainer, _seqcls_trainer])
def test_schedule_steps_once_per_step_and_rng_state_replays(make):
    """lr of group 0 after 3 steps = the schedule's closed form at t = 3 (the CPU schedule
    tests' restatement, to their 1e-12: the same float64 formula). Then, from a snapshot of
    parameters, moments and counters: rng_state -> 2 steps -> everything put back with
    load_rng_state -> the same 2 steps give the same loss bits, and the state that was put back
    is not the one the steps left behind (so the dropout draws were in fact replayed)."""
    tr, ids, labels = make()
    for _ in range(3):
        tr.step(ids, labels)
    assert tr.global_step == 3 and tr.sched._last_epoch == 3
    want = optim_ref.linear_warmup_lr(3, BASE_LR, SCHED["warmup_t"], SCHED["t_initial"],
                                      SCHED["warmup_lr_init"], SCHED["lr_min"])
    assert math.isclose(tr.opt.param_groups[0]["lr"], want, rel_tol=1e-12)
    snap = _snapshot(tr)
    first = [tr.step(ids, labels).clone() for _ in range(2)]
    after = tr.rng_state()
    assert any(not torch.equal(torch.as_tensor(after[k]), torch.as_tensor(snap[5][k]))
               for k in after)
    _restore(tr, snap)
    again = [tr.step(ids, labels).clone() for _ in range(2)]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
    assert tr.sched._last_epoch == 5


def test_module_trainer_hands_a_tuple_batch_to_loss_fn_whole():
    """ModuleTrainer.step(batch) is one micro-batch whatever its type: a tuple is not taken for
    a list of micro-batches (that rule belongs to MLMTrainer / BlmTrainer.step)."""
    from dna_amd.trainer import ModuleTrainer
    torch.manual_seed(0)
    seen = []

    def loss_fn(model, batch):
        seen.append(batch)
        x, y = batch
        return ((model(x) - y) ** 2).mean()

    tr = ModuleTrainer(torch.nn.Linear(64, 64), DEV, loss_fn, autocast=None)
    batch = (torch.randn(2, 64, device=DEV), torch.randn(2, 64, device=DEV))
    before = tr.flat.flat.clone()
    loss = tr.step(batch)
    assert len(seen) == 1 and seen[0] is batch
    assert loss.shape == () and bool(torch.isfinite(loss)) and tr.global_step == 1
    assert not torch.equal(before, tr.flat.flat)
