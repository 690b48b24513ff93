#!/usr/bin/env python
"""Bit digests of the trainers' steps and of the two classification-loss kernels (GPU), to
compare two commits:

    python scripts/trainer_digest.py --out a.jsonl [--dump DIR]
    python scripts/trainer_digest.py --compare parent_1.jsonl parent_2.jsonl head.jsonl \
        [--dumps DIR_1 DIR_2 DIR_HEAD]

Only public API that both commits have, so the same file runs in a copy of the older tree. One
JSON line per case, from fixed seeds and tiny models (the BERT models hash-initialised,
oracle/hashinit.py; the others from torch's CPU generator): the loss bits of each of 3 steps,
SHA-256 of flat.flat, opt.exp_avg_sq and (where there is one) flat.shadow after the last step,
the lr of every param group, global_step and the RNG state; for the loss kernels the loss /
dlogits / pred bits. --dump also writes each case's final flat.flat as DIR/<case>.npy.

--compare: which cases the first commit reproduces bit for bit between two fresh processes, and
whether the second commit equals it. Where the first commit does not reproduce itself (atomics
in the Caduceus scan backward) and the dumps are given: max |flat difference| of the two parent
runs, and of the head against each of them.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
GOLDEN = os.path.join(ROOT, "tests", "golden")
SINGLE, REGRESSION, MULTI = ("single_label_classification", "regression",
                             "multi_label_classification")


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _bits(t):
    t = t.detach().reshape(-1).cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else t.dtype).tolist()


def _rng(st):
    return {k: (_sha(v) if torch.is_tensor(v) else v) for k, v in st.items()}


def _digest(tr, losses, rng_state=None):
    torch.cuda.synchronize()
    d = {"loss_bits": [_bits(v)[0] for v in losses], "flat": _sha(tr.flat.flat),
         "exp_avg_sq": _sha(tr.opt.exp_avg_sq), "lr": [g["lr"] for g in tr.opt.param_groups],
         "global_step": tr.global_step}
    if tr.flat.shadow is not None:
        d["shadow"] = _sha(tr.flat.shadow)
    if rng_state is not None:
        d["rng"] = _rng(rng_state)
    return d


def _hash_init(m, tied=()):
    from oracle.hashinit import hash_tensor
    tied = dict(tied)
    m.load_state_dict({k: torch.from_numpy(hash_tensor(tied.get(k, k), tuple(v.shape)))
                       for k, v in m.state_dict().items()}, strict=True)
    return m


def _bert_cfg(**kw):
    z = np.load(os.path.join(GOLDEN, "model_tiny.npz"))
    L, d, H, Fd = json.loads(z["config"].tobytes().decode())
    cfg = dict(vocab_size=4096, hidden_size=d, num_hidden_layers=L, num_attention_heads=H,
               intermediate_size=Fd, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0,
               layer_norm_eps=1e-12, max_position_embeddings=512, type_vocab_size=2,
               pad_token_id=0, alibi_starting_size=512, hidden_act="gelu", initializer_range=0.02)
    cfg.update(kw)
    return z, cfg


SCHED = dict(t_in_epochs=False, t_initial=100, warmup_t=2, warmup_lr_init=1e-6, lr_min=0.0)


def mlm_case(precision, micro):
    from dna_amd.bert_layers import BertForMaskedLM
    from dna_amd.trainer import MLMTrainer
    z, cfg = _bert_cfg(hyena_framework=True)
    m = _hash_init(BertForMaskedLM(cfg, precision=precision),
                   [("cls.predictions.decoder.weight", "bert.embeddings.word_embeddings.weight")])
    tr = MLMTrainer(m, torch.device(DEV, 0), lr=1e-3, weight_decay=1e-5, scheduler=SCHED, seed=7)
    host = [torch.as_tensor(z[k].astype(np.int64)) for k in ("masked_ids", "labels", "target")]
    mask = torch.as_tensor(z["mask"])
    batches = [tr.device_batch(host[0], mask, host[1], host[2]),
               tr.device_batch(host[0].flip(0), mask.flip(0), host[1].flip(0), host[2].flip(0))]
    losses = [tr.step(batches[0]) if micro == 1 else tr.step(batches, accum=2) for _ in range(3)]
    return tr, losses, tr.rng_state()


def cls_case():
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import ClsTrainer
    _, cfg = _bert_cfg(num_labels=3, problem_type=SINGLE)
    m = _hash_init(BertForSequenceClassification(cfg))
    tr = ClsTrainer(m, DEV, lr=1e-4, scheduler=SCHED, seed=1)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(5, 4096, (5, 72), generator=g)
    ids[:, 0] = 1
    ids[::2, 40:] = 3
    labels = torch.randint(0, 3, (5,), generator=g).to(DEV)
    losses = [tr.step(ids.to(DEV), labels) for _ in range(3)]
    return tr, losses, tr.rng_state()


def _hyena_layer(L, **kw):
    return dict({"_name_": "hyena", "emb_dim": 5, "filter_order": 16, "short_filter_order": 3,
                 "l_max": L, "modulate": True, "w": 10, "lr_pos_emb": 0.0}, **kw)


def _perturb(m, seed):
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if not n.endswith("freq"):
                p.add_(torch.randn_like(p) * 0.02)
    return m


def seqcls_case(frozen):
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.hyena_lm import DNAEmbeddingModel, load_backbone
    from dna_amd.trainer import SeqClsTrainer
    L = 130
    torch.manual_seed(11)
    emb = DNAEmbeddingModel(d_model=64, n_layer=2, d_inner=256, vocab_size=16, embed_dropout=0.1,
                            residual_in_fp32=True, layer=_hyena_layer(L))
    m = _perturb(SequenceClassifier(emb, 2, mode="pool"), 3)
    if frozen:
        load_backbone(m.model, {k: v.clone() for k, v in m.model.state_dict().items()},
                      freeze_backbone=True)
    tr = SeqClsTrainer(m, torch.device(DEV), lr=1e-3, weight_decay=0.1, seed=5, scheduler=SCHED)
    ids = torch.randint(0, 16, (3, L), generator=torch.Generator().manual_seed(4)).to(DEV)
    labels = torch.tensor([1, 0, 1], device=DEV)
    losses = [tr.step(ids, labels) for _ in range(3)]
    return tr, losses, tr.rng_state()


def blm_case(autocast):
    from dna_amd.hyena_lm import BertLMHeadModel
    from dna_amd.trainer import BlmTrainer
    L, V = 130, 12
    torch.manual_seed(12)
    m = BertLMHeadModel(d_model=64, n_layer=2, d_inner=256, vocab_size=V, pad_vocab_size_multiple=8,
                        embed_dropout=0.1, residual_in_fp32=True,
                        layer=_hyena_layer(L, bidirectional=True, wd=0.0, lr=2e-3))
    tr = BlmTrainer(_perturb(m, 3), torch.device(DEV), lr=2e-3, weight_decay=0.1, seed=5,
                    autocast=autocast,
                    scheduler={"t_initial": 20, "warmup_t": 1, "warmup_lr_init": 1e-4,
                               "lr_min": 6e-5, "t_in_epochs": False})
    batches = []
    for seed in (4, 5):
        g = torch.Generator().manual_seed(seed)
        target = torch.randint(0, V, (3, L), generator=g)
        mask = torch.rand(3, L, generator=g) < 0.15
        masked = torch.where(mask & (torch.rand(3, L, generator=g) < 0.8),
                             torch.full_like(target, 3), target)
        labels = torch.where(mask, target, torch.full_like(target, -100))
        batches.append(tr.device_batch(masked, mask, labels, target))
    losses = [tr.step(batches, accum=2) for _ in range(3)]
    return tr, losses, tr.rng_state()


def _caduceus_loss(model, batch):
    inp, labels = batch
    return model(inp, labels=labels)[0]


def module_case():
    from dna_amd.caduceus import CaduceusForMaskedLM
    from dna_amd.trainer import ModuleTrainer
    L = 1024
    torch.manual_seed(0)
    m = CaduceusForMaskedLM(d_model=64, n_layer=2, vocab_size=12, ssm_cfg={"d_state": 16})
    tr = ModuleTrainer(m, DEV, _caduceus_loss, lr=2e-3, weight_decay=0.1, max_grad_norm=1.0,
                       bucket_mb=0.05, autocast=torch.bfloat16)
    g = torch.Generator().manual_seed(10)
    ids = torch.randint(7, 11, (2, L), generator=g)
    masked = torch.zeros(2, L, dtype=torch.bool)
    for i in range(2):
        masked[i, torch.randperm(L, generator=g)[:150]] = True
    inp = torch.where(masked, torch.full_like(ids, 3), ids).to(DEV)
    labels = torch.where(masked, ids, torch.full_like(ids, -100)).to(DEV)
    losses = [tr.step((inp, labels)) for _ in range(3)]
    return tr, losses, None


def _loss_inputs(problem, B, C, edge):
    g = torch.Generator().manual_seed(1000 * B + C)
    x = torch.randn(B, C, generator=g) * 2.0
    if problem == SINGLE:
        labels = torch.randint(0, C, (B,), generator=g)
    else:
        labels = torch.randn(B, C, generator=g) if problem == REGRESSION else \
            (torch.rand(B, C, generator=g) < 0.5).float()
    if edge:
        x[1, 1] = x[1, 3] = x[1].max() + 1.0  # a tied maximum
        x[2] = 0.0                             # all equal
        labels[4] = C                          # out of range
    return x, labels


def loss_case(kernel, problem, B, C, edge=False):
    """-> loss / dlogits / pred bits of dna_cls_loss (fp32 rows) or of the pool head's loss
    (double rows; L = 1 and D = 4, or W = the identity for the edge case, so logits = x)."""
    from dna_amd import functional as DF
    from dna_amd import ops  # noqa: F401  (registers torch.ops.dna_amd.*)
    x, labels = _loss_inputs(problem, B, C, edge)
    if kernel == "cls":
        logits = x.to(DEV)
        loss, dl = torch.empty(1, device=DEV), torch.empty(B, C, device=DEV)
        pred = torch.empty(B, device=DEV, dtype=torch.int64) if problem == SINGLE else None
        lab = labels if problem == SINGLE else labels.reshape(-1)
        torch.ops.dna_amd.cls_loss(logits, lab.to(DEV).contiguous(), DF.CLS_PROBLEMS[problem],
                                   loss, dl, pred)
    else:
        if edge:
            h, w = x.reshape(B, 1, C), torch.eye(C)
        else:
            g = torch.Generator().manual_seed(B + C)
            h, w = torch.randn(B, 1, 4, generator=g), torch.randn(C, 4, generator=g)
        w = w.to(DEV).requires_grad_(True)  # a graph, for the saved dlogits
        logits, loss, pred = DF.pool_head(h.to(DEV), w, labels=labels.to(DEV), problem_type=problem)
        dl = logits.grad_fn.saved_tensors[2]
    torch.cuda.synchronize()
    return {"loss_bits": _bits(loss), "logits": _sha(logits), "dlogits": _sha(dl),
            "pred": None if pred is None else _sha(pred)}


def cases():
    out = {}
    for prec in ("fp32", "bf16"):
        for micro in (1, 2):
            out[f"mlm_{prec}_micro{micro}"] = lambda p=prec, k=micro: mlm_case(p, k)
    out["cls_dropout_sched"] = cls_case
    out["seqcls_hyena"] = lambda: seqcls_case(False)
    out["seqcls_hyena_frozen"] = lambda: seqcls_case(True)
    out["blm_bf16_accum2"] = lambda: blm_case(torch.bfloat16)
    out["blm_fp32_accum2"] = lambda: blm_case(None)
    out["module_caduceus_tuple"] = module_case
    return out


def run(out, dump):
    if dump:
        os.makedirs(dump, exist_ok=True)
    with open(out, "w") if out else sys.stdout as f:
        for name, fn in cases().items():
            tr, losses, rng = fn()
            print(json.dumps(dict(case=name, **_digest(tr, losses, rng))), file=f, flush=True)
            if dump:
                np.save(os.path.join(dump, name + ".npy"), tr.flat.flat.detach().cpu().numpy())
        for kernel in ("cls", "pool"):
            for problem in (SINGLE, REGRESSION, MULTI):
                for B, C in ((1, 1), (5, 3), (3, 64), (1030, 2)):
                    d = loss_case(kernel, problem, B, C)
                    print(json.dumps(dict(case=f"loss_{kernel}_{problem}_{B}x{C}", **d)), file=f)
            d = loss_case(kernel, SINGLE, 6, 4, edge=True)
            print(json.dumps(dict(case=f"loss_{kernel}_tie_and_out_of_range", **d)), file=f)


def compare(files, dumps):
    a1, a2, b = ({d["case"]: d for d in map(json.loads, open(p))} for p in files)
    print(f"{'case':46s} {'parent reproduces':18s} head equals parent")
    ok = True
    for name, d in a1.items():
        repro = d == a2[name]
        same = b.get(name) == d
        note = ""
        if not repro and dumps:
            x1, x2, y = (np.load(os.path.join(p, name + ".npy")).astype(np.float64) for p in dumps)
            own = np.abs(x1 - x2).max()
            head = max(np.abs(y - x1).max(), np.abs(y - x2).max())
            note = f"  max|flat diff| parent/parent {own:.3e}, head/parent {head:.3e}"
        ok = ok and (same or not repro)
        print(f"{name:46s} {str(repro):18s} {str(same) if repro else 'n/a'}{note}")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=3, metavar="JSONL")
    ap.add_argument("--dumps", nargs=3, metavar="DIR")
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare, args.dumps)
    run(args.out, args.dump)
    return 0


if __name__ == "__main__":
    sys.exit(main())
