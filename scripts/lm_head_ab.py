#!/usr/bin/env python
"""Masked-LM head measurements (GPU): the fused small-vocabulary head (DF.MaskedLMHead,
csrc/lm_head.hip) against the dense path it replaces, and its kernels' share of the HBM peak.

    python scripts/lm_head_ab.py [--out results.json] [--reps 50] [--no-step] [--no-profile]

1. Head only, forward + backward, bf16 hidden states: T = 131072 rows (config D: 2 x 65536),
   D = 256, V = 16, 15 % of the rows kept. Dense arm: hip_linear under bf16 autocast -> .float()
   -> F.cross_entropy(ignore_index, sum) / count -> autograd (what scripts/hyena_lm_bench.py runs).
2. Full step: the config-D training step (HyenaDNA-small, 8 layers, B = 2, L = 65536, bf16,
   ModuleTrainer) with BertLMHeadModel.mlm_loss against the bench script's dense loss.
HIP events around each repetition, the two arms interleaved, median after warm-up.
3. Kernel share of peak: a child process runs the fused head under `rocprofv3 --kernel-trace
   --stats`; per kernel the algorithmic bytes over its mean time, against the HBM peak of MI355X
   (8.0 TB/s specified, 6.29 TB/s measured with a float4 copy). Algorithmic bytes: rows_kernel
   reads the kept rows of h; dh_kernel writes every element of dh; dw_part_kernel reads the kept
   rows of h again (coef, W, labels and the partial sums are under 3 % of that and not counted).
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dna_amd import functional as DF  # noqa: E402

DEV = "cuda"
T, D, V, KEEP = 131072, 256, 16, 0.15
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes / s: specified peak, measured float4 copy


def _head_arms():
    from dna_amd.hyena import hip_linear
    g = torch.Generator().manual_seed(1)
    h = torch.randn(T, D, generator=g).to(DEV).to(torch.bfloat16).requires_grad_(True)
    w = torch.nn.Parameter((torch.randn(V, D, generator=g) * 0.05).to(DEV))
    w._dna_lp = w.detach().to(torch.bfloat16)  # the shadow a trainer keeps
    y = torch.randint(0, V, (T,), generator=g)
    labels = torch.where(torch.rand(T, generator=g) < KEEP, y, torch.full_like(y, -100)).to(DEV)
    kept = int((labels >= 0).sum())

    def fused():
        h.grad = w.grad = None
        loss, _ = DF.masked_lm_head(h, w, labels)
        loss.backward()
        return loss

    def dense():
        h.grad = w.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = hip_linear(h, w)
        ce = F.cross_entropy(logits.float(), labels, ignore_index=-100, reduction="none")
        loss = ce.sum() / (labels != -100).sum()
        loss.backward()
        return loss

    return {"fused": fused, "dense": dense}, kept


def _interleaved(arms, reps, warmup):
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return times


def head_ab(reps):
    arms, kept = _head_arms()
    lf, ld = float(arms["fused"]().detach()), float(arms["dense"]().detach())
    times = _interleaved(arms, reps, 10)
    row = dict(T=T, D=D, V=V, kept_rows=kept, dtype="bf16", reps=reps, loss_fused=lf, loss_dense=ld)
    for k, ts in times.items():
        row[f"{k}_us_median"] = round(statistics.median(ts), 2)
        row[f"{k}_us_min"] = round(min(ts), 2)
    row["fused_over_dense"] = round(row["fused_us_median"] / row["dense_us_median"], 4)
    print(json.dumps(row), flush=True)
    return row


def step_ab(reps, B=2, L=65536, layers=8):
    from dna_amd.hyena_lm import BertLMHeadModel, BlmIndex
    from dna_amd.trainer import ModuleTrainer
    layer = {"_name_": "hyena", "emb_dim": 5, "filter_order": 64, "short_filter_order": 3,
             "l_max": L, "modulate": True, "w": 10, "lr_pos_emb": 0.0, "bidirectional": True}
    g = torch.Generator(device=DEV).manual_seed(1)
    ids = torch.randint(7, 11, (B, L), device=DEV, generator=g)
    masked = torch.rand(B, L, device=DEV, generator=g) < 0.15
    inp = torch.where(masked, torch.full_like(ids, 3), ids)
    labels = torch.where(masked, ids, torch.full_like(ids, -100)).view(-1)
    index = BlmIndex.build(masked.cpu(), ids.cpu(), 16).to(DEV)

    def dense_loss(model, batch):
        (out, _) = model(batch)
        logits = out.logits[0]
        ce = F.cross_entropy(logits.reshape(-1, logits.shape[-1]).float(), labels,
                             ignore_index=-100, reduction="none")
        return ce.sum() / (labels != -100).sum()

    def fused_loss(model, batch):
        return model.mlm_loss(batch[0], batch[1], index)[0]

    arms = {}
    for name, fn in (("fused", fused_loss), ("dense", dense_loss)):
        torch.manual_seed(0)
        m = BertLMHeadModel(d_model=256, n_layer=layers, d_inner=1024, vocab_size=12,
                            pad_vocab_size_multiple=8, embed_dropout=0.1, residual_in_fp32=True,
                            layer=layer)
        tr = ModuleTrainer(m, DEV, fn, lr=6e-4, weight_decay=0.1, max_grad_norm=1.0)
        arms[name] = (lambda tr=tr: tr.step((inp, masked)))
    times = _interleaved(arms, reps, 3)
    row = dict(B=B, L=L, layers=layers, dtype="bf16", reps=reps,
               loss_fused=float(arms["fused"]()), loss_dense=float(arms["dense"]()))
    for k, ts in times.items():
        row[f"{k}_ms_median"] = round(statistics.median(ts) / 1e3, 3)
        row[f"{k}_ms_min"] = round(min(ts) / 1e3, 3)
    row["fused_over_dense"] = round(row["fused_ms_median"] / row["dense_ms_median"], 4)
    print(json.dumps(row), flush=True)
    return row


def child(reps=20, warmup=5):
    arms, _ = _head_arms()
    for _ in range(warmup + reps):
        arms["fused"]()
    torch.cuda.synchronize()


def kernel_shares(profile_dir, kept):
    d = os.path.join(profile_dir, "lm_head")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o",
           "run", "--", "timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__),
           "--child"]
    # the inner `timeout` ends the process that holds the GPU
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    if r.returncode != 0:
        raise SystemExit(f"rocprofv3 failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    nbytes = {"rows_kernel": kept * D * 2, "dh_kernel": T * D * 2, "dw_part_kernel": kept * D * 2,
              "finish_kernel": None, "dw_finish_kernel": None}
    row = dict(T=T, D=D, V=V, kept_rows=kept, kernels={})
    with open(os.path.join(d, "run_kernel_stats.csv"), newline="") as f:
        for rec in csv.DictReader(f):
            for k, nb in nbytes.items():
                if f"lmh::{k}" in rec["Name"]:
                    us = float(rec["AverageNs"]) / 1e3
                    e = {"calls": int(rec["Calls"]), "mean_us": round(us, 2),
                         "min_us": round(float(rec["MinNs"]) / 1e3, 2)}
                    if nb:
                        rate = nb / (us * 1e-6)
                        e.update(bytes=nb, TB_per_s=round(rate / 1e12, 3),
                                 share_of_spec_peak=round(rate / HBM_SPEC, 3),
                                 share_of_copy_peak=round(rate / HBM_COPY, 3))
                    row["kernels"][k] = e
    if set(row["kernels"]) != set(nbytes):
        raise SystemExit(f"lm-head kernels found: {sorted(row['kernels'])}")
    total = sum(e["mean_us"] for e in row["kernels"].values())
    moved = sum(nb for nb in nbytes.values() if nb)
    row["all_kernels_us"] = round(total, 2)
    row["all_bytes_share_of_spec_peak"] = round(moved / (total * 1e-6) / HBM_SPEC, 3)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-dir", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lm_head_ab.py measures on the GPU; none found")
    if a.child:
        return child()
    res = {"head": head_ab(a.reps)}
    if not a.no_step:
        res["step"] = step_ab(a.step_reps)
    if not a.no_profile:
        with tempfile.TemporaryDirectory() as tmp:
            res["kernels"] = kernel_shares(a.profile_dir or tmp, res["head"]["kept_rows"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
