#!/usr/bin/env python
"""Pooling-head measurements (GPU): the fused head (DF.PoolHead, csrc/pool_head.hip) against the
torch composition it replaces, and its kernels' share of the HBM peak.

    python scripts/pool_head_ab.py [--out results.json] [--reps 50] [--no-profile]

A/B: forward (with loss) + backward, bf16 hidden states, at (B, L, D, C) =
  (64, 1026, 128, 2)        HyenaDNA genomic-benchmark shape (launch-bound in both arms)
  (8, 65536, 256, 2)        a long-sequence batch
  (1, 131072, 2 x 256, 2)   one RCPS sequence, both halves read in place
  (128, 1024, 256, 919)     DeepSEA on HyenaDNA: the wide head (multi-label), bf16 and fp32 x
The Hyena torch arm is mean(1) -> F.linear -> cross_entropy and its autograd; the RCPS torch arm
is the reference's stack / flip / mean / score per strand / average (modeling_caduceus.py:
550-591); the DeepSEA torch arm is mean(1) -> F.linear -> binary_cross_entropy_with_logits. HIP events around each repetition, the two arms interleaved, median after warm-up;
kernel launches per repetition counted with torch.profiler in a repetition of their own.
Kernel share of peak: per shape, a child process runs the fused arm under `rocprofv3
--kernel-trace --stats`; the algorithmic bytes (x read once in the forward, dx written once in
the backward) over the mean time of the whole-tensor kernel of that pass, against the HBM peak
of MI355X (8.0 TB/s specified, 6.29 TB/s measured with a float4 copy).
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
PROBLEM, MULTI = "single_label_classification", "multi_label_classification"
SHAPES = [dict(B=64, L=1026, D=128, C=2, rcps=False), dict(B=8, L=65536, D=256, C=2, rcps=False),
          dict(B=1, L=131072, D=256, C=2, rcps=True),
          dict(B=128, L=1024, D=256, C=919, rcps=False, dtype="bf16", problem=MULTI),
          dict(B=128, L=1024, D=256, C=919, rcps=False, dtype="fp32", problem=MULTI)]
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes / s: specified peak, measured float4 copy


def algorithmic_bytes(s):
    """Bytes one pass must move: every element of the hidden state once."""
    es = 4 if s.get("dtype") == "fp32" else 2
    return s["B"] * s["L"] * s["D"] * (2 if s["rcps"] else 1) * es


def _arms(B, L, D, C, rcps, dtype="bf16", problem=PROBLEM):
    g = torch.Generator().manual_seed(B + L)
    width = 2 * D if rcps else D
    xdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    x = torch.randn(B, L, width, generator=g).to(DEV).to(xdt).requires_grad_(True)
    w = (torch.randn(C, D, generator=g) * 0.03).to(DEV).requires_grad_(True)
    b = None if rcps else (torch.randn(C, generator=g) * 0.03).to(DEV).requires_grad_(True)
    if problem == MULTI:
        labels = (torch.rand(B, C, generator=g) < 0.4).float().to(DEV)
        torch_loss = F.binary_cross_entropy_with_logits
    else:
        labels = torch.randint(0, C, (B,), generator=g).to(DEV)
        torch_loss = F.cross_entropy

    def clear():
        x.grad = w.grad = None
        if b is not None:
            b.grad = None

    def fused():
        clear()
        _, loss, _ = DF.pool_head(x, w, b, rcps=rcps, mirror2=rcps, labels=labels,
                                  problem_type=problem)
        loss.backward()

    def composed():
        clear()
        if rcps:
            h = torch.stack([x[..., :D], torch.flip(x[..., D:], dims=[1, 2])], dim=-1)
            p = h.mean(dim=1).float()
            logits = (F.linear(p[..., 0], w) + F.linear(p[..., 1], w)) / 2
        else:
            logits = F.linear(x.mean(1).float(), w, b)
        torch_loss(logits, labels).backward()

    return fused, composed


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def head_ab(reps, warmup=10, shapes=None):
    out = []
    for s in (SHAPES if shapes is None else [SHAPES[i] for i in shapes]):
        arms = dict(zip(("fused", "composed"), _arms(**s)))
        for _ in range(warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():  # interleaved
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3)
        row = dict(s, reps=reps, dtype=s.get("dtype", "bf16"), pass_bytes=algorithmic_bytes(s))
        for k in arms:
            row[f"{k}_us_median"] = round(statistics.median(times[k]), 2)
            row[f"{k}_us_min"] = round(min(times[k]), 2)
            row[f"{k}_launches"] = _launches(arms[k])
        out.append(row)
        print(json.dumps(row), flush=True)
        del arms
        torch.cuda.empty_cache()
    return out


def child(index, reps=20, warmup=5):
    """The fused arm alone, for the profiler: one shape per process, so that the per-kernel
    statistics belong to that shape."""
    fused, _ = _arms(**SHAPES[index])
    for _ in range(warmup + reps):
        fused()
    torch.cuda.synchronize()


KERNELS = {"partial_kernel": "fwd", "finish_kernel": None, "loss_kernel": None,
           "grad_kernel": None, "bcast_kernel": "bwd"}
WIDE_KERNELS = {"partial_kernel": "fwd", "pooled_kernel": None, "wide_logits_kernel": None,
                "wide_loss_kernel": None, "wide_loss_finish_kernel": None,
                "wide_grad_kernel": None, "bcast_kernel": "bwd"}


def kernel_shares(profile_dir, shapes=None):
    out = []
    for i, s in enumerate(SHAPES):
        if shapes is not None and i not in shapes:
            continue
        kernels = WIDE_KERNELS if s["C"] > 64 else KERNELS
        d = os.path.join(profile_dir, f"shape{i}")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o",
               "run", "--", "timeout", "-k", "10", "240", sys.executable,
               os.path.abspath(__file__), "--child", str(i)]
        # the inner `timeout` ends the process that holds the GPU; the outer limit would only
        # end the profiler in front of it
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            raise SystemExit(f"rocprofv3 failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
        path = os.path.join(d, "run_kernel_stats.csv")
        row = dict(s, pass_bytes=algorithmic_bytes(s), kernels={})
        with open(path, newline="") as f:
            for rec in csv.DictReader(f):
                for k, which in kernels.items():
                    if f"pool::{k}" in rec["Name"]:
                        us = float(rec["AverageNs"]) / 1e3
                        e = {"calls": int(rec["Calls"]), "mean_us": round(us, 2),
                             "min_us": round(float(rec["MinNs"]) / 1e3, 2)}
                        if which:
                            rate = row["pass_bytes"] / (us * 1e-6)
                            e.update(TB_per_s=round(rate / 1e12, 3),
                                     share_of_spec_peak=round(rate / HBM_SPEC, 3),
                                     share_of_copy_peak=round(rate / HBM_COPY, 3))
                        row["kernels"][k] = e
        if set(row["kernels"]) != set(kernels):
            raise SystemExit(f"{path}: pool-head kernels found: {sorted(row['kernels'])}")
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-dir", default=None, help="where rocprofv3 writes (default: a "
                    "temporary folder)")
    ap.add_argument("--shapes", type=int, nargs="*", default=None,
                    help="indices into SHAPES (default: all)")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_head_ab.py measures on the GPU; none found")
    if a.child is not None:
        return child(a.child)
    res = {"head": head_ab(a.reps, shapes=a.shapes)}
    if not a.no_profile:
        with tempfile.TemporaryDirectory() as tmp:
            res["kernels"] = kernel_shares(a.profile_dir or tmp, shapes=a.shapes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
