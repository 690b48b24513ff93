#!/usr/bin/env python
"""Golden fixture for masked-LM pretraining of the gated dilated CNN (dna_amd/denoise.py,
CNNModel(pretrain=True, for_representation=False)), produced by running the REFERENCE's CNNModel
(src/models/sequence/denoise.py, the `self.pretrain` branch of forward) on the CPU.

Run from the repo root:  python tests/golden/make_denoise_pretrain_golden.py
The reference is imported by path through make_denoise_golden.py (loaded as a module: its
stand-ins for the absent packages and its `denoise_state` weights are reused, nothing is copied).
Writes tests/golden/denoise_pretrain.npz with two configurations, eval mode:

  P  D 64,  k 9, dilation 2, num_conv1d 5, d_inner 2, B 3, L 96:  forget, use_comp, no final_conv
  Q  D 128, k 5, dilation 3, num_conv1d 3, d_inner 2, B 2, L 200: forget off, use_comp, final_conv

The weights are denoise_state's hash of (key, index): the file holds none. Ids lie in 0..4 with
runs of 4 (N). The mask covers positions 0 and L - 1 of every row and about 15 % of the others,
trimmed so that M is no multiple of 64; the input ids are the targets with every masked position
set to 4, as objective stdmlm_onehot shows a masked base. The loss is the reference's
bert_cross_entropy (src/tasks/metrics.py:268-273): F.cross_entropy(logits[mask], target[mask]).
Per configuration <X> and precision <p> in 32 | bf16 (CPU torch.autocast(bfloat16)):

  <X>/ids, <X>/mask, <X>/target, <X>/config, <X>/keys (JSON [[key, shape], ...] of the state dict)
  <X>/logits<p>    the logits at the masked rows [M, 5], fp32
  <X>/loss<p>
  <X>/gidx/<key>   up to 512 seeded element indices of the parameter's gradient
  <X>/gs<p>/<key>, <X>/gradnorm<p>/<key>   those elements, and the whole gradient's L2 norm
"""
import importlib.util
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
N_SAMPLE = 512

CONFIGS = {
    "P": dict(D=64, k=9, dilation=2, num_conv1d=5, d_inner=2, B=3, L=96, forget=True,
              use_comp=True, final_conv=False),
    "Q": dict(D=128, k=5, dilation=3, num_conv1d=3, d_inner=2, B=2, L=200, forget=False,
              use_comp=True, final_conv=True),
}


def _base():
    spec = importlib.util.spec_from_file_location("make_denoise_golden",
                                                  os.path.join(HERE, "make_denoise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _base()
denoise_state = MK.denoise_state


def model_kwargs(c):
    """The constructor arguments of CNNModel (the reference's and dna_amd.denoise's) for a
    configuration of CONFIGS: the fine-tuning ones with pretrain on and for_representation off."""
    kw = MK.model_kwargs(c)
    kw.update(pretrain=True, for_representation=False, final_conv=c["final_conv"])
    return kw


def make_batch(c, seed):
    """-> target [B, L] in 0..4 with runs of N, mask [B, L] bool, ids = target with 4 at the mask.
    Positions 0 and L - 1 of every row are masked; M % 64 != 0."""
    target, _ = MK.make_batch(c, seed)
    target[:, 0] = np.arange(c["B"]) % 4  # a base at position 0 (make_batch pads it with N)
    target[:, -1] = (np.arange(c["B"]) + 1) % 4
    rng = np.random.default_rng(seed + 1)
    mask = (rng.random(target.shape) < 0.15) & (target != 4)
    mask[:, 0] = mask[:, -1] = True
    if int(mask.sum()) % 64 == 0:
        b, l = np.argwhere(mask[:, 1:-1])[0]
        mask[b, l + 1] = False
    ids = np.where(mask, 4, target)
    return ids.astype(np.int64), mask, target.astype(np.int64)


def main():
    CNNModel = MK._reference_cnn()
    torch.set_num_threads(8)
    pick = np.random.default_rng(11)
    res = {}
    for tag, c in CONFIGS.items():
        ids, mask, target = make_batch(c, 200 + ord(tag))
        res[f"{tag}/ids"], res[f"{tag}/target"] = ids.astype(np.int8), target.astype(np.int8)
        res[f"{tag}/mask"] = mask
        res[f"{tag}/config"] = np.bytes_(json.dumps(c))
        tmask, ttarget = torch.as_tensor(mask), torch.as_tensor(target)
        for prec in ("32", "bf16"):
            m = CNNModel(**model_kwargs(c)).eval()
            keys = [(k, list(v.shape)) for k, v in m.state_dict().items()]
            res[f"{tag}/keys"] = np.bytes_(json.dumps(keys))
            m.load_state_dict(denoise_state(keys), strict=True)
            with torch.autocast("cpu", dtype=torch.bfloat16, enabled=prec == "bf16"):
                out, _ = m((torch.as_tensor(ids), tmask))
                logits, mask_out = out.logits
                assert mask_out is tmask
                rows = logits[tmask]
                loss = F.cross_entropy(rows.float(), ttarget[tmask])
            loss.backward()
            res[f"{tag}/logits{prec}"] = rows.detach().float().numpy()
            res[f"{tag}/loss{prec}"] = np.float64(loss.item())
            for n, p in m.named_parameters():
                g = p.grad.detach().float().reshape(-1).numpy()
                if prec == "32":
                    k = min(N_SAMPLE, g.size)
                    res[f"{tag}/gidx/{n}"] = np.sort(pick.choice(g.size, k, replace=False)).astype(
                        np.uint16 if g.size <= 65536 else np.int32)
                res[f"{tag}/gradnorm{prec}/{n}"] = np.float64(np.linalg.norm(g.astype(np.float64)))
                res[f"{tag}/gs{prec}/{n}"] = g[res[f"{tag}/gidx/{n}"].astype(np.int64)]
            print(f"denoise_cnn pretrain {tag}: precision {prec}, M {int(mask.sum())}, logits "
                  f"{tuple(logits.shape)} {logits.dtype}, loss {loss.item():.6f}")
    path = os.path.join(HERE, "denoise_pretrain.npz")
    np.savez_compressed(path, **res)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
