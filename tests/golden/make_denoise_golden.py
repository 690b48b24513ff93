#!/usr/bin/env python
"""Golden fixture for the gated dilated-CNN backbone (dna_amd/denoise.py), produced by running the
REFERENCE's CNNModel (src/models/sequence/denoise.py) on the CPU.

Run from the repo root:  python tests/golden/make_denoise_golden.py
Imports the reference's denoise.py by path (read-only, never copied). The packages its module body
imports but the `mode: dilation` path never calls -- flash_attn, timm, fftconv and its own
src.models.sequence.convNext -- are stood in for by empty modules whose attributes are empty
classes. Writes tests/golden/denoise_cnn.npz with two configurations:

  A  D 64,  k 9, dilation 4, num_conv1d 5, d_inner 2, B 3, L 96:  dilations 1, 1, 4, 16, 64 (the
     last one's padding of 256 exceeds L), forget=True, use_comp=False
  B  D 128, k 5, dilation 3, num_conv1d 4, d_inner 2, B 2, L 200: dilations 1, 1, 3, 9,
     forget=False, use_comp=True

Weights are `denoise_state` below (oracle/hashinit.py's hash of (key, index), so the tests rebuild
them and the file holds none): LayerNorm gammas in [0.5, 1.5], every bias non-zero. Ids lie in
0..4 with runs of 4 (N). Per configuration <X> and precision <p> in 32 (fp32) | bf16 (CPU
torch.autocast(bfloat16), as the reference's `precision: bf16` trains), eval mode:

  <X>/ids, <X>/labels, <X>/config, <X>/keys (JSON [[key, shape], ...] of the reference's state
                   dict; the pool decoder Linear(D, 2) is hashed under DECODER_KEYS)
  <X>/feat<p>      the backbone output [B, L, D] (bf16: the bf16 bits as uint16 when the reference
                   returns bf16)
  <X>/logits<p>    mean over L -> Linear(D, 2) (the reference's SequenceDecoder, mode pool), fp32
  <X>/loss<p>      cross entropy of the logits and the labels
  <X>/gidx/<key>   up to 1,024 seeded element indices of the parameter's gradient
  <X>/gs<p>/<key>, <X>/gradnorm<p>/<key>   those elements, and the whole gradient's L2 norm
"""
import importlib.abc
import importlib.machinery
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("DNA_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
N_SAMPLE = 1024

CONFIGS = {
    "A": dict(D=64, k=9, dilation=4, num_conv1d=5, d_inner=2, B=3, L=96, forget=True,
              use_comp=False),
    "B": dict(D=128, k=5, dilation=3, num_conv1d=4, d_inner=2, B=2, L=200, forget=False,
              use_comp=True),
}
DECODER_KEYS = ("decoder.0.output_transform.weight", "decoder.0.output_transform.bias")


def model_kwargs(c):
    """The constructor arguments of CNNModel (the reference's and dna_amd.denoise's) for a
    configuration of CONFIGS."""
    args = types.SimpleNamespace(mode="dilation", hidden_dim=c["D"], num_cnn_stacks=1, dropout=0.0,
                                 clean_data=False, cls_free_guidance=False,
                                 cls_expanded_simplex=True)
    return dict(args=args, alphabet_size=5, num_cls=0, for_representation=True, pretrain=False,
                dilation=c["dilation"], kernel_size=c["k"], mlp=True, use_outlinear=False,
                forget=c["forget"], num_conv1d=c["num_conv1d"], d_inner=c["d_inner"],
                final_conv=False, use_comp=c["use_comp"])


def _is_norm(key):
    return key.startswith(("norms.", "rc_norms.", "milinear.3.", "milinear.7."))


def denoise_state(named_shapes):
    """{key: fp32 tensor} for (key, shape) pairs of a CNNModel state dict (+ DECODER_KEYS), every
    element a hash of (key, index): weights uniform with std 1 / sqrt(fan_in) (the one-hot input
    layers: fan_in 9, one active channel per tap), LayerNorm gammas in [0.5, 1.5], every bias
    uniform in [-0.1, 0.1)."""
    sys.path.insert(0, ROOT)
    from oracle.hashinit import hash_uniform
    out = {}
    for key, shape in named_shapes:
        shape = tuple(int(s) for s in shape)
        u = hash_uniform(key, int(np.prod(shape))) * 2.0 - 1.0
        if _is_norm(key) and key.endswith("weight"):
            v = 1.0 + 0.5 * u
        elif key.endswith("bias"):
            v = 0.1 * u
        else:
            fan_in = 9 if key.startswith(("linear.", "rc_linear.")) else int(np.prod(shape[1:]))
            v = u * np.sqrt(3.0 / fan_in)
        out[key] = torch.from_numpy(v.astype(np.float32).reshape(shape))
    return out


def make_batch(c, seed):
    """ids [B, L] in 0..4 with runs of 4 (N: left padding and an inner run), labels [B]."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 4, size=(c["B"], c["L"]))
    for b in range(c["B"]):
        ids[b, :3 + 7 * b] = 4
        s = int(rng.integers(20, c["L"] - 20))
        ids[b, s:s + 5 + b] = 4
    ids[0, -1] = 4
    labels = rng.integers(0, 2, size=(c["B"],))
    return ids.astype(np.int64), labels.astype(np.int64)


class _StandInClass(type):
    def __getattr__(cls, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _StandInClass(k, (), {})

    def __call__(cls, *a, **k):
        if len(a) == 1 and callable(a[0]) and not k:  # used as a decorator
            return a[0]
        return super().__call__()


class _StandInModule(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _StandInClass(k, (), {})


WANTED = ("flash_attn", "timm", "fftconv")


class _AbsentPackages(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Last on sys.meta_path: asked only for what nothing else found."""

    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in WANTED:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _StandInModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, m):
        pass


def _reference_cnn():
    sys.meta_path.append(_AbsentPackages())
    for name in ("src", "src.models", "src.models.sequence", "src.models.sequence.convNext"):
        m = _StandInModule(name)  # the package __init__ files import the whole model zoo
        m.__path__ = []
        sys.modules[name] = m
    spec = importlib.util.spec_from_file_location(
        "ref_denoise", os.path.join(REF, "src/models/sequence/denoise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CNNModel


def main():
    CNNModel = _reference_cnn()
    torch.set_num_threads(8)
    pick = np.random.default_rng(7)
    res = {}
    for tag, c in CONFIGS.items():
        ids, labels = make_batch(c, 100 + ord(tag))
        res[f"{tag}/ids"], res[f"{tag}/labels"] = ids.astype(np.int8), labels
        res[f"{tag}/config"] = np.bytes_(json.dumps(c))
        for prec in ("32", "bf16"):
            m = CNNModel(**model_kwargs(c)).eval()
            keys = [(k, list(v.shape)) for k, v in m.state_dict().items()]
            res[f"{tag}/keys"] = np.bytes_(json.dumps(keys))
            sd = denoise_state(keys + [(DECODER_KEYS[0], (2, c["D"])), (DECODER_KEYS[1], (2,))])
            dec = torch.nn.Linear(c["D"], 2)
            with torch.no_grad():
                dec.weight.copy_(sd.pop(DECODER_KEYS[0]))
                dec.bias.copy_(sd.pop(DECODER_KEYS[1]))
            m.load_state_dict(sd, strict=True)
            with torch.autocast("cpu", dtype=torch.bfloat16, enabled=prec == "bf16"):
                feat, _ = m(torch.as_tensor(ids))
                logits = dec(feat.mean(dim=1))  # SequenceDecoder mode pool, l_output 0
                loss = F.cross_entropy(logits.float(), torch.as_tensor(labels))
            loss.backward()
            f = feat.detach()
            res[f"{tag}/feat{prec}"] = (f.view(torch.int16).numpy().view(np.uint16)
                                        if f.dtype == torch.bfloat16 else f.float().numpy())
            res[f"{tag}/logits{prec}"] = logits.detach().float().numpy()
            res[f"{tag}/loss{prec}"] = np.float64(loss.item())
            named = list(m.named_parameters()) + [(DECODER_KEYS[0], dec.weight),
                                                  (DECODER_KEYS[1], dec.bias)]
            for n, p in named:
                g = p.grad.detach().float().reshape(-1).numpy()
                if prec == "32":
                    k = min(N_SAMPLE, g.size)
                    res[f"{tag}/gidx/{n}"] = np.sort(pick.choice(g.size, k, replace=False)).astype(
                        np.uint16 if g.size <= 65536 else np.int32)
                res[f"{tag}/gradnorm{prec}/{n}"] = np.float64(np.linalg.norm(g.astype(np.float64)))
                res[f"{tag}/gs{prec}/{n}"] = g[res[f"{tag}/gidx/{n}"].astype(np.int64)]
            print(f"denoise_cnn {tag}: precision {prec}, feat {tuple(feat.shape)} {feat.dtype}, "
                  f"loss {loss.item():.6f}")
    path = os.path.join(HERE, "denoise_cnn.npz")
    np.savez_compressed(path, **res)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
