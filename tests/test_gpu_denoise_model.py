"""The gated dilated-CNN backbone (dna_amd/denoise.py) under SequenceClassifier against the
reference's CNNModel + pool decoder, as recorded by tests/golden/make_denoise_golden.py
(denoise_cnn.npz: configurations A -- D 64, k 9, dilations 1, 1, 4, 16, 64 at L 96, forget -- and
B -- D 128, k 5, dilations 1, 1, 3, 9 at L 200, add, complemented gate input), with the weights
rebuilt from the same hash.

  fp32   feat, logits and loss within 1e-3 (this project's fp32 parity bound); per parameter the
         sampled gradient elements within 1e-3 relative L2 and the gradient norm within 1e-3.
  bf16   the rule of test_gpu_model.test_bf16_train_step_vs_reference_fixture, through
         SeqClsTrainer under autocast: whatever bf16 costs the reference, ours may cost at most
         twice that -- logits max / rms error <= 2x the reference's own bf16-vs-fp32 error,
         gradients <= 2x its error + 5e-3, loss <= 2x its error + 1e-3.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _maker():
    spec = importlib.util.spec_from_file_location(
        "make_denoise_golden", os.path.join(GOLDEN, "make_denoise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _maker()
Z = np.load(os.path.join(GOLDEN, "denoise_cnn.npz"))


def _classifier(tag):
    """SequenceClassifier(CNNModel) of configuration `tag` with the fixture's hashed weights, and
    the fixture's batch on the device."""
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.denoise import CNNModel
    c = MK.CONFIGS[tag]
    keys = json.loads(Z[f"{tag}/keys"].tobytes().decode())
    sd = MK.denoise_state(keys + [(MK.DECODER_KEYS[0], (2, c["D"])), (MK.DECODER_KEYS[1], (2,))])
    clf = SequenceClassifier(CNNModel(**MK.model_kwargs(c)), 2, mode="pool")
    clf.load_state_dict({(k if k.startswith("decoder.") else "model." + k): v
                         for k, v in sd.items()}, strict=True)
    ids = torch.as_tensor(Z[f"{tag}/ids"].astype(np.int64), device=DEV)
    labels = torch.as_tensor(Z[f"{tag}/labels"], device=DEV)
    return clf, ids, labels


def _fixture_name(n):
    return n[len("model."):] if n.startswith("model.") else n


def _feat_bf16(tag):
    f = Z[f"{tag}/featbf16"]
    if f.dtype == np.uint16:
        f = torch.from_numpy(f.view(np.int16).copy()).view(torch.bfloat16).float().numpy()
    return f


def _ban_libraries(mp):
    """DNA_STRICT_NATIVE=1 (every counted fallback raises LibraryFallbackError) and every torch
    convolution / GEMM entry point raises."""
    mp.setenv("DNA_STRICT_NATIVE", "1")

    def banned(name):
        def f(*a, **k):
            raise AssertionError(f"library call torch.{name} in the denoise_cnn hot path")
        return f
    for name in ("mm", "addmm", "bmm", "baddbmm", "matmul", "einsum", "conv1d", "conv2d",
                 "convolution", "conv_transpose1d"):
        mp.setattr(torch, name, banned(name))
    for name in ("linear", "conv1d", "conv2d"):
        mp.setattr(torch.nn.functional, name, banned("nn.functional." + name))
    mp.setattr(torch.Tensor, "__matmul__", banned("Tensor.__matmul__"))


@pytest.mark.parametrize("tag", ["A", "B"])
def test_fp32_forward_and_gradients_vs_reference_fixture(tag, monkeypatch):
    clf, ids, labels = _classifier(tag)
    clf = clf.to(DEV).eval()
    with monkeypatch.context() as mp:
        _ban_libraries(mp)
        feat, _ = clf.model(ids)
        loss, logits = clf(ids, labels)
        loss.backward()
    f32, l32 = Z[f"{tag}/feat32"], Z[f"{tag}/logits32"]
    ferr = float(np.abs(feat.detach().float().cpu().numpy() - f32).max())
    lerr = float(np.abs(logits.detach().float().cpu().numpy() - l32).max())
    print(f"denoise {tag} fp32: feat err {ferr:.3e} (max |feat| {np.abs(f32).max():.3f}), "
          f"logits err {lerr:.3e}, loss {loss.item():.6f} vs {float(Z[f'{tag}/loss32']):.6f}")
    assert feat.dtype == torch.float32 and tuple(feat.shape) == f32.shape
    assert ferr <= 1e-3 and lerr <= 1e-3
    assert abs(loss.item() - float(Z[f"{tag}/loss32"])) <= 1e-3
    worst = (0.0, None)
    for n, p in clf.named_parameters():
        k = _fixture_name(n)
        assert p.grad is not None, n
        g = p.grad.detach().reshape(-1).cpu().numpy().astype(np.float64)
        g32 = Z[f"{tag}/gs32/{k}"].astype(np.float64)
        rel = np.linalg.norm(g[Z[f"{tag}/gidx/{k}"].astype(np.int64)] - g32) / np.linalg.norm(g32)
        worst = max(worst, (float(rel), n))
        assert rel <= 1e-3, (n, rel)
        gn, rn = float(np.linalg.norm(g)), float(Z[f"{tag}/gradnorm32/{k}"])
        assert abs(gn - rn) <= 1e-3 * rn, (n, gn, rn)
    print(f"denoise {tag} fp32: worst sampled-gradient relative L2 {worst[0]:.3e} ({worst[1]})")


@pytest.mark.parametrize("tag", ["A", "B"])
def test_bf16_train_step_vs_reference_fixture(tag):
    from dna_amd.trainer import SeqClsTrainer
    clf, ids, labels = _classifier(tag)
    tr = SeqClsTrainer(clf, torch.device(DEV), lr=1e-3, weight_decay=0.1, max_grad_norm=1.0,
                       autocast=torch.bfloat16)
    clf.eval()  # the fixture is eval mode (no dropout)
    logits, _, _ = tr.evaluate(ids, labels)
    clf.eval()
    logits = logits.float().cpu().numpy()
    l32, l16 = Z[f"{tag}/logits32"], Z[f"{tag}/logitsbf16"]
    ref_max, ref_rms = np.abs(l16 - l32).max(), np.sqrt(((l16 - l32) ** 2).mean())
    our_max, our_rms = np.abs(logits - l32).max(), np.sqrt(((logits - l32) ** 2).mean())
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        feat = clf.model(ids)[0].float().cpu().numpy()
    f32 = Z[f"{tag}/feat32"]
    print(f"denoise {tag} bf16: logits max {our_max:.3e} (reference {ref_max:.3e}), rms "
          f"{our_rms:.3e} ({ref_rms:.3e}); feat max err {np.abs(feat - f32).max():.3e} "
          f"(reference {np.abs(_feat_bf16(tag) - f32).max():.3e})")
    assert our_max <= 2 * ref_max, (our_max, ref_max)
    assert our_rms <= 2 * ref_rms, (our_rms, ref_rms)
    loss = tr.step(ids, labels)
    torch.cuda.synchronize()
    ref_loss_err = abs(float(Z[f"{tag}/lossbf16"]) - float(Z[f"{tag}/loss32"]))
    assert abs(loss.item() - float(Z[f"{tag}/loss32"])) <= 2 * ref_loss_err + 1e-3
    worst = (0.0, None, 0.0)
    for n, p in clf.named_parameters():
        k = _fixture_name(n)
        g = p.grad.detach().reshape(-1).cpu().numpy()
        g32, g16 = Z[f"{tag}/gs32/{k}"], Z[f"{tag}/gsbf16/{k}"]
        nref = np.linalg.norm(g32)
        err = np.linalg.norm(g[Z[f"{tag}/gidx/{k}"].astype(np.int64)] - g32) / nref
        ref_err = np.linalg.norm(g16 - g32) / nref
        worst = max(worst, (float(err - 2 * ref_err), n, float(err)))
        assert err <= 2 * ref_err + 5e-3, (n, err, ref_err)
    print(f"denoise {tag} bf16: largest (err - 2 ref_err) {worst[0]:.3e} at {worst[1]} "
          f"(err {worst[2]:.3e})")


def _toy_folder(root, n_per_class=24, length=48):
    """A separable Genomic Benchmarks folder: class a is A/C-rich, class b G/T-rich."""
    rng = np.random.default_rng(3)
    for split, n in (("train", n_per_class), ("test", 8)):
        for cls, rich in (("a", "AC"), ("b", "GT")):
            d = os.path.join(root, "toy", split, cls)
            os.makedirs(d)
            for i in range(n):
                seq = "".join(rng.choice(list(rich)) if rng.random() < 0.85 else rng.choice(list("ACGTN"))
                              for _ in range(length - int(rng.integers(0, 6))))
                with open(os.path.join(d, f"{i}.txt"), "w") as f:
                    f.write(seq)


def _small_classifier():
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.denoise import CNNModel
    kw = MK.model_kwargs(dict(MK.CONFIGS["A"], num_conv1d=3, k=5, dilation=2))
    kw["args"].dropout = 0.1
    torch.manual_seed(0)
    return SequenceClassifier(CNNModel(**kw), 2, mode="pool")


def test_training_on_a_toy_folder_evaluate_checkpoint_and_library_ban(tmp_path, monkeypatch):
    import finetune
    import train as T
    from dna_amd.finetune_data import GenomicBenchmarkFolder
    from dna_amd.trainer import SeqClsTrainer
    _toy_folder(str(tmp_path))
    train_ds = GenomicBenchmarkFolder(tmp_path, "toy", "train", 48, use_tokenizer=False)
    test_ds = GenomicBenchmarkFolder(tmp_path, "toy", "val", 48, use_tokenizer=False,
                                     classes=train_ds.classes)
    ids, labels = train_ds.collate([train_ds[i] for i in range(len(train_ds))])
    assert int(ids.max()) <= 4 and int(ids.min()) >= 0
    ids, labels = ids.to(DEV), labels.to(DEV)
    clf = _small_classifier()
    tr = SeqClsTrainer(clf, torch.device(DEV), lr=2e-3, weight_decay=0.0, max_grad_norm=1.0,
                       seed=1, autocast=torch.bfloat16)
    with monkeypatch.context() as mp:  # a full step and an eval forward with every library banned
        _ban_libraries(mp)
        losses = [tr.step(ids, labels).item()]
        assert bool(torch.isfinite(tr.evaluate(ids, labels)[0]).all())
    m0 = finetune.evaluate(tr, test_ds, 8, torch.device(DEV), 2)
    assert np.isfinite(losses[0]) and np.isfinite(m0["loss"]) and 0.0 <= m0["accuracy"] <= 1.0
    assert clf.training  # evaluate restores the training mode
    for _ in range(19):
        losses.append(tr.step(ids, labels).item())
    torch.cuda.synchronize()
    print("denoise toy losses:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    m1 = finetune.evaluate(tr, test_ds, 8, torch.device(DEV), 2)
    assert m1["loss"] < m0["loss"]
    # checkpoint: written in train.py's layout, read back by finetune.py's loader, strictly
    path = os.path.join(str(tmp_path), "last.ckpt")
    T.save_checkpoint(path, tr, 1)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    clf2 = _small_classifier()
    assert finetune.load_pretrained(clf2, ck["state_dict"]) == {"loaded": "classifier"}
    want = clf.state_dict()
    assert sorted(clf2.state_dict()) == sorted(want)
    for k, v in clf2.state_dict().items():
        assert torch.equal(v, want[k].cpu()), k
    # the same weights outside a trainer (bf16 from a cast) give the trainer's eval logits: the
    # trainer's bf16 copy is what a cast gives, and a forward never reads a stale one
    clf2 = clf2.to(DEV).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        _, l2 = clf2(ids, labels)
    l1 = tr.evaluate(ids, labels)[0]
    assert torch.equal(l1, l2)
    with torch.no_grad():
        clf.model.convs[0].weight.zero_()      # an edit behind the trainer's back ...
        clf2.model.convs[0].weight.zero_()
        clf.eval()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, l3 = clf(ids, labels)           # ... is seen by a forward outside trainer.step
            _, l4 = clf2(ids, labels)
        clf.train()
    assert torch.equal(l3, l4) and not torch.equal(l3, l1)


def test_library_arm_is_refused_under_strict_native(monkeypatch):
    """DNA_CONV_IMPL=torch (MIOpen, measurement only) counts as a library fallback."""
    from dna_amd.functional import LibraryFallbackError
    clf, ids, labels = _classifier("A")
    clf = clf.to(DEV).eval()
    monkeypatch.setenv("DNA_CONV_IMPL", "torch")
    with torch.no_grad():
        lib_feat = clf.model(ids)[0]
    assert float((lib_feat.cpu() - torch.from_numpy(Z["A/feat32"])).abs().max()) <= 1e-3
    monkeypatch.setenv("DNA_STRICT_NATIVE", "1")
    with pytest.raises(LibraryFallbackError):
        clf.model(ids)
