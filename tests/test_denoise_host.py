"""Host-side checks of the gated dilated-CNN backbone (dna_amd/denoise.py) and what was built
around it: the module tree against the reference's recorded state-dict keys, the options that
are not built, the one-hot id remap of the three character-level loaders, the three experiments,
and the new C entry points' argument checks (nothing here launches a kernel)."""
import ctypes
import gzip
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

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


@pytest.mark.parametrize("tag", ["A", "B"])
def test_state_dict_keys_and_shapes_are_the_references(tag):
    from dna_amd.denoise import CNNModel
    m = CNNModel(**MK.model_kwargs(MK.CONFIGS[tag]))
    ours = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    ref = json.loads(Z[f"{tag}/keys"].tobytes().decode())
    assert sorted(ours) == sorted(ref)
    assert m.d_output == MK.CONFIGS[tag]["D"]
    # a same-key state dict loads strictly, and the dilations follow the reference's ladder
    m.load_state_dict(MK.denoise_state(ref), strict=True)
    d = MK.CONFIGS[tag]["dilation"]
    assert [c.dilation[0] for c in m.convs] == [1, 1, d, d ** 2, d ** 3][:len(m.convs)]
    assert [c.padding[0] for c in m.gates] == [(MK.CONFIGS[tag]["k"] - 1) // 2 * c.dilation[0]
                                               for c in m.gates]


def test_stacks_repeat_each_layer_and_optional_modules():
    from dna_amd.denoise import CNNModel
    kw = MK.model_kwargs(MK.CONFIGS["A"])
    kw["args"].num_cnn_stacks = 2
    kw.update(num_conv1d=3, mlp=False, final_conv=True)
    m = CNNModel(**kw)
    assert [c.dilation[0] for c in m.convs] == [1, 1, 1, 1, 4, 4] and m.num_layers == 6
    keys = set(m.state_dict())
    assert not any(k.startswith("milinear") for k in keys)
    assert {"final_conv.0.weight", "final_conv.2.bias", "norms.5.weight", "rc_norms.5.bias"} <= keys
    assert tuple(m.final_conv[0].weight.shape) == (64, 64, 1)


@pytest.mark.parametrize("change,name", [
    (dict(mode="up_down"), "up_down"), (dict(mode="convnext"), "convnext"),
    (dict(mode="pure_gate"), "pure_gate"), (dict(mode="dirichlet"), "dirichlet"),
    (dict(cls_free_guidance=True), "cls_free_guidance"), (dict(clean_data=True), "clean_data"),
    (dict(hidden_dim=96), "hidden_dim"), (dict(hidden_dim=576), "hidden_dim"),
    (dict(pretrain=True), "pretrain"), (dict(classifier=True), "classifier"),
    (dict(use_outlinear=True), "use_outlinear"), (dict(for_representation=False), "for_representation"),
    (dict(kernel_size=11), "kernel_size"), (dict(kernel_size=4), "kernel_size"),
    (dict(num_conv1d=6), "num_conv1d"), (dict(dilation=0), "dilation")])
def test_out_of_scope_options_raise_naming_the_option(change, name):
    from dna_amd.denoise import CNNModel
    kw = MK.model_kwargs(MK.CONFIGS["A"])
    for k, v in change.items():
        if hasattr(kw["args"], k):
            setattr(kw["args"], k, v)
        else:
            kw[k] = v
    with pytest.raises(NotImplementedError, match=name):
        CNNModel(**kw)


def test_forward_has_no_cpu_path():
    from dna_amd.denoise import CNNModel
    m = CNNModel(**MK.model_kwargs(MK.CONFIGS["A"]))
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 16, dtype=torch.int64))


# ------------------------------------------------------------------------------------ loaders
SEQS = ["ACGTNACGT", "TTGACN", "NNACGTACGTACGTAC", "G"]
ML = 12


def _tok():
    from dna_amd.tokenizer import CharacterTokenizer
    return CharacterTokenizer(["A", "C", "G", "T", "N"], ML + 2, padding_side="left")


def _expected(seq):
    """Left-padded, truncated to ML: A C G T = 0..3, N and padding = 4."""
    return [4] * max(0, ML - len(seq)) + ["ACGTN".index(c) for c in seq[:ML]]


def _check_pair(make):
    plain, remapped = make({}), make(dict(id_remap=True))
    ids_t = torch.stack([plain[i][0] for i in range(len(plain))])
    ids_r = torch.stack([remapped[i][0] for i in range(len(remapped))])
    tok = _tok()
    want = [tok(s, add_special_tokens=False, padding="max_length", max_length=ML,
                truncation=True)["input_ids"] for s in SEQS]
    assert ids_t.tolist() == want                                   # tokenizer ids: as before
    rule = ids_t - 7
    rule[(rule >= 4) | (rule < 0)] = 4
    assert torch.equal(ids_r, rule) and ids_r.tolist() == [_expected(s) for s in SEQS]
    return remapped


def test_genomic_benchmark_id_remap(tmp_path):
    from dna_amd.finetune_data import GenomicBenchmarkFolder
    for i, s in enumerate(SEQS):
        d = tmp_path / "toy" / "train" / ("a" if i < 2 else "b")
        d.mkdir(parents=True, exist_ok=True)
        (d / f"{i}.txt").write_text(s)
    make = lambda kw: GenomicBenchmarkFolder(tmp_path, "toy", "train", ML, tokenizer=_tok(), **kw)
    _check_pair(make)
    ds = make(dict(use_tokenizer=False, return_mask=True))           # the reference's spelling
    ids, label, mask = ds[3]
    assert ids.tolist() == _expected("G") and int(label) == 1
    assert mask.tolist() == [False] * (ML - 1) + [True]              # from the tokenizer's padding


def test_deepstarr_id_remap(tmp_path):
    from dna_amd.finetune_data import DeepSTARRFolder
    with open(tmp_path / "Sequences_Train.fa", "w") as f:
        for i, s in enumerate(SEQS):
            f.write(f">s{i}\n{s}\n")
    with open(tmp_path / "Sequences_activity_Train.txt", "w") as f:
        f.write("Dev_log2_enrichment\tHk_log2_enrichment\n")
        for i in range(len(SEQS)):
            f.write(f"{i}.5\t-{i}.25\n")
    ds = _check_pair(lambda kw: DeepSTARRFolder(tmp_path, "train", ML, tokenizer=_tok(), **kw))
    assert ds[2][1].tolist() == [2.5, -2.25]


def test_deepsea_id_remap(tmp_path):
    from dna_amd.finetune_data import DEEPSEA_LABELS, DeepSEACsv
    with gzip.open(tmp_path / "train.csv.gz", "wt") as f:
        for i, s in enumerate(SEQS):
            f.write(s + "," + ",".join(str((i + j) % 2) for j in range(DEEPSEA_LABELS)) + "\n")
    make = lambda kw: DeepSEACsv(tmp_path, "train", ML, tokenizer=_tok(), **kw)
    _check_pair(make)
    assert make(dict(use_tokenizer=False))[0][0].tolist() == _expected(SEQS[0])


# ------------------------------------------------------------------------------------ experiments
EXPERIMENTS = ["genomic_benchmark_denoise", "deepstarr_denoise", "deepsea_denoise"]


@pytest.mark.parametrize("name", EXPERIMENTS)
def test_experiments_compose(name):
    from dna_amd.compose import compose
    cfg = compose(os.path.join(ROOT, "configs"), "config", [f"experiment=denoise/{name}"])
    m = cfg.model.to_container()
    assert m["_name_"] == "denoise_cnn" and m["kernel_size"] == 9 and m["dilation"] == 4
    assert m["args"]["mode"] == "dilation" and m["args"]["hidden_dim"] == 128
    assert m["length"] == cfg.dataset.max_length
    assert cfg.dataset.use_tokenizer is False and cfg.decoder.mode == "pool"


@pytest.mark.parametrize("name", EXPERIMENTS)
def test_finetune_dry_run(name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--dry-run",
                        f"experiment=denoise/{name}"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["dry_run"] and info["model"] == "denoise_cnn" and info["model_params"] > 1_600_000


def test_pretrained_state_dicts_load_strictly():
    """train.pretrained_model_path: a reference-layout checkpoint (model.<backbone key>, its own
    decoder.* keys dropped, head fresh) and one of finetune.py's own (everything)."""
    import finetune
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.denoise import CNNModel
    c = MK.CONFIGS["A"]
    keys = json.loads(Z["A/keys"].tobytes().decode())
    sd = MK.denoise_state(keys)
    clf = SequenceClassifier(CNNModel(**MK.model_kwargs(c)), 2, mode="pool")
    head = clf.decoder[0].output_transform.weight.detach().clone()
    ref_ckpt = {"model." + k: v for k, v in sd.items()}
    ref_ckpt["decoder.0.output_transform.weight"] = torch.zeros(2, c["D"])
    info = finetune.load_pretrained(clf, ref_ckpt)
    assert info["loaded"] == "backbone"
    assert torch.equal(clf.model.convs[3].weight, sd["convs.3.weight"])
    assert torch.equal(clf.decoder[0].output_transform.weight, head)
    with pytest.raises(RuntimeError, match="Missing key"):
        finetune.load_pretrained(clf, {k: v for k, v in ref_ckpt.items() if "gates.1" not in k})
    own = {"model." + k: v.clone() for k, v in clf.state_dict().items()}  # Lightning layout
    clf2 = SequenceClassifier(CNNModel(**MK.model_kwargs(c)), 2, mode="pool")
    assert finetune.load_pretrained(clf2, own) == {"loaded": "classifier"}
    for k, v in clf.state_dict().items():
        assert torch.equal(clf2.state_dict()[k], v), k


# ------------------------------------------------------------------------------------ C ABI
NEW_SYMBOLS = ["dna_dconv_fwd", "dna_dconv_bwd_elem", "dna_dconv_wgrad", "dna_dconv_wgrad_splits",
               "dna_dconv_wgrad_workspace", "dna_onehot_conv_fwd", "dna_onehot_conv_bwd",
               "dna_onehot_conv_bwd_workspace"]


def test_new_symbols_are_declared_exported_and_counted():
    from dna_amd import _native as N
    L = N.lib()
    declared = N.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in N._SIGS and hasattr(L, s), s
    assert L.dna_abi_version() == 1 and L.dna_abi_revision() >= 4
    from dna_amd import ops
    for name in ("dconv_fwd", "dconv_bwd_elem", "dconv_wgrad", "onehot_conv_fwd",
                 "onehot_conv_bwd"):
        assert name in ops.OPS and hasattr(torch.ops.dna_amd, name)


def test_bad_arguments_are_invalid_before_anything_is_launched():
    """Bad C / K / dilation / dtype and null pointers: DNA_ERR_INVALID with a message. The
    pointers are never dereferenced on the host, so small fake addresses stand in for buffers."""
    from dna_amd import _native as N
    L = N.lib()
    P = ctypes.c_void_p(4096)

    def fwd(x=P, dtype=N.BF16, w=P, B=2, Ln=96, C=64, K=9, d=4, epi=N.DCONV_PLAIN, out=P, g=None,
            res=None, z=None, res_out=None):
        return L.dna_dconv_fwd(x, dtype, w, None, B, Ln, C, K, d, epi, N.ACT_NONE, g, res, out, z,
                               res_out, None)

    bad = [dict(C=96), dict(C=32), dict(C=576), dict(K=4), dict(K=11), dict(d=0), dict(x=None),
           dict(w=None), dict(out=None), dict(dtype=N.F16), dict(B=0), dict(B=70000), dict(Ln=0),
           dict(epi=7), dict(epi=N.DCONV_GATE), dict(epi=N.DCONV_MAIN_MUL, g=P, res=P, res_out=P),
           dict(x=ctypes.c_void_p(4100))]
    for kw in bad:
        assert fwd(**kw) == 1, kw
        assert b"dna_dconv_fwd" in L.dna_last_error(), kw
    assert L.dna_dconv_bwd_elem(None, None, P, P, None, N.F32, 256, 1, P, P, None) == 1
    assert L.dna_dconv_bwd_elem(P, None, P, P, None, N.F32, 258, 1, P, P, None) == 1    # n % 4
    assert L.dna_dconv_bwd_elem(P, None, P, None, None, N.F32, 256, 1, P, P, None) == 1  # forget: g
    assert L.dna_dconv_bwd_elem(P, None, P, P, None, N.F32, 256, 0, P, P, None) == 1    # gelu: z_g
    assert L.dna_dconv_wgrad_splits(2, 96, 96, 9) == 0 and L.dna_dconv_wgrad_splits(2, 96, 64, 9) >= 1
    assert L.dna_dconv_wgrad_workspace(2, 96, 64, 9) >= 4 * (9 * 64 * 64 + 64)
    ws = L.dna_dconv_wgrad_workspace(2, 96, 64, 9)
    assert L.dna_dconv_wgrad(P, P, N.BF16, 2, 96, 96, 9, 4, P, P, 0, P, 1 << 30, None) == 1
    assert L.dna_dconv_wgrad(P, P, N.BF16, 2, 96, 64, 9, 4, P, P, 0, P, ws - 4, None) == 1
    assert L.dna_dconv_wgrad(P, None, N.BF16, 2, 96, 64, 9, 4, P, P, 0, P, ws, None) == 1
    assert b"dna_dconv_wgrad" in L.dna_last_error()
    assert L.dna_onehot_conv_fwd(P, P, P, 2, 96, 96, 5, 9, 0, N.ACT_GELU, P, None) == 1
    assert L.dna_onehot_conv_fwd(P, P, P, 2, 96, 64, 9, 9, 0, N.ACT_GELU, P, None) == 1  # V > 8
    assert L.dna_onehot_conv_fwd(P, P, P, 2, 96, 64, 5, 8, 0, N.ACT_GELU, P, None) == 1  # even KW
    assert L.dna_onehot_conv_fwd(None, P, P, 2, 96, 64, 5, 9, 0, N.ACT_GELU, P, None) == 1
    assert L.dna_onehot_conv_bwd_workspace(2, 96, 96, 5, 9) == 0
    assert L.dna_onehot_conv_bwd(P, P, P, P, 2, 96, 64, 5, 9, 0, N.ACT_GELU, P, P, 0, P, 16,
                                 None) == 1
    assert b"dna_onehot_conv_bwd" in L.dna_last_error()


def test_shadow_copy_is_not_read_once_the_parameter_moved_on():
    """functional._shadow: the trainer's bf16 copy stands for the parameter only at the version
    the trainer stamped; after an in-place change outside the optimizer step the parameter itself
    is cast."""
    from dna_amd import functional as DF
    w = torch.nn.Parameter(torch.full((4, 4, 3), 1.0))
    w._dna_lp = torch.full((4, 4, 3), 1.0, dtype=torch.bfloat16)
    w._dna_lp_version = w._version
    assert DF._shadow(w, torch.bfloat16) is w._dna_lp
    with torch.no_grad():
        w.mul_(2.0)
    got = DF._shadow(w, torch.bfloat16)
    assert got is not w._dna_lp and float(got[0, 0, 0]) == 2.0
    del w._dna_lp_version  # a copy nobody vouched for is not read either
    assert DF._shadow(w, torch.bfloat16) is not w._dna_lp
    taps = DF.conv_taps(torch.arange(24.).reshape(2, 4, 3)[:, :2], torch.float32)
    assert taps.shape == (3, 2, 2) and float(taps[2, 1, 0]) == 14.0     # [t][co][ci] = W[co, ci, t]
    back = DF.conv_taps_dgrad(torch.arange(24.).reshape(2, 4, 3)[:, :2], torch.float32)
    assert float(back[0, 1, 0]) == 5.0                                   # [t][ci][co] = W[co, ci, K-1-t]
