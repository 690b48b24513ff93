#!/usr/bin/env python
"""tests/golden/species_golden.json and species_splits.json: the reference's SpeciesDataset
(src/dataloaders/datasets/species_dataset.py, loaded by path, never copied) run on small synthetic
genomes, and its chromosome table.

    DNA_REFERENCE=<reference checkout> python tests/golden/make_species_golden.py

Stand-ins, as in make_golden.py: `pyfaidx.Fasta` is a small class over the FASTA files this script
writes into a temporary folder (one record per file; it honours sequence_always_upper, len() and
slicing, and logs how many bases each slice returned), and the module the reference imports its
tokenizer from is the project's CharacterTokenizer (the reference's own cannot be constructed
under this transformers version; tests/golden/make_char_golden.py pins the two against each
other). The reference draws from the global `random`: it is seeded per case.

Two species (mouse, hippo), chromosomes of 150-400 bp with an N run and a lower-case run,
max_length 64, 64 items for every combination of add_eos x remove_tail_ends on the train split,
and one case on the test split (cutoff_test). Per case the seed is searched until the reference's
own output holds at least one partly-N-padded row and one all-N row. The fixture holds the FASTA
texts, the cases with their seeds, and the expected ids and targets.
"""
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DNA_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from dna_amd.tokenizer import CharacterTokenizer  # noqa: E402

SPECIES = ["mouse", "hippo"]
MAX_LENGTH, ITEMS = 64, 64
SLICES = []  # bases returned by every slice of a record, in call order


class _Record:
    def __init__(self, seq):
        self.seq = seq

    def __len__(self):
        return len(self.seq)

    def __getitem__(self, key):
        out = self.seq[key]
        SLICES.append(len(out))
        return out


class Fasta:
    """One-record FASTA file -> fasta[0] is the record."""

    def __init__(self, path, sequence_always_upper=False):
        with open(path) as f:
            lines = f.read().splitlines()
        seq = "".join(l.strip() for l in lines if not l.startswith(">"))
        self.records = [_Record(seq.upper() if sequence_always_upper else seq)]

    def __getitem__(self, i):
        return self.records[i]

    def __len__(self):
        return len(self.records[0])

    def close(self):
        pass


def load_reference():
    pf = types.ModuleType("pyfaidx")
    pf.Fasta = Fasta
    sys.modules["pyfaidx"] = pf
    for name in ("src", "src.dataloaders", "src.dataloaders.datasets"):
        sys.modules.setdefault(name, types.ModuleType(name))
    tok = types.ModuleType("src.dataloaders.datasets.hg38_char_tokenizer")
    tok.CharacterTokenizer = CharacterTokenizer
    sys.modules[tok.__name__] = tok
    spec = importlib.util.spec_from_file_location(
        "ref_species_dataset", os.path.join(REF, "src/dataloaders/datasets/species_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic_chromosome(rng):
    n = rng.randint(150, 400)
    s = [rng.choice("ACGT") for _ in range(n)]
    a, k = rng.randrange(0, n - 20), rng.randint(3, 15)
    s[a:a + k] = "N" * k
    b = rng.randrange(0, n - 40)
    for i in range(b, b + rng.randint(5, 40)):
        s[i] = s[i].lower()
    return "".join(s)


def main():
    ref = load_reference()
    table = ref.SPECIES_CHROMOSOME_SPLITS
    with open(os.path.join(HERE, "species_splits.json"), "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    rng = random.Random(4242)
    fasta = {}
    for spec in SPECIES:
        for split in ("train", "valid", "test"):
            for chrom in table[spec][split]:
                seq = synthetic_chromosome(rng)
                wrapped = "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60))
                fasta[f"{spec}/chr{chrom}.fna"] = f">chr{chrom} synthetic {spec}\n{wrapped}\n"
    tok = CharacterTokenizer(["A", "C", "G", "T", "N"], MAX_LENGTH + 2)
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for rel, text in fasta.items():
            os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
            with open(os.path.join(tmp, rel), "w") as f:
                f.write(text)
        combos = [("train", e, r) for e in (False, True) for r in (False, True)]
        combos.append(("test", True, True))
        for split, add_eos, tails in combos:
            for seed in range(10000):
                ds = ref.SpeciesDataset(species=SPECIES, species_dir=tmp, split=split,
                                        max_length=MAX_LENGTH, total_size=ITEMS, tokenizer=tok,
                                        tokenizer_name="char", add_eos=add_eos,
                                        task="species_classification", remove_tail_ends=tails,
                                        cutoff_train=0.1, cutoff_test=0.2)
                random.seed(seed)
                del SLICES[:]
                items = [ds[i] for i in range(len(ds))]
                if 0 in SLICES and any(0 < n < MAX_LENGTH for n in SLICES):
                    break
            else:
                raise AssertionError("no seed gives a partly padded and an all-N row")
            ids = torch.stack([x for x, _ in items])
            n_id = tok("N", add_special_tokens=False)["input_ids"][0]
            assert any(bool((row == n_id).all()) for row in ids), "no all-N row"
            assert len(SLICES) == ITEMS
            cases.append({"split": split, "add_eos": add_eos, "remove_tail_ends": tails,
                          "seed": seed, "bases_read": list(SLICES), "ids": ids.tolist(),
                          "targets": [int(t) for _, t in items]})
            print(f"{split} add_eos={add_eos} remove_tail_ends={tails}: seed {seed}, "
                  f"{SLICES.count(0)} all-N rows, "
                  f"{sum(0 < n < MAX_LENGTH for n in SLICES)} partly padded, ids {tuple(ids.shape)}")
    out = os.path.join(HERE, "species_golden.json")
    with open(out, "w") as f:
        json.dump({"species": SPECIES, "max_length": MAX_LENGTH, "total_size": ITEMS,
                   "cutoff_train": 0.1, "cutoff_test": 0.2, "fasta": fasta, "cases": cases}, f,
                  separators=(",", ":"))
        f.write("\n")
    print(f"{out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
