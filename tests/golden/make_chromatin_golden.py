#!/usr/bin/env python
"""tests/golden/chromatin_golden.json: the reference's ChromatinProfileDataset
(src/dataloaders/datasets/chromatin_profile_dataset.py, loaded by path, never copied) run on a
small synthetic genome and coordinates table.

    DNA_REFERENCE=<reference checkout> python tests/golden/make_chromatin_golden.py

Stand-ins, as in make_golden.py: `pyfaidx.Fasta` is a dict of str-backed records parsed from the
FASTA file this script writes into a temporary folder, `liftover` is an empty module (no
coordinates are lifted: the table is named for the genome version it is read with), and the
tokenizer is the project's CharacterTokenizer, built as genomics.py:464-468 builds the
reference's (tests/golden/make_char_golden.py pins the two against each other).

Three records of 1,300-2,500 bp (with N and lower-case runs), nine rows -- windows at both ends
of a chromosome, an interval of 901 bases (grows, odd base to the right) and one of 1,200 (cut)
-- seven y_ columns and a leading index column as a saved table has, max_length 512, 1000, 1024
and 1100. The script asserts that rows padded on the left only, on the right only and not at all
occur. The fixture holds the FASTA text, the CSV text and, per max_length, the reference's
windows (tokenizer=None), ids and targets.
"""
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DNA_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from dna_amd.tokenizer import CharacterTokenizer  # noqa: E402

MAX_LENGTHS = (512, 1000, 1024, 1100)
LENGTHS = {"chr1": 1300, "chr2": 1777, "chr3": 2500}
N_TARGETS = 7


class _Record(str):
    """Slicing gives a str; pyfaidx gives a Sequence whose str() is the slice."""


class Fasta(dict):
    def __init__(self, path):
        super().__init__()
        name, parts = None, []
        with open(path) as f:
            for line in f.read().splitlines() + [">"]:
                if line.startswith(">"):
                    if name is not None:
                        self[name] = _Record("".join(parts))
                    name, parts = line[1:].split()[0] if line[1:].split() else None, []
                else:
                    parts.append(line.strip())


def load_reference():
    pf = types.ModuleType("pyfaidx")
    pf.Fasta = Fasta
    sys.modules["pyfaidx"] = pf
    sys.modules["liftover"] = types.ModuleType("liftover")
    spec = importlib.util.spec_from_file_location(
        "ref_chromatin_profile_dataset",
        os.path.join(REF, "src/dataloaders/datasets/chromatin_profile_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic_record(rng, n):
    s = [rng.choice("ACGT") for _ in range(n)]
    for _ in range(3):
        a, k = rng.randrange(0, n - 30), rng.randint(3, 25)
        s[a:a + k] = "N" * k
    for _ in range(3):
        b = rng.randrange(0, n - 200)
        for i in range(b, b + rng.randint(20, 200)):
            s[i] = s[i].lower()
    return "".join(s)


def main():
    ref = load_reference()
    rng = random.Random(919)
    records = {k: synthetic_record(rng, n) for k, n in LENGTHS.items()}
    fasta = "".join(f">{k} synthetic\n" + "\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n"
                    for k, s in records.items())
    coords = [(0, 0, 1000), (0, 300, 1300), (0, 150, 1150), (1, 0, 1000), (1, 777, 1777),
              (1, 400, 1301), (2, 600, 1800), (2, 30, 1030), (2, 1480, 2480)]
    header = ["", "Chr_No", "Start", "End"] + [f"y_{i}" for i in range(N_TARGETS)]
    lines = [",".join(header)]
    for i, (c, s, e) in enumerate(coords):
        lines.append(",".join([str(i), str(c), str(s), str(e)]
                              + [str(rng.randint(0, 1)) for _ in range(N_TARGETS)]))
    table = "\n".join(lines) + "\n"
    out = {"fasta": fasta, "csv": table, "version": "hg38", "split": "train", "cases": {}}
    kinds = set()
    with tempfile.TemporaryDirectory() as tmp:
        fa, path = os.path.join(tmp, "genome.fa"), os.path.join(tmp, "train_hg38_coords_targets.csv")
        with open(fa, "w") as f:
            f.write(fasta)
        with open(path, "w") as f:
            f.write(table)
        for ml in MAX_LENGTHS:
            tok = CharacterTokenizer(["A", "C", "G", "T", "N"], ml + 2)
            kw = dict(max_length=ml, ref_genome_path=fa, ref_genome_version="hg38",
                      coords_target_path=path, use_padding=True)
            raw = ref.ChromatinProfileDataset(tokenizer=None, **kw)
            ds = ref.ChromatinProfileDataset(tokenizer=tok, tokenizer_name="char", **kw)
            assert len(ds) == len(coords)
            windows = [raw[i][0] for i in range(len(raw))]
            for w in windows:
                left, right = len(w) - len(w.lstrip(".")), len(w) - len(w.rstrip("."))
                kinds.add(("left" if left else "") + ("right" if right else "") or "none")
            items = [ds[i] for i in range(len(ds))]
            out["cases"][str(ml)] = {"windows": windows, "ids": [x.tolist() for x, _ in items],
                                     "targets": [y.tolist() for _, y in items]}
            print(f"max_length {ml}: item lengths {sorted({len(x) for x, _ in items})}")
    assert {"left", "right", "none"} <= kinds, kinds
    dest = os.path.join(HERE, "chromatin_golden.json")
    with open(dest, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"{dest}: kinds {sorted(kinds)}, {os.path.getsize(dest)} bytes")


if __name__ == "__main__":
    main()
