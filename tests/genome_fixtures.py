"""Helpers of the genome-window tests: the golden fixtures (tests/golden/species_golden.json,
chromatin_golden.json; the reference's own outputs) written out as the folders the datasets
read."""
import gzip
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def species_folder(root, gold=None):
    """<root>/<species>/chr*.{fna,fa,fna.gz}: the suffix cycles, so all three are read."""
    gold = gold or load("species_golden.json")
    for n, (rel, text) in enumerate(sorted(gold["fasta"].items())):
        path = os.path.join(str(root), rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if n % 3 == 1:
            path = path[:-len(".fna")] + ".fa"
        if n % 3 == 2:
            with gzip.open(path + ".gz", "wt") as f:
                f.write(text)
        else:
            with open(path, "w") as f:
                f.write(text)
    return gold


def chromatin_folder(root, gold=None, gz=False, splits=("train", "val", "test")):
    """<root>/genome.fa[.gz] and <root>/<split>_<version>_coords_targets.csv (every split the
    fixture's one table). -> (gold, genome path)."""
    gold = gold or load("chromatin_golden.json")
    fa = os.path.join(str(root), "genome.fa" + (".gz" if gz else ""))
    with (gzip.open(fa, "wt") if gz else open(fa, "w")) as f:
        f.write(gold["fasta"])
    for split in splits:
        with open(os.path.join(str(root), f"{split}_{gold['version']}_coords_targets.csv"),
                  "w") as f:
            f.write(gold["csv"])
    return gold, fa
