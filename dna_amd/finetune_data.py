"""Labelled-sequence data for fine-tuning: GUE-layout folders (the DNABERT-2 benchmark's
`train.csv` / `dev.csv` / `test.csv`, each row `sequence,label`), tokenised with the C++ BPE
tokenizer as [CLS] ... [SEP], truncated to max_length, padded per batch; and Genomic Benchmarks
folders (`<dest>/<name>/<split>/<class>/*.txt`, one sequence per file), tokenised per character
to a fixed length for the HyenaDNA / Caduceus classifiers; and, tokenised the same way, the
DeepSTARR files (two regression targets per sequence), the DeepSEA tables (919 0/1 labels) and the
Nucleotide Transformer benchmark's FASTA files (labels in the headers; NT_TASKS is its task
table)."""
import csv
import gzip
import os
import random

import torch

from .tokenizer import CharacterTokenizer, DNABertTokenizer

SPLITS = ("train", "dev", "test")


def _is_int(s):
    try:
        int(s)
        return True
    except ValueError:
        return False


def read_csv(path):
    """-> (sequences, int labels); a first row whose label is not an integer is a header."""
    seqs, labels = [], []
    with open(path, newline="") as f:
        for i, row in enumerate(csv.reader(f)):
            if len(row) < 2:
                continue
            if i == 0 and not _is_int(row[1].strip()):
                continue
            seqs.append(row[0].strip())
            labels.append(int(row[1]))
    return seqs, labels


class SequenceClassificationCSV(torch.utils.data.Dataset):
    """One split of a GUE-layout folder. Items are (ids int64 [n <= max_length], label); the whole
    split is tokenised once at construction (GUE splits are a few thousand short sequences)."""

    def __init__(self, data_dir, split="train", max_length=128, tokenizer=None):
        if split not in SPLITS:
            raise ValueError(f"split {split!r}: one of {SPLITS}")
        self.path = os.path.join(data_dir, f"{split}.csv")
        if not os.path.exists(self.path):
            raise FileNotFoundError(f"{self.path}: a GUE folder holds train.csv, dev.csv, test.csv")
        self.max_length = int(max_length)
        self.tokenizer = tokenizer or DNABertTokenizer()
        seqs, labels = read_csv(self.path)
        self.labels = torch.tensor(labels, dtype=torch.int64)
        self.ids = [torch.tensor(self.tokenizer(s, max_length=self.max_length, truncation=True)
                                 ["input_ids"], dtype=torch.int64) for s in seqs]
        self.num_labels = int(self.labels.max()) + 1 if labels else 0

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        return self.ids[i], self.labels[i]

    @property
    def pad_token_id(self):
        return self.tokenizer.pad_token_id

    def collate(self, items, unpad=False):
        """-> (ids, labels), padded to a multiple of 64 (collate_padded). unpad: (ids, labels,
        PackedIndex) for the packed encoder path; the width is then the batch maximum as it is --
        the rectangle only carries the ids, no kernel runs on its [PAD] cells."""
        if not unpad:
            return collate_padded(items, self.pad_token_id)
        from .bert_layers import PackedIndex
        ids, labels = collate_padded(items, self.pad_token_id, multiple=1)
        return ids, labels, PackedIndex.build(ids, self.pad_token_id)


def collate_padded(items, pad_token_id=3, multiple=64):
    """[(ids, label)] -> (ids [b, W] int64, labels [b]): W = the batch maximum rounded up to
    `multiple` (the bf16 attention kernel's tile), [PAD] fill."""
    width = max(int(ids.numel()) for ids, _ in items)
    width = (width + multiple - 1) // multiple * multiple
    out = torch.full((len(items), width), pad_token_id, dtype=torch.int64)
    for r, (ids, _) in enumerate(items):
        out[r, : ids.numel()] = ids
    return out, torch.stack([torch.as_tensor(l) for _, l in items])


_COMPLEMENT = str.maketrans("ACGTacgt", "TGCAtgca")


def string_reverse_complement(seq):
    """Reversed, A<->T and C<->G in either case; any other character stays as it is."""
    return seq[::-1].translate(_COMPLEMENT)


def remap_ids(ids):
    """Character-tokenizer ids -> the one-hot models' alphabet (the reference's datasets with
    use_tokenizer=False: genomic_bench_dataset.py:205-208, deepstarr.py:214-217,
    deepsea.py:188-191, hg38_dataset.py:383-386): ids - 7, then everything >= 4 or < 0 becomes 4.
    With the character vocabulary A C G T N = 7..11 that is A C G T = 0..3 and N, padding and
    every special token = 4."""
    ids = ids - 7
    return torch.where((ids >= 4) | (ids < 0), torch.full_like(ids, 4), ids)


def _want_remap(use_tokenizer, id_remap):
    """Both spellings of the remap: use_tokenizer=False (the reference's) or id_remap=True."""
    return (not use_tokenizer) if id_remap is None else bool(id_remap)


class _CharItems(torch.utils.data.Dataset):
    """What the character-level fine-tuning datasets share: how a sequence becomes an item.
    Tokenisation as the reference calls its tokenizer: truncation to max_length, padding to
    max_length on the tokenizer's side (left by default), add_eos appends [SEP] inside max_length,
    rc_aug replaces a sequence by its reverse complement with probability 1/2 per access (`rng`:
    a random.Random, for seeded draws). Items are (ids int64 [max_length], target) and, with
    return_mask, the attention mask (bool [max_length], False on padding) as a third entry.
    id_remap (the reference's use_tokenizer=False, for its one-hot models such as denoise_cnn):
    the ids become `remap_ids` of the tokenizer's -- A C G T = 0..3 and everything else, padding
    included, 4 -- and the mask is taken from the tokenizer's ids before that."""

    def _init_items(self, max_length, tokenizer, use_padding, add_eos, rc_aug, return_mask, rng,
                    id_remap=False):
        self.id_remap = bool(id_remap)
        self.max_length = int(max_length)
        self.tokenizer = tokenizer or CharacterTokenizer(["A", "C", "G", "T", "N"],
                                                         self.max_length + 2)
        self.use_padding, self.add_eos = use_padding, add_eos
        self.rc_aug, self.return_mask = rc_aug, return_mask
        self.rng = rng or random.Random()

    @property
    def pad_token_id(self):
        return self.tokenizer.pad_token_id

    def _item(self, x, target):
        if self.rc_aug and self.rng.random() < 0.5:
            x = string_reverse_complement(x)
        ids = self.tokenizer(x, add_special_tokens=bool(self.add_eos),
                             padding="max_length" if self.use_padding else False,
                             max_length=self.max_length, truncation=True)["input_ids"]
        ids = torch.tensor(ids, dtype=torch.int64)
        mask = ids != self.pad_token_id
        if self.id_remap:
            ids = remap_ids(ids)
        if self.return_mask:
            return ids, target, mask
        return ids, target

    def __getitem__(self, idx):
        return self._item(*self._pair(idx))

    def pairs(self):
        """(sequence string, target) of every item in order, before rc_aug and tokenisation: what
        a device-resident copy of the split is made from (resident.ResidentSplit). A loader
        defines `_pair(idx)`."""
        return (self._pair(i) for i in range(len(self)))

    def collate(self, items):
        """[(ids, target[, mask])] of one fixed length -> stacked tensors, in the same order."""
        return tuple(torch.stack(col) for col in zip(*items))


class GenomicBenchmarkFolder(_CharItems):
    """One split of a Genomic Benchmarks dataset as the reference's GenomicBenchmarkDataset reads
    it (src/dataloaders/datasets/genomic_bench_dataset.py:122-216): the folder
    `<dest_path>/<dataset_name>/<split>/<class>/` holds one text file per sequence; split "val"
    reads "test" (the benchmarks have no validation split). Nothing is ever downloaded: a missing
    folder is an error that says where the files are expected.

    Classes are numbered by sorted folder name. The reference numbers them in the order
    `Path.iterdir()` lists them, which depends on the file system and can differ between the train
    and the test folder; sorted names give every split and every machine the same labels.

    Items are (ids int64 [max_length], label int64) and, with return_mask, the attention mask
    (bool [max_length], False on padding) as a third entry. Tokenisation as the reference calls
    its tokenizer: truncation to max_length, padding to max_length on the tokenizer's side (left
    by default), add_eos appends [SEP] inside max_length, rc_aug replaces a sequence by its
    reverse complement with probability 1/2 per access (`rng`: a random.Random, for seeded
    draws). classes: the class folders another split of the dataset has (its `.classes`); a
    split whose folders differ is an error, since a missing class would shift the labels.
    use_tokenizer=False (or id_remap=True): the ids of the one-hot models (`remap_ids`)."""

    def __init__(self, dest_path, dataset_name, split, max_length, tokenizer=None, d_output=None,
                 use_padding=True, add_eos=False, rc_aug=False, return_mask=False, rng=None,
                 classes=None, use_tokenizer=True, id_remap=None):
        self.split = "test" if split == "val" else split
        self.base_path = os.path.join(str(dest_path), dataset_name, self.split)
        if not os.path.isdir(self.base_path):
            raise FileNotFoundError(
                f"{self.base_path}: no such folder. Genomic Benchmarks data is not downloaded "
                f"here; put the dataset at <dest_path>/{dataset_name}/{self.split}/<class>/*.txt")
        self._init_items(max_length, tokenizer, use_padding, add_eos, rc_aug, return_mask, rng,
                         _want_remap(use_tokenizer, id_remap))
        self.classes = sorted(d for d in os.listdir(self.base_path)
                              if os.path.isdir(os.path.join(self.base_path, d)))
        if not self.classes:
            raise FileNotFoundError(f"{self.base_path}: no class folders")
        if classes is not None and list(classes) != self.classes:
            raise ValueError(f"{self.base_path}: class folders {self.classes} differ from the "
                             f"expected {list(classes)}; the labels would not mean the same")
        self.all_seqs, self.all_labels = [], []
        for label, name in enumerate(self.classes):
            folder = os.path.join(self.base_path, name)
            for fn in sorted(os.listdir(folder)):
                with open(os.path.join(folder, fn)) as f:
                    self.all_seqs.append(f.read())
                self.all_labels.append(label)
        self.num_labels = len(self.classes)
        self.d_output = self.num_labels if d_output is None else int(d_output)

    def __len__(self):
        return len(self.all_labels)

    def _pair(self, idx):
        return self.all_seqs[idx], torch.tensor(self.all_labels[idx], dtype=torch.int64)


DEEPSTARR_TARGETS = ("Dev_log2_enrichment", "Hk_log2_enrichment")
_DEEPSTARR_SPLITS = {"train": "Train", "val": "Val", "valid": "Val", "test": "Test"}


class DeepSTARRFolder(_CharItems):
    """One split of the DeepSTARR enhancer-activity data as the reference's DeepSTARRDataset
    reads it (src/dataloaders/datasets/deepstarr.py:123-225): `<dest_path>/Sequences_<Split>.fa`
    (Split Train | Val | Test; "val" and "valid" read Val) and
    `<dest_path>/Sequences_activity_<Split>.txt`, tab-separated with a header, of which the two
    columns DEEPSTARR_TARGETS are taken by name. The FASTA is read as the reference reads it: one
    sequence line per header, stopping at the first empty line. Nothing is ever downloaded: a
    missing file is an error that says where it is expected, and so is a FASTA whose sequence
    count differs from the table's.

    Items are (ids int64 [max_length], target fp32 [2]) (+ mask); tokenisation, add_eos, rc_aug,
    return_mask and collate as in _CharItems. id_remap=True gives the ids of the one-hot models
    (`remap_ids`, the reference's use_tokenizer=False). The spelling use_tokenizer=False itself
    stays the error it has always been here (callers rely on it): it names id_remap."""

    num_labels = d_output = len(DEEPSTARR_TARGETS)

    def __init__(self, dest_path, split, max_length, tokenizer=None, use_padding=True,
                 add_eos=False, rc_aug=False, return_mask=False, rng=None, use_tokenizer=True,
                 id_remap=False):
        if not use_tokenizer:
            raise NotImplementedError("DeepSTARRFolder use_tokenizer=False is not taken: the "
                                      "diffusion models' id remap is id_remap=True here")
        if split.lower() not in _DEEPSTARR_SPLITS:
            raise ValueError(f"split {split!r}: one of {sorted(_DEEPSTARR_SPLITS)}")
        name = _DEEPSTARR_SPLITS[split.lower()]
        self.fasta_path = os.path.join(str(dest_path), f"Sequences_{name}.fa")
        self.table_path = os.path.join(str(dest_path), f"Sequences_activity_{name}.txt")
        for path in (self.fasta_path, self.table_path):
            if not os.path.exists(path):
                raise FileNotFoundError(
                    f"{path}: no such file. DeepSTARR data is not downloaded here; put "
                    f"Sequences_{name}.fa and Sequences_activity_{name}.txt into <dest_path>")
        self._init_items(max_length, tokenizer, use_padding, add_eos, rc_aug, return_mask, rng,
                         id_remap)
        with open(self.table_path, newline="") as f:
            rows = csv.reader(f, delimiter="\t")
            header = next(rows, [])
            missing = [c for c in DEEPSTARR_TARGETS if c not in header]
            if missing:
                raise ValueError(f"{self.table_path}: no column {missing} in the header {header}")
            cols = [header.index(c) for c in DEEPSTARR_TARGETS]
            targets = [[float(r[c]) for c in cols] for r in rows if r]
        self.targets = torch.tensor(targets, dtype=torch.float32).reshape(-1, len(cols))
        self.all_seqs = []
        with open(self.fasta_path) as f:
            seen_header = False
            for line in f:
                line = line.strip()
                if not line:
                    break
                if line.startswith(">"):
                    seen_header = True
                    continue
                if not seen_header:
                    raise ValueError(f"{self.fasta_path}: a sequence before the first header")
                self.all_seqs.append(line)
        if len(self.all_seqs) != len(self.targets):
            raise ValueError(f"{self.fasta_path}: {len(self.all_seqs)} sequences, but "
                             f"{self.table_path} has {len(self.targets)} rows of targets")

    def __len__(self):
        return len(self.all_seqs)

    def _pair(self, idx):
        return self.all_seqs[idx], self.targets[idx]


DEEPSEA_LABELS = 919


class DeepSEACsv(_CharItems):
    """One split of the DeepSEA chromatin-profile data as the reference's DeepSEADataset reads it
    (src/dataloaders/datasets/deepsea.py:121-199): `<dest_path>/<split>.csv.gz` (train | valid |
    test; "val" reads valid), no header, column 0 the sequence and columns 1 .. 919 the 0/1
    labels. Read with gzip + csv; the labels are held as one uint8 array [rows, 919]. max_rows:
    only the first rows of the file are kept -- the reference hard-codes 40,000 per split, the
    default here; None reads everything. Nothing is ever downloaded: a missing file is an error
    that says where it is expected.

    Items are (ids int64 [max_length], target fp32 [919]) (+ mask); tokenisation, add_eos, rc_aug,
    return_mask and collate as in _CharItems. use_tokenizer=False (or id_remap=True): the ids of
    the one-hot models (`remap_ids`)."""

    num_labels = d_output = DEEPSEA_LABELS

    def __init__(self, dest_path, split, max_length, max_rows=40000, tokenizer=None,
                 use_padding=True, add_eos=False, rc_aug=False, return_mask=False, rng=None,
                 use_tokenizer=True, id_remap=None):
        split = "valid" if split.lower() == "val" else split.lower()
        if split not in ("train", "valid", "test"):
            raise ValueError(f"split {split!r}: one of train, val / valid, test")
        self.path = os.path.join(str(dest_path), f"{split}.csv.gz")
        if not os.path.exists(self.path):
            raise FileNotFoundError(
                f"{self.path}: no such file. DeepSEA data is not downloaded here; put train.csv.gz, "
                "valid.csv.gz and test.csv.gz into <dest_path>")
        self._init_items(max_length, tokenizer, use_padding, add_eos, rc_aug, return_mask, rng,
                         _want_remap(use_tokenizer, id_remap))
        self.all_seqs, rows = [], []
        with gzip.open(self.path, "rt", newline="") as f:
            for i, row in enumerate(csv.reader(f)):
                if max_rows is not None and i >= int(max_rows):
                    break
                if len(row) != DEEPSEA_LABELS + 1:
                    raise ValueError(f"{self.path}: row {i} has {len(row)} columns, not a sequence "
                                     f"and {DEEPSEA_LABELS} labels")
                self.all_seqs.append(row[0])
                rows.append(bytes(int(v) for v in row[1:]))
        self.labels = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8).reshape(
            len(rows), DEEPSEA_LABELS) if rows else torch.zeros(0, DEEPSEA_LABELS, dtype=torch.uint8)

    def __len__(self):
        return len(self.all_seqs)

    def _pair(self, idx):
        return self.all_seqs[idx], self.labels[idx].to(torch.float32)


# The Nucleotide Transformer benchmark's 18 tasks: the per-task entries of the reference's
# configs/dataset/nucleotide_transformer.yaml (tests/golden/nt_tasks.json is parsed from it).
# train_len: training sequences (the cosine schedule's length); classes: d_output; max_length:
# the tokenised length; metric: what train.monitor follows as val/<metric>.
def _nt(train_len, classes, max_length, metric):
    return {"train_len": train_len, "classes": classes, "max_length": max_length, "metric": metric}


NT_TASKS = {
    "enhancer": _nt(14968, 2, 200, "mcc"),
    "enhancer_types": _nt(14968, 3, 200, "mcc"),
    "H3": _nt(13468, 2, 500, "mcc"),
    "H3K4me1": _nt(28509, 2, 500, "mcc"),
    "H3K4me2": _nt(27614, 2, 500, "mcc"),
    "H3K4me3": _nt(33119, 2, 500, "mcc"),
    "H3K9ac": _nt(25003, 2, 500, "mcc"),
    "H3K14ac": _nt(29743, 2, 500, "mcc"),
    "H3K36me3": _nt(31392, 2, 500, "mcc"),
    "H3K79me3": _nt(25953, 2, 500, "mcc"),
    "H4": _nt(13140, 2, 500, "mcc"),
    "H4ac": _nt(30685, 2, 500, "mcc"),
    "promoter_all": _nt(53276, 2, 300, "f1_macro"),
    "promoter_non_tata": _nt(47759, 2, 300, "f1_macro"),
    "promoter_tata": _nt(5517, 2, 300, "f1_macro"),
    "splice_sites_acceptor": _nt(19961, 2, 600, "f1_macro"),
    "splice_sites_donor": _nt(19775, 2, 600, "f1_macro"),
    "splice_sites_all": _nt(27000, 3, 600, "f1_macro"),
}


def read_fasta(path):
    """-> [(header line after '>', sequence)] of a FASTA file with any line wrapping; blank lines
    are skipped, sequence lines are joined without their line ends."""
    records, key, parts = [], None, []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if key is not None:
                    records.append((key, "".join(parts)))
                key, parts = line[1:], []
            elif line.strip():
                if key is None:
                    raise ValueError(f"{path}: a sequence before the first header")
                parts.append(line.strip())
    if key is not None:
        records.append((key, "".join(parts)))
    return records


class NucleotideTransformerFasta(_CharItems):
    """One split of a Nucleotide Transformer benchmark task as the reference's
    NucleotideTransformerDataset reads it (src/dataloaders/datasets/
    nucleotide_transformer_dataset.py:26-113): the folder `<dest_path>/<dataset_name>/` holds one
    `*.fasta` file per split, found by the split's name in the file name; split "val" reads
    "test" (the benchmark has no validation split). A record's key is its whole header line
    after '>' (pyfaidx read_long_names) and its label the key's last character, as an integer:
    `int(key.rstrip()[-1])`. Nothing is ever downloaded: a missing folder or file is an error
    that says where the files are expected.

    Two deliberate differences from the reference. It tests `split in str(file)` on the whole
    path, so a parent directory named like a split matches every file and the last one
    `iterdir()` lists wins; here only the file name is matched, and no match or more than one
    is an error. Duplicate headers are an error (pyfaidx's default makes them one), and so is a
    label >= d_output.

    Items are (ids int64 [max_length], label int64) (+ mask); tokenisation, add_eos, rc_aug,
    return_mask and collate as in _CharItems. use_tokenizer=False (or id_remap=True): the ids of
    the one-hot models (`remap_ids`)."""

    def __init__(self, dest_path, dataset_name, split, max_length, tokenizer=None, d_output=None,
                 use_padding=True, add_eos=False, rc_aug=False, return_mask=False, rng=None,
                 use_tokenizer=True, id_remap=None):
        self.split = "test" if split == "val" else split
        self.base_path = os.path.join(str(dest_path), dataset_name)
        where = (f"Nucleotide Transformer benchmark data is not downloaded here; put the task's "
                 f"files at <dest_path>/{dataset_name}/*{self.split}*.fasta")
        if not os.path.isdir(self.base_path):
            raise FileNotFoundError(f"{self.base_path}: no such folder. {where}")
        found = sorted(fn for fn in os.listdir(self.base_path)
                       if fn.endswith(".fasta") and self.split in fn)
        if not found:
            raise FileNotFoundError(f"{self.base_path}: no *.fasta file named after the split "
                                    f"{self.split!r}. {where}")
        if len(found) > 1:
            raise ValueError(f"{self.base_path}: {found} all match the split {self.split!r}; "
                             "exactly one *.fasta file per split is expected")
        self.path = os.path.join(self.base_path, found[0])
        self._init_items(max_length, tokenizer, use_padding, add_eos, rc_aug, return_mask, rng,
                         _want_remap(use_tokenizer, id_remap))
        known = NT_TASKS.get(dataset_name)
        self.d_output = int(d_output) if d_output is not None else (known["classes"] if known
                                                                    else None)
        self.all_seqs, self.all_labels, seen = [], [], set()
        for key, seq in read_fasta(self.path):
            if key in seen:
                raise ValueError(f"{self.path}: duplicate header {key!r}")
            seen.add(key)
            last = key.rstrip()[-1:]
            if not last.isdigit():
                raise ValueError(f"{self.path}: header {key!r} does not end in a label digit")
            label = int(last)
            if self.d_output is not None and label >= self.d_output:
                raise ValueError(f"{self.path}: header {key!r} has label {label}, but d_output "
                                 f"is {self.d_output}")
            self.all_seqs.append(seq)
            self.all_labels.append(label)
        self.num_labels = (self.d_output if self.d_output is not None
                           else max(self.all_labels, default=-1) + 1)

    def __len__(self):
        return len(self.all_labels)

    def _pair(self, idx):
        return self.all_seqs[idx], torch.tensor(self.all_labels[idx], dtype=torch.int64)


# ------------------------------------------------------------------ windows cut out of genomes
# The chromosomes of each split of the species benchmark: the reference's table
# (species_dataset.py SPECIES_CHROMOSOME_SPLITS; tests/golden/species_splits.json is dumped from
# it) restated. Validation and test chromosomes are the same for all ten species; the training
# chromosomes are the even ones up to 8, then 14 up to the species' last autosome, then the sex
# chromosomes it has (the great apes' chromosome 2 is 2A and 2B).
_SPECIES_VALID = ["1", "3", "12", "13"]
_SPECIES_TEST = ["5", "7", "9", "10", "11"]


def _species_train(last, sex, two=("2",)):
    return list(two) + ["4", "6", "8"] + [str(i) for i in range(14, last + 1)] + list(sex)


SPECIES_SPLITS = {
    name: {"train": train, "valid": list(_SPECIES_VALID), "test": list(_SPECIES_TEST)}
    for name, train in {
        "human": _species_train(22, "XY"),
        "lemur": _species_train(27, "XY"),
        "goat": _species_train(29, "XY"),
        "sheep": _species_train(26, "XY"),
        "pig": _species_train(18, "XY"),
        "mouse": _species_train(19, "X"),
        "gorilla": _species_train(22, "XY", ("2A", "2B")),
        "orangutan": _species_train(22, "XY", ("2A", "2B")),
        "chimpanzee": _species_train(22, "XY", ("2A", "2B")),
        "hippo": _species_train(17, "X"),
    }.items()
}


def species_split_sizes(total_size, max_length, max_length_val=None, max_length_test=None):
    """-> {"train", "valid", "test": (items, max_length)} as the reference's Species data module
    sizes its splits (genomics.py:584-602): total_size * ((max_length_test + 2) // max_len) items
    for train and valid, total_size for test."""
    mv = max_length if max_length_val is None else max_length_val
    mt = max_length if max_length_test is None else max_length_test
    return {"train": (int(total_size) * ((mt + 2) // max_length), int(max_length)),
            "valid": (int(total_size) * ((mt + 2) // mv), int(mv)),
            "test": (int(total_size), int(mt))}


class SpeciesWindows(torch.utils.data.Dataset):
    """One split of the long-range species classification benchmark as the reference's
    SpeciesDataset makes it (src/dataloaders/datasets/species_dataset.py:82-333, tokenizer_name
    char): every access draws a random window of a random chromosome of a random species, and the
    target is the species' index. Files are `<species_dir>/<species>/chr<name>.{fna,fa,fna.gz}`
    (a .gz is read in memory, never unzipped into the folder), one record each, upper-cased; the
    chromosomes of `split` (train | valid | test; "val" reads valid) come from SPECIES_SPLITS.

    Per item `rng` (a random.Random; the reference draws from the global one) is asked, in this
    order, for rng.choices(species, species_weights), rng.choices(chromosomes, weights) and
    rng.randint(left, right), where with remove_tail_ends left, right = int(len * cutoff),
    int(len * (1 - cutoff)) (cutoff_train for train, cutoff_test otherwise) and without it
    left, right = 0, len - max_length -- a chromosome shorter than max_length raises there, as
    randint does. The window is chrom[start : min(start + max_length, right)], right-justified
    to max_length with N. That keeps a quirk of the reference: `right` bounds the slice too, so
    the last max_length bases of a chromosome are never read and rows can be partly or wholly N.
    The ids are the character ids, [SEP] appended with add_eos, then the last id dropped:
    max_length ids with add_eos, max_length - 1 without. The index of an access is ignored.

    species_weights / chromosome_weights: "uniform", "weighted_by_bp" (by record length,
    normalised) or explicit -- a list per species, {species: list} for the chromosomes.
    weighted_by_bp restates the reference's `len(Fasta)`-based weights from the record lengths;
    no fixture pins it, since pyfaidx is not available to run the reference's version.
    task: species_classification only. use_tokenizer=False (or id_remap=True): `remap_ids`.

    `store` is a genome.GenomeStore of this split's chromosomes under "<species>/chr<name>";
    rows(k) draws k windows as (src, n, left, targets) for resident.ResidentWindows, consuming
    the rng exactly as k accesses do."""

    redraws = True  # a pass over the split draws new windows

    def __init__(self, species, species_dir, split, max_length, total_size, tokenizer=None,
                 add_eos=True, species_weights="uniform", chromosome_weights="uniform",
                 task="species_classification", remove_tail_ends=False, cutoff_train=0.1,
                 cutoff_test=0.2, rng=None, use_tokenizer=True, id_remap=None):
        from .genome import GenomeStore
        if task == "next_token_pred":
            raise NotImplementedError("SpeciesWindows task=next_token_pred is not built; "
                                      "species_classification only")
        if task != "species_classification":
            raise ValueError(f"task {task!r}: species_classification")
        self.split = "valid" if split == "val" else split
        if self.split not in ("train", "valid", "test"):
            raise ValueError(f"split {split!r}: one of train, val / valid, test")
        self.species = list(species)
        self.max_length, self.total_size = int(max_length), int(total_size)
        self.add_eos = bool(add_eos)
        self.row_length = self.max_length if self.add_eos else self.max_length - 1
        if self.row_length < 1:
            raise ValueError(f"max_length {max_length}: no id is left after the last is dropped")
        self.tokenizer = tokenizer or CharacterTokenizer(["A", "C", "G", "T", "N"],
                                                         self.max_length + 2)
        self.id_remap = _want_remap(use_tokenizer, id_remap)
        self.rng = rng or random.Random()
        self.remove_tail_ends = bool(remove_tail_ends)
        self.cutoff = float(cutoff_train if self.split == "train" else cutoff_test)
        self.num_labels = self.d_output = len(self.species)
        records, self.chromosomes = {}, {}
        for spec in self.species:
            if spec not in SPECIES_SPLITS:
                raise ValueError(f"species {spec!r}: one of {sorted(SPECIES_SPLITS)}")
            folder = os.path.join(str(species_dir), spec)
            if not os.path.isdir(folder):
                raise FileNotFoundError(f"{folder}: no such folder. Genomes are not downloaded "
                                        "here; put chr<name>.fna (.fa, .fna.gz) files there")
            self.chromosomes[spec] = list(SPECIES_SPLITS[spec][self.split])
            for chrom in self.chromosomes[spec]:
                path = GenomeStore.find(folder, f"chr{chrom}")
                recs = GenomeStore.from_fasta(path, upper=True)
                if len(recs) != 1:
                    raise ValueError(f"{path}: {len(recs)} records, one chromosome is expected")
                records[f"{spec}/chr{chrom}"] = recs.record(recs.names[0])
        self.store = GenomeStore(records)
        lens = {s: [self.store.length(f"{s}/chr{c}") for c in self.chromosomes[s]]
                for s in self.species}
        norm = lambda w: [x / sum(w) for x in w]
        self.chromosome_weights = {}
        for spec in self.species:
            w = (chromosome_weights.get(spec) if isinstance(chromosome_weights, dict)
                 else chromosome_weights)
            if w == "uniform":
                w = [1] * len(lens[spec])
            elif w == "weighted_by_bp":
                w = norm(lens[spec])
            elif not isinstance(w, (list, tuple)) or len(w) != len(lens[spec]):
                raise ValueError(f"chromosome_weights for {spec!r}: uniform, weighted_by_bp or "
                                 f"{len(lens[spec])} weights, one per chromosome of the split")
            self.chromosome_weights[spec] = list(w)
        if species_weights == "uniform":
            self.species_weights = [1] * len(self.species)
        elif species_weights == "weighted_by_bp":
            self.species_weights = norm([sum(lens[s]) for s in self.species])
        elif isinstance(species_weights, (list, tuple)) and len(species_weights) == len(self.species):
            self.species_weights = list(species_weights)
        else:
            raise ValueError(f"species_weights: uniform, weighted_by_bp or {len(self.species)} "
                             "weights, one per species")

    def __len__(self):
        return self.total_size

    def draw(self):
        """One window: (species index, record name, start, bases read), three draws."""
        spec = self.rng.choices(self.species, weights=self.species_weights, k=1)[0]
        chrom = self.rng.choices(self.chromosomes[spec], weights=self.chromosome_weights[spec],
                                 k=1)[0]
        name = f"{spec}/chr{chrom}"
        length = self.store.length(name)
        if self.remove_tail_ends:
            left, right = int(length * self.cutoff), int(length * (1 - self.cutoff))
        else:
            left, right = 0, length - self.max_length
        start = self.rng.randint(left, right)
        return self.species.index(spec), name, start, min(start + self.max_length, right) - start

    def __getitem__(self, idx):
        label, name, start, n = self.draw()
        seq = self.store.record(name)[start:start + n].decode("latin-1").rjust(self.max_length, "N")
        ids = self.tokenizer(seq, add_special_tokens=False)["input_ids"]
        if self.add_eos:
            ids.append(self.tokenizer.sep_token_id)
        ids = torch.tensor(ids, dtype=torch.int64)[:-1].clone()
        if self.id_remap:
            ids = remap_ids(ids)
        return ids, torch.tensor(label, dtype=torch.int64)

    def rows(self, k):
        """k windows as the device kernel takes them -> (src int64 [k], n int32 [k], left int32
        [k], targets int64 [k]): the same draws, in the same order, as k accesses."""
        src, n, tgt = torch.empty(k, dtype=torch.int64), torch.empty(k, dtype=torch.int32), \
            torch.empty(k, dtype=torch.int64)
        for i in range(k):
            label, name, start, nb = self.draw()
            src[i], n[i], tgt[i] = self.store.offset(name) + start, nb, label
        return src, n, self.max_length - n, tgt

    def window_spec(self):
        """How a row is filled: (byte -> id table int64 [256], fill id, eos id or -1, tail id or
        -1). The fill is N's id; the [SEP] of add_eos is the id that is dropped."""
        lut = torch.from_numpy(self.tokenizer._lut.astype("int64").copy())
        fill = torch.tensor(int(lut[ord("N")]))
        if self.id_remap:
            lut, fill = remap_ids(lut), remap_ids(fill)
        return lut, int(fill), -1, -1

    def collate(self, items):
        return tuple(torch.stack(col) for col in zip(*items))


class ChromatinProfile(torch.utils.data.Dataset):
    """One split of the chromatin-profile benchmark as the reference's ChromatinProfileDataset
    reads it (src/dataloaders/datasets/chromatin_profile_dataset.py:30-224, genomics.py:420-494):
    `<data_path>/<split>_<ref_genome_version>_coords_targets.csv` (split train | val | test) with
    the columns Chr_No (0-based: record chr{Chr_No + 1} of the genome), Start, End and one 0/1
    column per name that begins with y_ (919 in the benchmark). ref_genome_version is hg19 or
    hg38 and must be named by the coordinates file: the reference lifts hg19 coordinates over to
    hg38 on the fly, which is not built here -- such a pair raises and says so.

    The window of a row (FastaInterval.__call__): Start and End move outwards by
    int((max_length - 1000) / 2) each; an interval shorter than max_length grows symmetrically
    (the odd base to the right); what falls off either end of the chromosome becomes '.'; of an
    interval longer than max_length the first max_length bases are kept. The window is
    upper-cased and tokenised with the tokenizer's default call, so '.' is [UNK] and [SEP] is
    appended: max_length + 1 ids for the benchmark's 1,000-base intervals. No padding, and no
    reverse complement (the reference builds its interval reader without it).

    Items are (ids int64, target fp32 [labels]) -- the dtype and shape DeepSEACsv gives, so head,
    loss and AUROC are DeepSEA's. use_tokenizer=False (or id_remap=True): `remap_ids`.
    genome: a genome.GenomeStore of the reference genome that the splits share; it is read from
    ref_genome_path (.fa / .fna, plain or .gz) otherwise. `store` holds only the chromosomes
    this split names; rows() gives every item's (src, n, left, right) for
    resident.ResidentWindows."""

    redraws = False

    def __init__(self, data_path, ref_genome_path, ref_genome_version, split, max_length,
                 tokenizer=None, use_tokenizer=True, id_remap=None, genome=None,
                 coords_target_path=None):
        from .genome import GenomeStore
        self.max_length = int(max_length)
        if self.max_length % 2:
            raise ValueError(f"max_length {max_length}: the window must be even")
        if ref_genome_version not in ("hg19", "hg38"):
            raise ValueError('ref_genome_version must be "hg19" or "hg38"')
        split = "val" if split in ("valid", "dev") else split
        other = "hg38" if ref_genome_version == "hg19" else "hg19"
        path = coords_target_path or os.path.join(
            str(data_path), f"{split}_{ref_genome_version}_coords_targets.csv")
        fn = os.path.basename(path)
        if ref_genome_version not in fn or not os.path.exists(path):
            alt = path if other in fn else os.path.join(
                os.path.dirname(path), fn.replace(ref_genome_version, other))
            if other in os.path.basename(alt) and os.path.exists(alt):
                raise ValueError(
                    f"{alt}: coordinates of {other}, but ref_genome_version={ref_genome_version!r}. "
                    "Liftover between genome versions is not built here; convert the coordinates "
                    f"first and name the file {split}_{ref_genome_version}_coords_targets.csv")
            if not os.path.exists(path):
                raise FileNotFoundError(
                    f"{path}: no such file. The chromatin-profile tables are not downloaded here; "
                    "put {train,val,test}_<version>_coords_targets.csv into <data_path>")
            raise ValueError(f"{path}: the file name must carry the genome version "
                             f"{ref_genome_version!r} of its coordinates")
        self.path = path
        self.tokenizer = tokenizer or CharacterTokenizer(["A", "C", "G", "T", "N"],
                                                         self.max_length + 2)
        self.id_remap = _want_remap(use_tokenizer, id_remap)
        self.coords, rows = [], []
        with open(path, newline="") as f:
            reader = csv.reader(f)
            header = next(reader, [])
            missing = [c for c in ("Chr_No", "Start", "End") if c not in header]
            if missing:
                raise ValueError(f"{path}: no column {missing} in the header")
            ci, si, ei = (header.index(c) for c in ("Chr_No", "Start", "End"))
            self.target_columns = [c for c in header if c[:2] == "y_"]
            ycols = [i for i, c in enumerate(header) if c[:2] == "y_"]
            for row in reader:
                if not row:
                    continue
                self.coords.append((int(row[ci]), int(row[si]), int(row[ei])))
                rows.append(bytes(1 if row[i].strip() in ("1", "1.0", "True", "true") else 0
                                  for i in ycols))
        self.num_labels = self.d_output = len(ycols)
        self.labels = (torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8)
                       .reshape(len(rows), len(ycols)) if rows and ycols
                       else torch.zeros(len(rows), len(ycols), dtype=torch.uint8))
        if genome is None:
            genome = GenomeStore.from_fasta(ref_genome_path)
        names = sorted({f"chr{c + 1}" for c, _, _ in self.coords}, key=lambda s: int(s[3:]))
        absent = [k for k in names if k not in genome]
        if absent:
            raise ValueError(f"{path}: names {absent}, which the reference genome does not hold")
        self.store = genome.subset(names)
        half = int((self.max_length - 1000) / 2)
        self._windows = [self._window(f"chr{c + 1}", s - half, e + half)
                         for c, s, e in self.coords]

    def _window(self, name, start, end):
        """FastaInterval.__call__ -> (record, first base, bases read, '.' before, '.' after)."""
        length, ml = self.store.length(name), self.max_length
        interval = end - start
        if interval < ml:
            extra = ml - interval
            start -= extra // 2
            end += extra - extra // 2
        left = right = 0
        if start < 0:
            left, start = -start, 0
        if end > length:
            right, end = end - length, length
        if interval > ml:
            end = start + ml
        cut = range(length)[start:end]  # what a Python slice of the record reads
        return name, cut.start if len(cut) else 0, len(cut), left, right

    def __len__(self):
        return len(self.coords)

    def __getitem__(self, idx):
        name, start, n, left, right = self._windows[idx]
        seq = "." * left + self.store.record(name)[start:start + n].decode("latin-1") + "." * right
        ids = torch.tensor(self.tokenizer(seq.upper())["input_ids"], dtype=torch.int64)
        if self.id_remap:
            ids = remap_ids(ids)
        return ids, self.labels[idx].to(torch.float32)

    def rows(self):
        """Every item's window -> (src int64 [N], n, left, right int32 [N])."""
        src = torch.tensor([self.store.offset(w[0]) + w[1] for w in self._windows],
                           dtype=torch.int64)
        n, left, right = (torch.tensor([w[i] for w in self._windows], dtype=torch.int32)
                          for i in (2, 3, 4))
        return src, n, left, right

    @property
    def row_length(self):
        return self.max_length + 1

    def window_spec(self):
        """(byte -> id table of the upper-cased byte, fill id = '.', eos id, tail id): [SEP]
        follows the bases directly when no window runs off a chromosome's right end (eos id);
        otherwise it is written into the last cell after the fill (tail id)."""
        base = self.tokenizer._lut.astype("int64")
        lut = torch.tensor([int(base[bytes([b]).upper()[0]]) for b in range(256)])
        fill, sep = torch.tensor(int(base[ord(".")])), torch.tensor(self.tokenizer.sep_token_id)
        if self.id_remap:
            lut, fill, sep = remap_ids(lut), remap_ids(fill), remap_ids(sep)
        runs_off = any(w[4] > 0 for w in self._windows)
        return lut, int(fill), -1 if runs_off else int(sep), int(sep) if runs_off else -1

    def collate(self, items):
        return tuple(torch.stack(col) for col in zip(*items))
