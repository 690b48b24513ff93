"""A genome as bytes: named records (chromosomes), one byte per base, with an offsets table.

GenomeStore is what the whole-genome fine-tuning datasets (finetune_data.SpeciesWindows,
ChromatinProfile) cut their windows out of on the host, and -- after `to(device)` -- what
resident.ResidentWindows cuts them out of on the device with `dna_genome_windows`
(csrc/genome_windows.hip): the records concatenated into one uint8 tensor, and a record's window
addressed by `offset(name) + start`.

FASTA files are read whole, line breaks stripped, case as in the file unless `upper`. `.fa`,
`.fna`, `.fasta` and their `.gz` forms are accepted; a `.gz` file is read in memory and nothing
is written (the reference unzips `chr*.fna.gz` into the data folder, which needs a writable
dataset; here the folder may be read-only).
"""
import gzip
import os

import numpy as np
import torch

FASTA_SUFFIXES = (".fna", ".fa", ".fasta", ".fna.gz", ".fa.gz", ".fasta.gz")


def read_fasta_bytes(path):
    """-> [(header line after '>', sequence bytes)] of a FASTA file with any line wrapping:
    finetune_data.read_fasta on bytes, and through gzip for a name ending in .gz."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        data = f.read()
    records = []
    for n, chunk in enumerate(data.split(b">")):
        if n == 0:
            if chunk.strip():
                raise ValueError(f"{path}: a sequence before the first header")
            continue
        head, _, body = chunk.partition(b"\n")
        records.append((head.rstrip(b"\r").decode("latin-1"), b"".join(body.split())))
    return records


class GenomeStore:
    """records: {name: bytes}, in insertion order. `bases` is their concatenation (uint8 tensor,
    one spare byte at the end so an empty store still has a buffer), `offsets` int64 [R + 1].
    to(device) returns a store whose `bases` live there; names, lengths and offsets stay on the
    host, where every window is decided."""

    def __init__(self, records):
        self.names = list(records)
        lens = [len(records[k]) for k in self.names]
        self.offsets = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(np.asarray(lens, dtype=np.int64), out=self.offsets[1:])
        self._index = {k: i for i, k in enumerate(self.names)}
        self._records = {k: bytes(records[k]) for k in self.names}
        self._bases = None

    @classmethod
    def from_fasta(cls, path, upper=False, names=None):
        """Every record of one FASTA file under its first header word (pyfaidx's key), or only
        `names`. upper: upper-cased, as pyfaidx's sequence_always_upper."""
        recs = {}
        for head, seq in read_fasta_bytes(path):
            key = head.split()[0] if head.split() else ""
            if names is not None and key not in names:
                continue
            if key in recs:
                raise ValueError(f"{path}: duplicate record {key!r}")
            recs[key] = seq.upper() if upper else seq
        return cls(recs)

    @staticmethod
    def find(folder, stem):
        """The file `<folder>/<stem><suffix>` for the first of FASTA_SUFFIXES that exists."""
        tried = [os.path.join(str(folder), stem + s) for s in FASTA_SUFFIXES]
        for p in tried:
            if os.path.exists(p):
                return p
        raise FileNotFoundError(f"none of {tried} exists")

    def __len__(self):
        return len(self.names)

    def __contains__(self, name):
        return name in self._index

    @property
    def n_bases(self):
        return int(self.offsets[-1])

    def length(self, name):
        i = self._index[name]
        return int(self.offsets[i + 1] - self.offsets[i])

    def offset(self, name):
        return int(self.offsets[self._index[name]])

    def record(self, name):
        return self._records[name]

    def subset(self, names):
        """A store of only these records (a split uploads its own chromosomes)."""
        return GenomeStore({k: self._records[k] for k in names})

    @property
    def bases(self):
        if self._bases is None:
            buf = bytearray(b"".join(self._records[k] for k in self.names) + b"\0")
            self._bases = torch.frombuffer(buf, dtype=torch.uint8)
        return self._bases

    @property
    def device(self):
        return self.bases.device

    def to(self, device):
        out = GenomeStore.__new__(GenomeStore)
        out.__dict__.update(self.__dict__)
        out._bases = self.bases.to(device)
        return out
