"""A fine-tuning split held on the device, and its batches built there by one HIP kernel.

The character-level datasets (finetune_data._CharItems) make an item per access on the host: the
tokenizer runs on a Python string, then torch.tensor, remap_ids and torch.stack per batch.
ResidentSplit uploads a split once -- every sequence's bytes, their offsets, the targets, and the
tokenizer as a 256-entry byte -> id table -- and `batch(start, stop)` assembles rows
order[start:stop] with `dna_char_batch` (csrc/char_batch.hip): truncation, [SEP], padding on
either side, the reverse complement and the one-hot models' id remap included, integer-exact
with `collate([ds[j] for j in order[start:stop]])`. No host-to-device copy and no sync per batch.

Randomness stays on the host, where the item-by-item path has it: the caller draws the epoch's
permutation, and the reverse-complement flags come from the dataset's own random.Random, one draw
per item in access order, as `_CharItems._item` draws them. The same seeds give the same batches
on both paths.

ResidentWindows carries the same idea from per-sequence splits to whole genomes: the datasets
that cut their windows out of chromosomes (species, chromatin_profile) keep a genome.GenomeStore
on the device, and `dna_genome_windows` (csrc/genome_windows.hip) builds a batch from one
(src, n, left) triple per row.
"""
import numpy as np
import torch

from . import _native as N
from .finetune_data import remap_ids

_COMPLEMENT_PAIRS = ("ACGTacgt", "TGCAtgca")  # finetune_data._COMPLEMENT as bytes


def complement_table():
    """uint8 [256]: the bytes of ACGTacgt swapped as finetune_data._COMPLEMENT swaps the
    characters, identity elsewhere."""
    t = np.arange(256, dtype=np.uint8)
    for a, b in zip(*_COMPLEMENT_PAIRS):
        t[ord(a)] = ord(b)
    return t


class ResidentSplit:
    """One `_CharItems` dataset on the device. from_dataset(ds, device) builds it; set_epoch
    uploads an epoch's order (and reverse-complement flags); batch(start, stop) -> (ids int64
    [b, max_length], targets[, mask bool [b, max_length]]) on the device."""

    def __init__(self, bases, offsets, targets, lut, max_length, pad_id, eos_id, pad_left,
                 return_mask=False, rc_aug=False, rng=None, device="cuda"):
        """bases: bytes of all sequences, concatenated; offsets: int64 [N + 1] (host); targets:
        [N] or [N, C] (host); lut: int64 [256] byte -> output id (host). pad_id / eos_id: the
        output ids (eos_id < 0: no eos)."""
        self.device = torch.device(device)
        offsets = torch.as_tensor(offsets, dtype=torch.int64)
        self.n = int(offsets.numel()) - 1
        self.n_bases = int(offsets[-1]) if self.n >= 0 else 0
        if self.n < 1:
            raise ValueError("ResidentSplit: an empty split")
        if int(offsets[0]) != 0 or bool((offsets[1:] < offsets[:-1]).any()) \
                or self.n_bases != len(bases):
            raise ValueError("ResidentSplit: offsets do not partition the bases")
        if len(targets) != self.n:
            raise ValueError(f"ResidentSplit: {len(targets)} targets for {self.n} sequences")
        lut = torch.as_tensor(lut, dtype=torch.int64)
        if lut.shape != (256,) or int(lut.min()) < 0:
            raise ValueError("ResidentSplit: the id table is int64 [256], non-negative")
        self.max_length = int(max_length)
        self.pad_id, self.eos_id, self.pad_left = int(pad_id), int(eos_id), bool(pad_left)
        self.return_mask, self.rc_aug, self.rng = bool(return_mask), bool(rc_aug), rng
        if self.max_length < 1 or self.pad_id < 0:
            raise ValueError("ResidentSplit: max_length >= 1 and pad_id >= 0")
        up = lambda t: t.to(self.device)
        # one spare byte: an all-empty split still has a buffer to point at (it is never read)
        self.bases = up(torch.frombuffer(bytearray(bases) + b"\0", dtype=torch.uint8))
        self.offsets, self.targets, self.lut = up(offsets), up(targets.contiguous()), up(lut)
        self.comp = up(torch.from_numpy(complement_table()))
        self._order = self._flags = None
        self.set_epoch(range(self.n), rc_flags=[False] * self.n if self.rc_aug else None)

    @classmethod
    def from_dataset(cls, ds, device):
        """Any finetune_data._CharItems dataset (its `pairs()`, tokenizer, max_length, add_eos,
        id_remap, rc_aug / rng, return_mask). use_padding=False gives ragged items with no fixed
        length: refused."""
        if not getattr(ds, "use_padding", True):
            raise ValueError("ResidentSplit: use_padding=False gives ragged items with no fixed "
                             "length; a resident split builds [batch, max_length] rectangles only")
        tok = ds.tokenizer
        if not hasattr(tok, "_lut"):
            raise TypeError(f"ResidentSplit: {type(tok).__name__} is no character tokenizer "
                            "(one id per byte)")
        lut = torch.from_numpy(np.asarray(tok._lut, dtype=np.int64).copy())
        pad, eos = torch.tensor(tok.pad_token_id), torch.tensor(tok.sep_token_id)
        if bool((lut == tok.pad_token_id).any()):
            raise ValueError("ResidentSplit: a character tokenises to [PAD]; the mask would "
                             "differ from the item-by-item path's")
        if ds.id_remap:
            lut, pad, eos = remap_ids(lut), remap_ids(pad), remap_ids(eos)
        chunks, lens, targets = [], [], []
        for seq, target in ds.pairs():
            b = seq.encode("latin-1", errors="replace")  # CharacterTokenizer.encode_raw's bytes
            chunks.append(b)
            lens.append(len(b))
            targets.append(torch.as_tensor(target))
        if not chunks:
            raise ValueError("ResidentSplit: an empty split")
        offsets = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(np.asarray(lens, dtype=np.int64), out=offsets[1:])
        return cls(b"".join(chunks), torch.from_numpy(offsets), torch.stack(targets), lut,
                   ds.max_length, int(pad), int(eos) if ds.add_eos else -1,
                   tok.padding_side == "left", return_mask=ds.return_mask, rc_aug=ds.rc_aug,
                   rng=ds.rng, device=device)

    def __len__(self):
        return self.n

    def set_epoch(self, order, rc_flags=None):
        """The epoch's item order (any sequence of indices, repeats allowed), checked on the host
        against [0, N) and uploaded once. rc_flags: one flag per entry of `order`; None draws
        them from the dataset's random.Random when the dataset has rc_aug -- one draw per item
        in this order, as item-by-item access would -- and means the forward strand otherwise."""
        order = torch.as_tensor(list(order) if isinstance(order, range) else order,
                                dtype=torch.int64).reshape(-1)
        if order.numel() and (int(order.min()) < 0 or int(order.max()) >= self.n):
            raise IndexError(f"ResidentSplit.set_epoch: order has entries outside [0, {self.n})")
        if rc_flags is None and self.rc_aug:
            rc_flags = [self.rng.random() < 0.5 for _ in range(order.numel())]
        if rc_flags is not None:
            rc_flags = torch.as_tensor(rc_flags, dtype=torch.bool).reshape(-1)
            if rc_flags.numel() != order.numel():
                raise ValueError(f"ResidentSplit.set_epoch: {rc_flags.numel()} rc flags for "
                                 f"{order.numel()} items")
            rc_flags = rc_flags.to(torch.uint8).to(self.device)
        self._order, self._flags = order.to(self.device), rc_flags

    def batch(self, start, stop):
        """Items order[start:stop] of the epoch -> (ids, targets[, mask]) on the device: one
        kernel launch and an index_select, on the current stream."""
        start, stop = max(0, int(start)), min(int(stop), int(self._order.numel()))
        if stop <= start:
            raise IndexError(f"ResidentSplit.batch: empty range [{start}, {stop})")
        idx = self._order[start:stop]
        b, L = stop - start, self.max_length
        ids = torch.empty((b, L), dtype=torch.int64, device=self.device)
        mask = torch.empty((b, L), dtype=torch.bool, device=self.device) if self.return_mask else None
        N.call("dna_char_batch", self.bases.data_ptr(), self.n_bases, self.offsets.data_ptr(),
               self.n, idx.data_ptr(), N.ptr(None if self._flags is None else self._flags[start:stop]),
               self.lut.data_ptr(), self.comp.data_ptr(), b, L, int(self.pad_left), self.pad_id,
               self.eos_id, ids.data_ptr(), N.ptr(mask), N.stream_ptr(self.device))
        targets = self.targets.index_select(0, idx)
        return (ids, targets, mask) if self.return_mask else (ids, targets)


class ResidentWindows:
    """A split of finetune_data.SpeciesWindows or ChromatinProfile whose genome is on the device
    (genome.GenomeStore.to): `batch(start, stop)` cuts rows [start, stop) of the current pass out
    of it with `dna_genome_windows` (csrc/genome_windows.hip), integer-exact with
    `collate([ds[j] ...])`. The interface is ResidentSplit's (__len__, set_epoch, batch).

    Every decision stays on the host and only (src, n, left) per row goes up. A species split
    draws a pass's windows at set_epoch -- three draws per entry of `order`, in order, from the
    dataset's own random.Random, as that many accesses would (the entries themselves are ignored,
    as the dataset ignores its index) -- so finetune.evaluate starts each pass with set_epoch, and
    a train epoch followed by the val and test passes consumes a shared rng as item-by-item
    access does. (A pass cut short, train.max_steps, has still drawn all its windows.) A
    chromatin split's rows are fixed: they are computed and checked once here, and set_epoch
    uploads the order alone."""

    def __init__(self, ds, store):
        """ds: the dataset (its rows / window_spec / row_length); store: ds.store.to(device)."""
        self.ds, self.store, self.device = ds, store, store.device
        if store.n_bases != ds.store.n_bases:
            raise ValueError("ResidentWindows: the store is not the dataset's own")
        self.n_bases, self.L = store.n_bases, int(ds.row_length)
        lut, self.fill_id, self.eos_id, self.tail_id = ds.window_spec()
        if lut.shape != (256,) or int(lut.min()) < 0 or self.fill_id < 0:
            raise ValueError("ResidentWindows: the id table is int64 [256], non-negative")
        self.lut = lut.to(self.device)
        self.redraws = bool(ds.redraws)
        if not self.redraws:
            src, n, left, right = ds.rows()
            if bool((left + n + right != self.L - 1).any()):
                bad = int((left + n + right != self.L - 1).nonzero()[0])
                raise ValueError(f"ResidentWindows: item {bad} is {int((left + n + right)[bad])} "
                                 f"characters long, not {self.L - 1}; a resident split builds "
                                 "rectangles only (intervals of one length)")
            self._check(src, n, left)
            self._all = tuple(t.to(self.device) for t in (src, n, left))
            self.targets = ds.labels.to(self.device)
        self._rows = self._targets = self._order = None
        self._count = len(ds)
        if not self.redraws:
            self.set_epoch()

    @classmethod
    def from_dataset(cls, ds, device):
        return cls(ds, ds.store.to(device))

    def _check(self, src, n, left):
        """What the kernel would write as fill is an error here, before anything is uploaded."""
        if src.numel() and (int(src.min()) < 0 or int(n.min()) < 0 or int(left.min()) < 0
                            or int((src + n).max()) > self.n_bases):
            raise ValueError("ResidentWindows: a window lies outside the genome store")

    def __len__(self):
        return len(self.ds)

    def device_bytes(self):
        """Bytes this split holds on the device between batches."""
        held = [self.store.bases, self.lut] + list(self._rows or ()) + \
            ([] if self.redraws else list(self._all) + [self.targets]) + \
            ([self._targets] if self._targets is not None else [])
        return sum(t.numel() * t.element_size() for t in held)

    def set_epoch(self, order=None):
        """Starts a pass of len(order) rows (None: one per item, in the dataset's order)."""
        if self.redraws:
            k = len(self.ds) if order is None else len(order)
            src, n, left, tgt = self.ds.rows(k)
            self._check(src, n, left)
            self._rows = tuple(t.to(self.device) for t in (src, n, left))
            self._targets, self._order, self._count = tgt.to(self.device), None, k
            return
        if order is None:
            self._rows, self._order, self._count = self._all, None, len(self.ds)
            return
        order = torch.as_tensor(list(order) if isinstance(order, range) else order,
                                dtype=torch.int64).reshape(-1)
        if order.numel() and (int(order.min()) < 0 or int(order.max()) >= len(self.ds)):
            raise IndexError(f"ResidentWindows.set_epoch: order has entries outside "
                             f"[0, {len(self.ds)})")
        self._order = order.to(self.device)
        self._rows = tuple(t.index_select(0, self._order) for t in self._all)
        self._count = int(order.numel())

    def batch(self, start, stop):
        """Rows [start, stop) of the pass -> (ids int64 [b, row_length], targets) on the device."""
        if self._rows is None:
            raise RuntimeError("ResidentWindows.batch before set_epoch: no windows are drawn yet")
        start, stop = max(0, int(start)), min(int(stop), self._count)
        if stop <= start:
            raise IndexError(f"ResidentWindows.batch: empty range [{start}, {stop})")
        src, n, left = (t[start:stop] for t in self._rows)
        b = stop - start
        ids = torch.empty((b, self.L), dtype=torch.int64, device=self.device)
        N.call("dna_genome_windows", self.store.bases.data_ptr(), self.n_bases, src.data_ptr(),
               n.data_ptr(), left.data_ptr(), self.lut.data_ptr(), b, self.L, self.fill_id,
               self.eos_id, ids.data_ptr(), N.stream_ptr(self.device))
        if self.tail_id >= 0:  # a window runs off a right end: [SEP] stands after the fill
            ids[:, self.L - 1] = self.tail_id
        if self.redraws:
            return ids, self._targets[start:stop]
        idx = (self._order[start:stop] if self._order is not None
               else torch.arange(start, stop, device=self.device))
        return ids, self.targets.index_select(0, idx).to(torch.float32)


RESIDENT = (ResidentSplit, ResidentWindows)
