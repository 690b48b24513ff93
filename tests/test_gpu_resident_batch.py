"""resident.ResidentSplit.batch (csrc/char_batch.hip) against the item-by-item path it replaces:
torch.equal with `collate([ds[j] for j in order])` of the same _CharItems dataset. Integer-exact:
ids, mask and targets are integers or copies, so there is no tolerance anywhere."""
import itertools
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ACGTN, lowercase, an IUPAC letter, a line end, a latin-1 character and a non-latin-1 one
ALPHABET = "ACGTNacgtR\né€"


class _Coins:
    """Stands in for the dataset's random.Random: random() < 0.5 exactly where a flag is set."""

    def __init__(self, flags):
        self.flags = list(flags)

    def random(self):
        return 0.0 if self.flags.pop(0) else 1.0


def _toy(seqs, targets, **kw):
    from dna_amd.finetune_data import _CharItems
    from dna_amd.tokenizer import CharacterTokenizer

    class Toy(_CharItems):
        def __init__(self):
            side = kw.pop("padding_side", "left")
            tok = CharacterTokenizer(["A", "C", "G", "T", "N"], kw["max_length"] + 2,
                                     padding_side=side)
            self._init_items(kw.pop("max_length"), tok, kw.pop("use_padding", True),
                             kw.pop("add_eos", False), kw.pop("rc_aug", False),
                             kw.pop("return_mask", False), kw.pop("rng", None),
                             kw.pop("id_remap", False))
            assert not kw, kw

        def __len__(self):
            return len(seqs)

        def _pair(self, i):
            return seqs[i], targets[i]

    return Toy()


def _seqs(L):
    """Three sequences (each starting elsewhere in the alphabet) of every length that matters at
    max_length L: empty, one base, one short of L, exact fit, one over, more than twice over. The
    last one is the longest, so a reversed read of it touches the last byte of the split."""
    out = []
    for n in (0, 1, L - 1, L, L + 1, 2 * L + 3):
        for phase in (0, 4, 9):
            out.append("".join(ALPHABET[(phase + 3 * j + j // 7) % len(ALPHABET)] for j in range(n)))
    return out


def _orders(n):
    # B = 1: the split's last sequence. B = 130 (more rows than a wave has lanes, and more than
    # one workgroup's): reverse order with repeats, holding the last sequence.
    return {1: [n - 1], 130: [n - 1 - (i * 7) % n for i in range(130)]}


def _flags(kind, b):
    return {"off": [False] * b, "on": [True] * b, "mixed": [(5 * i + 1) % 3 == 0 for i in range(b)]}[kind]


@pytest.mark.parametrize("L", [1, 5, 64, 200, 513])
def test_batch_equals_item_by_item_collate(L):
    from dna_amd.resident import ResidentSplit
    seqs = _seqs(L)
    targets = [torch.tensor(i % 3, dtype=torch.int64) for i in range(len(seqs))]
    orders = _orders(len(seqs))
    for side, eos, remap in itertools.product(("left", "right"), (False, True), (False, True)):
        cfg = dict(max_length=L, padding_side=side, add_eos=eos, id_remap=remap)
        splits = {m: ResidentSplit.from_dataset(_toy(seqs, targets, return_mask=m, **cfg), DEV)
                  for m in (False, True)}
        for (b, order), rc in itertools.product(orders.items(), ("off", "on", "mixed")):
            flags = _flags(rc, b)
            ref_ds = _toy(seqs, targets, return_mask=True, rc_aug=rc != "off",
                          rng=_Coins(flags), **cfg)
            want = ref_ds.collate([ref_ds[j] for j in order])
            for with_mask, split in splits.items():
                split.set_epoch(order, rc_flags=None if rc == "off" else flags)
                got = split.batch(0, b)
                what = (L, side, eos, remap, b, rc, with_mask)
                assert len(got) == (3 if with_mask else 2), what
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and g.shape == w.shape, what
                    assert torch.equal(g.cpu(), w), what


def test_batch_ranges_within_an_epoch():
    """batch(start, stop) reads order[start:stop] and its flags; the last range may be short."""
    from dna_amd.resident import ResidentSplit
    L = 64
    seqs = _seqs(L)
    targets = [torch.tensor(i, dtype=torch.int64) for i in range(len(seqs))]
    order = _orders(len(seqs))[130]
    flags = _flags("mixed", 130)
    ref_ds = _toy(seqs, targets, max_length=L, rc_aug=True, rng=_Coins(flags))
    split = ResidentSplit.from_dataset(_toy(seqs, targets, max_length=L), DEV)
    split.set_epoch(order, rc_flags=flags)
    for start in range(0, 130, 48):
        ids, labels = split.batch(start, start + 48)
        want_ids, want_labels = ref_ds.collate([ref_ds[j] for j in order[start:start + 48]])
        assert torch.equal(ids.cpu(), want_ids) and torch.equal(labels.cpu(), want_labels), start


@pytest.mark.parametrize("kind", ["int64", "fp32x3"])
def test_targets(kind):
    from dna_amd.resident import ResidentSplit
    seqs = _seqs(5)
    if kind == "int64":
        targets = [torch.tensor(i % 4, dtype=torch.int64) for i in range(len(seqs))]
    else:
        targets = list(torch.arange(len(seqs) * 3, dtype=torch.float32).reshape(-1, 3) / 7)
    ds = _toy(seqs, targets, max_length=5)
    split = ResidentSplit.from_dataset(ds, DEV)
    order = _orders(len(seqs))[130]
    split.set_epoch(order)
    ids, got = split.batch(0, 130)
    want_ids, want = ds.collate([ds[j] for j in order])
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got.cpu(), want) and torch.equal(ids.cpu(), want_ids)


def test_one_epoch_with_seeded_shuffle_and_rc_aug():
    """The loop's contract: the same permutation and the same dataset seed give, step by step, the
    (ids, labels) the item-by-item path builds."""
    from dna_amd.resident import ResidentSplit
    L, bs = 64, 16
    seqs = _seqs(L) * 3
    targets = [torch.tensor(i % 2, dtype=torch.int64) for i in range(len(seqs))]
    mk = lambda: _toy(seqs, targets, max_length=L, rc_aug=True, rng=random.Random(5))
    ref_ds, split = mk(), ResidentSplit.from_dataset(mk(), DEV)
    for epoch in range(2):
        order = torch.randperm(len(seqs), generator=torch.Generator().manual_seed(11 + epoch))
        split.set_epoch(order)
        order = order.tolist()
        for i in range(0, len(order), bs):
            want_ids, want_labels = ref_ds.collate([ref_ds[j] for j in order[i:i + bs]])
            ids, labels = split.batch(i, i + bs)
            assert torch.equal(ids.cpu(), want_ids) and torch.equal(labels.cpu(), want_labels), \
                (epoch, i)


def test_bad_input_raises_on_the_host():
    from dna_amd.resident import ResidentSplit
    seqs = _seqs(5)
    targets = [torch.tensor(0, dtype=torch.int64)] * len(seqs)
    with pytest.raises(ValueError, match="use_padding=False"):
        ResidentSplit.from_dataset(_toy(seqs, targets, max_length=5, use_padding=False), DEV)
    split = ResidentSplit.from_dataset(_toy(seqs, targets, max_length=5), DEV)
    for bad in ([0, len(seqs)], [-1, 0]):
        with pytest.raises(IndexError, match="outside"):
            split.set_epoch(bad)
    with pytest.raises(ValueError, match="rc flags"):
        split.set_epoch([0, 1], rc_flags=[True])
    # the refused epochs left the split as it was: the identity order of construction
    assert split.batch(0, 2)[0].shape == (2, 5)
