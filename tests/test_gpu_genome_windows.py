"""dna_genome_windows (csrc/genome_windows.hip) against a numpy restatement of its row rule,
integer-exact, and resident.ResidentWindows against the item-by-item path of the two datasets it
serves (torch.equal on ids and targets, same seeds)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import genome_fixtures as GF  # noqa: E402

pytestmark = pytest.mark.gpu

N_BASES, FILL = 20001, 5


def _restate(bases, src, n, left, lut, L, fill, eos):
    """fill x left | lut[bases[src + j]], j < n | eos (if any) | fill ..., cut at L; a row with
    src < 0, n < 0, left < 0 or src + n > len(bases) is all fill."""
    out = np.full((len(src), L), fill, dtype=np.int64)
    for r, (s, k, l) in enumerate(zip(src, n, left)):
        if s < 0 or k < 0 or l < 0 or s + k > len(bases):
            continue
        row = [fill] * l + lut[bases[s:s + k]].tolist() + ([eos] if eos >= 0 else [])
        row = row[:L]
        out[r, :len(row)] = row
    return out


@pytest.fixture(scope="module")
def genome():
    rng = np.random.default_rng(11)
    bases = rng.integers(0, 256, N_BASES, dtype=np.uint8)
    lut = rng.integers(6, 40, 256).astype(np.int64)
    dev = torch.device("cuda", 0)
    return bases, lut, torch.from_numpy(bases).to(dev), torch.from_numpy(lut).to(dev)


def _launch(dbases, n_bases, dlut, src, n, left, L, fill, eos):
    from dna_amd import _native as N
    dev = dbases.device
    up = lambda a, dt: torch.tensor(list(a), dtype=dt, device=dev)
    s, k, l = up(src, torch.int64), up(n, torch.int32), up(left, torch.int32)
    ids = torch.full((len(src), L), -7, dtype=torch.int64, device=dev)  # no cell keeps this
    N.call("dna_genome_windows", dbases.data_ptr(), n_bases, s.data_ptr(), k.data_ptr(),
           l.data_ptr(), dlut.data_ptr(), len(src), L, fill, eos, ids.data_ptr(),
           N.stream_ptr(dev))
    return ids.cpu().numpy()


def _valid_rows(L):
    """(src, n, left) of every valid kind the row rule distinguishes."""
    return [
        (100, L, 0),                      # left = 0, n = L: all bases (an eos is cut off)
        (200, 5, L),                      # left = L: all fill
        (300, 0, min(3, L - 1)),          # n = 0: fill, then the eos directly
        (400, L - 1, 0),                  # the eos lands in the last cell
        (0, min(L, 77), 0),               # src = 0
        (N_BASES - min(L, 50), min(L, 50), 0),  # src + n = n_bases: the last byte is read
        (7, max(L // 3, 1), 1 if L > 1 else 0),  # odd src, fill on both sides
        (1001, L, L // 2),                # left + n > L: the bases are cut
        (N_BASES, 0, 0),                  # an empty window at the very end is valid
    ]


INVALID = [(-1, 4, 0), (50, -1, 0), (50, 4, -1), (N_BASES - 2, 5, 0), (2 ** 33, 1, 0)]


@pytest.mark.parametrize("eos", [-1, 1])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("L", [1, 63, 64, 257, 8193])
def test_kernel_equals_the_row_rule(genome, L, B, eos):
    bases, lut, dbases, dlut = genome
    valid = _valid_rows(L)
    if B == 1:
        groups = [[row] for row in valid + INVALID]
    else:  # every invalid kind sits between valid rows of the same launch
        groups = [valid[i:i + B] for i in range(0, len(valid), B)]
        groups += [[valid[i % len(valid)], valid[(i + 3) % len(valid)], bad,
                    valid[(i + 5) % len(valid)], valid[(i + 6) % len(valid)]]
                   for i, bad in enumerate(INVALID)]
    for rows in groups:
        src, n, left = zip(*rows)
        got = _launch(dbases, N_BASES, dlut, src, n, left, L, FILL, eos)
        want = _restate(bases, src, n, left, lut, L, FILL, eos)
        assert np.array_equal(got, want), (rows, np.argwhere(got != want)[:4].tolist())
        for r, row in enumerate(rows):
            if row in INVALID:
                assert (got[r] == FILL).all(), row


def test_offsets_past_two_to_the_31(genome):
    """A store larger than 2^31 bytes: windows whose src, and whose src + n, lie past 2^31."""
    _, lut, _, dlut = genome
    dev = dlut.device
    big = 2 ** 31 + 8192
    dbases = torch.zeros(big, dtype=torch.uint8, device=dev)
    tail = np.random.default_rng(5).integers(1, 256, 8192 + 300, dtype=np.uint8)
    dbases[big - len(tail):] = torch.from_numpy(tail).to(dev)
    first = big - len(tail)
    rows = [(first + 1, 257, 3), (2 ** 31 - 100, 257, 0), (big - 64, 64, 10), (big - 63, 64, 0)]
    src, n, left = zip(*rows)
    got = _launch(dbases, big, dlut, src, n, left, 300, FILL, 1)
    host = {s: (tail[s - first:s - first + k] if s >= first else
                np.concatenate([np.zeros(first - s, np.uint8), tail])[:k]) for s, k, _ in rows}
    for r, (s, k, l) in enumerate(rows):
        if s + k > big:
            assert (got[r] == FILL).all()
            continue
        want = ([FILL] * l + lut[host[s]].tolist() + [1] + [FILL] * 300)[:300]
        assert got[r].tolist() == want, r
    del dbases


# ------------------------------------------------------------------------------------ resident
def _species_splits(root, gold, seed, add_eos, tails, use_tokenizer):
    from dna_amd.finetune_data import SpeciesWindows
    rng = random.Random(seed)  # one generator for the three splits
    return {s: SpeciesWindows(gold["species"], root, s, gold["max_length"], size, add_eos=add_eos,
                              remove_tail_ends=tails, rng=rng, use_tokenizer=use_tokenizer)
            for s, size in (("train", 48), ("valid", 24), ("test", 16))}


@pytest.fixture(scope="module")
def species(tmp_path_factory):
    root = tmp_path_factory.mktemp("species")
    return GF.species_folder(root), str(root)


@pytest.mark.parametrize("use_tokenizer", [True, False])
@pytest.mark.parametrize("add_eos,tails", [(True, False), (False, True)])
def test_resident_species_equals_the_item_path(species, add_eos, tails, use_tokenizer):
    """One shuffled train epoch, then a val and a test pass, all on one rng."""
    from dna_amd.resident import ResidentWindows
    gold, root = species
    dev = torch.device("cuda", 0)
    host = _species_splits(root, gold, 31, add_eos, tails, use_tokenizer)
    twin = _species_splits(root, gold, 31, add_eos, tails, use_tokenizer)
    res = {k: ResidentWindows.from_dataset(v, dev) for k, v in twin.items()}
    assert res["train"].store.names == twin["train"].store.names  # its own chromosomes only
    assert res["train"].store.n_bases < sum(len(t) for t in gold["fasta"].values())
    order = torch.randperm(48, generator=torch.Generator().manual_seed(3))
    for name, bs in (("train", 10), ("valid", 7), ("test", 16)):
        ds, rs = host[name], res[name]
        idx = order.tolist() if name == "train" else list(range(len(ds)))
        rs.set_epoch(order if name == "train" else None)
        assert len(rs) == len(ds)
        for i in range(0, len(idx), bs):
            want_ids, want_t = ds.collate([ds[j] for j in idx[i:i + bs]])
            ids, t = rs.batch(i, i + bs)
            assert ids.device.type == "cuda" and ids.dtype == torch.int64
            assert torch.equal(ids.cpu(), want_ids) and torch.equal(t.cpu(), want_t), (name, i)
    assert host["train"].rng.random() == twin["train"].rng.random()  # the same draws consumed
    assert res["train"].device_bytes() > res["train"].store.n_bases


@pytest.mark.parametrize("use_tokenizer", [True, False])
@pytest.mark.parametrize("max_length", [512, 1024, 1100])
def test_resident_chromatin_equals_the_item_path(tmp_path, max_length, use_tokenizer):
    from dna_amd.finetune_data import ChromatinProfile
    from dna_amd.resident import ResidentWindows
    gold, fa = GF.chromatin_folder(tmp_path, splits=("train",))
    ds = ChromatinProfile(str(tmp_path), fa, "hg38", "train", max_length,
                          use_tokenizer=use_tokenizer)
    rs = ResidentWindows.from_dataset(ds, torch.device("cuda", 0))
    for order in (None, [8, 0, 3, 3, 7, 1, 4, 2, 6, 5, 0]):
        rs.set_epoch(order)
        idx = list(range(len(ds))) if order is None else order
        for i in range(0, len(idx), 4):
            want_ids, want_t = ds.collate([ds[j] for j in idx[i:i + 4]])
            ids, t = rs.batch(i, i + 4)
            assert torch.equal(ids.cpu(), want_ids), (order, i)
            assert t.dtype == torch.float32 and torch.equal(t.cpu(), want_t), (order, i)
    with pytest.raises(IndexError):
        rs.set_epoch([9])
    with pytest.raises(IndexError):
        rs.batch(11, 12)


def test_resident_windows_refuses_what_it_cannot_build(tmp_path):
    """Items of unequal length (an interval cut at max_length that also runs off the end)."""
    from dna_amd.finetune_data import ChromatinProfile
    from dna_amd.resident import ResidentWindows
    gold = GF.load("chromatin_golden.json")
    lines = gold["csv"].splitlines()
    lines[2] = lines[2].replace(",0,300,1300,", ",0,200,1400,")  # 1,200 bases, 100 past the end
    GF.chromatin_folder(tmp_path, gold=dict(gold, csv="\n".join(lines) + "\n"), splits=("train",))
    ds = ChromatinProfile(str(tmp_path), os.path.join(str(tmp_path), "genome.fa"), "hg38",
                          "train", 1000)
    assert len({len(ds[i][0]) for i in range(len(ds))}) > 1
    with pytest.raises(ValueError, match="rectangles"):
        ResidentWindows.from_dataset(ds, torch.device("cuda", 0))
