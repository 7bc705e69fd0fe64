"""The in-place updates of the resident lists at the smallest shapes that reach every branch of the copy they share
(csrc/update_steps.h): appends (3.10), removals (3.11) and Grouping appends (3.12) on CSR arrays built
directly with numpy -- no oracle and no graph -- compared byte for byte with numpy's answer: download_ivf, and the
sub-group size table of a Grouping handle.

Code sizes 4, 12, 16 and 28 make a row 1, 3, 4 and 7 dwords: rows that are a fraction of a 16-byte group, that straddle
groups, that are one group, and that are no whole number of groups.  The appends end at 2047, 2048, 2049 and 4096 rows (a
tile is 2048 rows: a last group in part, a full tile, a second tile of one row, two full tiles), put 2100 rows into one
list (a tile of new rows only: every source a hole), fill a handle of empty lists, and grow the last list alone.  The
removals empty a whole tile, match nothing, leave 2045, 2046 and 2047 rows in the first tile (so the second tile's range
starts at each non-zero offset into a 16-byte group) and remove everything.  The Grouping appends run nsubc 64 over 4
long lists (the tile's prefix sums cached in LDS) and over 256 short ones (more than 16 lists to a tile: searched in
global memory), leave lists and sub-groups untouched, and fill sub-groups of size 0.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048
CODE_SIZES = [4, 12, 16, 28]


def _rows(rng, n, M, first_id):
    """n rows: distinct ids from first_id up (shuffled), random codes and norm codes."""
    ids = (first_id + rng.permutation(n)).astype(np.uint32)
    return ids, rng.integers(0, 256, (n, M), dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)


def _lists(rng, lens, M):
    lens = np.asarray(lens, np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return (off,) + _rows(rng, int(lens.sum()), M, 0)


def _upload(gpu, lists, M):
    off, ids, codes, ncodes = lists
    nc, d = len(off) - 1, 4 * M
    g = gpu()
    g.upload_ivf(d, M, off, ids, codes, ncodes, np.zeros(nc, np.float32), np.zeros(256 * d, np.float32),
                 np.zeros(256, np.float32))
    return g


def _assert_lists(g, want):
    off, ids, codes, ncodes = g.download_ivf()
    assert np.array_equal(off, want[0])
    assert np.array_equal(ids, want[1])
    assert np.array_equal(ncodes, want[3])
    assert np.array_equal(codes, want[2])


def _split_into(rng, total, nparts):
    """nparts non-negative integers that sum to total."""
    cuts = np.sort(rng.integers(0, total + 1, nparts - 1))
    return np.diff(np.concatenate([[0], cuts, [total]]))


def np_append(lists, batch, sizes=None, sub=None):
    """Every list's old rows and then its batch rows in arrival order; with sizes [nc, nsubc] and sub the same inside
    every sub-group.  Returns (lists, new sizes)."""
    off, ids, codes, ncodes = lists
    lid, bids, bcodes, bncodes = batch
    nc = len(off) - 1
    order = []  # (from the batch, row)
    lens = []
    for c in range(nc):
        old = np.arange(int(off[c]), int(off[c + 1]))
        new = np.nonzero(lid == c)[0]
        if sizes is None:
            parts = [(0, old), (1, new)]
        else:
            parts, at = [], 0
            for s in range(sizes.shape[1]):
                parts += [(0, old[at:at + sizes[c, s]]), (1, new[sub[new] == s])]
                at += int(sizes[c, s])
        order += parts
        lens.append(len(old) + len(new))
    pick = lambda a, b: np.concatenate([(b if w else a)[r] for w, r in order]) if order else a[:0]
    new_sizes = None
    if sizes is not None:
        new_sizes = sizes.copy()
        np.add.at(new_sizes, (lid, sub), 1)
    out = (np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), pick(ids, bids), pick(codes, bcodes), pick(ncodes, bncodes))
    return out, new_sizes


def np_remove(lists, labels):
    off, ids, codes, ncodes = lists
    keep = ~np.isin(ids, labels)
    lid = np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))
    lens = np.bincount(lid[keep], minlength=len(off) - 1)
    removed = np.bincount(lid[~keep], minlength=len(off) - 1).astype(np.uint32)
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), ids[keep], codes[keep], ncodes[keep]), removed


# ---- appends --------------------------------------------------------------------------------------------------
def _append_case(rng, case, M):
    """(old list lengths, list ids of the batch) of one case; nc = 8."""
    nc = 8
    if isinstance(case, int):  # n_local after the append
        n_old = case * 3 // 5
        lens = _split_into(rng, n_old, nc)
        lens[2] = 0 if lens[2] < 50 else lens[2]
        lid = rng.integers(0, nc, case - int(lens.sum()))
    elif case == "one_list":   # one tile holds nothing but new rows
        lens = _split_into(rng, 700, nc)
        lid = np.full(2100, 3)
    elif case == "empty":
        lens = np.zeros(nc, np.int64)
        lid = rng.integers(0, nc, 3000)
    else:                      # only the last list grows
        lens = _split_into(rng, 2500, nc)
        lid = np.full(900, nc - 1)
    return lens, lid.astype(np.uint32)


@pytest.mark.parametrize("M", CODE_SIZES)
@pytest.mark.parametrize("case", [2047, 2048, 2049, 4096, "one_list", "empty", "last_list"])
def test_append(gpu, case, M):
    rng = np.random.default_rng(1000 + M)
    lens, lid = _append_case(rng, case, M)
    lists = _lists(rng, lens, M)
    batch = (lid,) + _rows(rng, len(lid), M, 1 << 20)
    g = _upload(gpu, lists, M)
    g.append_ivf(*batch)
    want, _ = np_append(lists, batch)
    if isinstance(case, int):
        assert len(want[1]) == case
    _assert_lists(g, want)


# ---- removals -------------------------------------------------------------------------------------------------
def _remove_rows(rng, case, n):
    """The rows (positions in the local arrays) a case removes."""
    if case == "tile":                         # tile 1 keeps nothing
        return np.arange(TILE - 48, 2 * TILE + 152)
    if case == "none":
        return np.zeros(0, np.int64)
    if case == "all":
        return np.arange(n)
    first = rng.choice(TILE, TILE - case, replace=False)            # the first tile keeps `case` rows
    rest = TILE + np.nonzero(rng.random(n - TILE) < 0.3)[0]
    return np.concatenate([first, rest])


@pytest.mark.parametrize("M", CODE_SIZES)
@pytest.mark.parametrize("case", ["tile", "none", 2045, 2046, 2047, "all"])
def test_remove(gpu, case, M):
    rng = np.random.default_rng(2000 + M)
    lists = _lists(rng, _split_into(rng, 3 * TILE + 300, 8), M)
    rows = _remove_rows(rng, case, len(lists[1]))
    labels = lists[1][rows] if case != "none" else np.arange(1 << 21, (1 << 21) + 500, dtype=np.uint32)
    labels = rng.permutation(np.concatenate([labels, labels[:7]]))  # any order, repeats allowed
    g = _upload(gpu, lists, M)
    n_removed, per_list = g.remove_ids(labels)
    want, removed = np_remove(lists, labels)
    if isinstance(case, int):
        assert int(np.isin(lists[1][:TILE], labels).sum()) == TILE - case
    assert n_removed == len(rows) and np.array_equal(per_list, removed)
    _assert_lists(g, want)


# ---- Grouping appends -----------------------------------------------------------------------------------------
NSUBC = 64


def _grouping_case(rng, shape):
    """(sizes [nc, nsubc], the batch's (list, sub-group) ids).  Every third list and every fifth sub-group stay untouched,
    list 1 holds only empty sub-groups, a quarter of the others are empty too, and the batch targets them all."""
    nc, per = (4, 24) if shape == "long" else (256, 1)
    sizes = rng.integers(0, 2 * per + 1, (nc, NSUBC))
    sizes[rng.random((nc, NSUBC)) < 0.25] = 0
    sizes[1] = 0
    lists_t = np.array([c for c in range(nc) if c % 3 != 2])
    subs_t = np.array([s for s in range(NSUBC) if s % 5 != 4])
    n = 1200 if shape == "long" else 1500
    n += -(int(sizes.sum()) + n) % 4   # the new n_local is a multiple of 4
    return sizes.astype(np.uint32), rng.choice(lists_t, n).astype(np.uint32), rng.choice(subs_t, n).astype(np.uint32)


def _upload_grouping(gpu, lists, sizes, M):
    g = _upload(gpu, lists, M)
    nc = sizes.shape[0]
    g.upload_grouping(NSUBC, np.ones(nc, np.float32), np.zeros((nc, NSUBC), np.uint32), sizes,
                      np.zeros((nc, NSUBC), np.float32))
    return g


@pytest.mark.parametrize("M", CODE_SIZES)
@pytest.mark.parametrize("shape", ["long", "short"])
def test_append_grouping(gpu, shape, M):
    rng = np.random.default_rng(3000 + M)
    sizes, lid, sub = _grouping_case(rng, shape)
    lists = _lists(rng, sizes.sum(1), M)
    batch = (lid,) + _rows(rng, len(lid), M, 1 << 20)
    # the shapes reach what they are for: lists per tile on both sides of the 1024 cached prefix sums
    lists_per_tile = TILE / (sizes.sum() / sizes.shape[0])
    assert lists_per_tile * NSUBC < 1024 / 2 if shape == "long" else lists_per_tile > 16
    assert (sizes[lid, sub] == 0).any() and (len(lists[1]) + len(lid)) % 4 == 0
    g = _upload_grouping(gpu, lists, sizes, M)
    g.append_grouping(lid, sub, *batch[1:])
    want, new_sizes = np_append(lists, batch, sizes, sub)
    _assert_lists(g, want)
    assert np.array_equal(g.download_grouping(), new_sizes)


# ---- cross-checks ---------------------------------------------------------------------------------------------
def test_append_then_remove_restores(gpu):
    M = 12
    rng = np.random.default_rng(7)
    lists = _lists(rng, _split_into(rng, 2 * TILE + 77, 8), M)
    lid = rng.integers(0, 8, 1500).astype(np.uint32)
    batch = (lid,) + _rows(rng, len(lid), M, 1 << 20)
    g = _upload(gpu, lists, M)
    g.append_ivf(*batch)
    n_removed, per_list = g.remove_ids(batch[1])
    assert n_removed == len(lid) and np.array_equal(per_list, np.bincount(lid, minlength=8))
    _assert_lists(g, lists)


def test_dev_forms_equal_host_forms(gpu):
    import torch
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to(dev)
    M = 28
    rng = np.random.default_rng(8)
    sizes, lid, sub = _grouping_case(rng, "long")
    lists = _lists(rng, sizes.sum(1), M)
    batch = (lid,) + _rows(rng, len(lid), M, 1 << 20)
    labels = rng.permutation(np.concatenate([lists[1][100:2300], batch[1][::3]]))
    # IVFADC handle: append, then remove
    host, devh = _upload(gpu, lists, M), _upload(gpu, lists, M)
    host.append_ivf(*batch)
    devh.append_ivf_dev(len(lid), *[to_dev(a) for a in batch])
    n_host, per_host = host.remove_ids(labels)
    d_per = torch.zeros(len(sizes), dtype=torch.int32, device=dev)
    assert devh.remove_ids_dev(len(labels), to_dev(labels), d_per) == n_host == len(labels)
    assert np.array_equal(d_per.cpu().numpy().view(np.uint32), per_host)
    _assert_lists(devh, host.download_ivf())
    _assert_lists(host, np_remove(np_append(lists, batch)[0], labels)[0])
    # Grouping handle: append
    host, devh = _upload_grouping(gpu, lists, sizes, M), _upload_grouping(gpu, lists, sizes, M)
    host.append_grouping(lid, sub, *batch[1:])
    devh.append_grouping_dev(len(lid), to_dev(lid), to_dev(sub), *[to_dev(a) for a in batch[1:]])
    _assert_lists(devh, host.download_ivf())
    assert np.array_equal(devh.download_grouping(), host.download_grouping())
    _assert_lists(host, np_append(lists, batch, sizes, sub)[0])
