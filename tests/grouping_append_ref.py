"""The lists of a Grouping index after codes were added to sub-groups (ivfhnsw_gpu_append_grouping, IndexIVF_HNSW_
Grouping.cpp:127-155), restated in numpy the slow, obvious way: a list is its nsubc sub-groups end to
end; new code i goes to the end of sub-group sub_idx[i] of list list_idx[i], codes of one sub-group keep ascending i."""
import numpy as np


def merge_lists(offsets, ids, codes, norm_codes, subgroup_sizes, list_idx, sub_idx, new_ids, new_codes, new_norm_codes):
    """dict(offsets u64 [nc+1], ids, codes, norm_codes, subgroup_sizes u32 [nc, nsubc]) after the append."""
    off = np.asarray(offsets, np.int64)
    nc = len(off) - 1
    sg = np.asarray(subgroup_sizes, np.int64).reshape(nc, -1)
    nsubc = sg.shape[1]
    ids = np.asarray(ids, np.uint32)
    codes = np.asarray(codes, np.uint8).reshape(len(ids), -1)
    norm_codes = np.asarray(norm_codes, np.uint8)
    li = np.asarray(list_idx, np.int64).ravel()
    si = np.asarray(sub_idx, np.int64).ravel()
    new_ids = np.asarray(new_ids, np.uint32).ravel()
    new_codes = np.asarray(new_codes, np.uint8)
    new_codes = new_codes.reshape(len(li), -1) if len(li) else np.zeros((0, codes.shape[1]), np.uint8)
    new_norm_codes = np.asarray(new_norm_codes, np.uint8).ravel()
    assert (sg.sum(1) == np.diff(off)).all() and (li < nc).all() and (si < nsubc).all()
    o_ids, o_codes, o_nc = [], [], []
    sg2 = sg.copy()
    for c in range(nc):
        a = int(off[c])
        mine = np.nonzero(li == c)[0]
        for s in range(nsubc):
            b = a + int(sg[c, s])
            add = mine[si[mine] == s]      # ascending i
            o_ids += [ids[a:b], new_ids[add]]
            o_codes += [codes[a:b], new_codes[add]]
            o_nc += [norm_codes[a:b], new_norm_codes[add]]
            sg2[c, s] += len(add)
            a = b
    noff = np.concatenate([[0], np.cumsum(sg2.sum(1))]).astype(np.uint64)
    M = codes.shape[1] if codes.size or not new_codes.size else new_codes.shape[1]
    return dict(offsets=noff, ids=np.concatenate(o_ids).astype(np.uint32),
                codes=np.ascontiguousarray(np.concatenate(o_codes).reshape(-1, M)),
                norm_codes=np.concatenate(o_nc).astype(np.uint8), subgroup_sizes=sg2.astype(np.uint32))


def rows_of(offsets, subgroup_sizes):
    """(list, sub-group) of every row of the CSR arrays."""
    sg = np.asarray(subgroup_sizes, np.int64)
    nc, nsubc = sg.shape
    flat = np.repeat(np.arange(sg.size), sg.ravel())
    return flat // nsubc, flat % nsubc


def tail_mask(c, rng, whole=0.15, none=0.15, skip_lists=0.1, whole_lists=0.1):
    """Rows to hold back so that appending them again restores c: a tail of random length of every sub-group (about
    half its rows on average; the whole sub-group for a share `whole`, nothing for a share `none`), every row of a share
    `whole_lists` of the lists and nothing at all from a share `skip_lists` of them."""
    sg = np.asarray(c["subgroup_sizes"], np.int64)
    nc, nsubc = sg.shape
    u = rng.random(sg.shape)
    take = np.floor(rng.random(sg.shape) * (sg + 1)).astype(np.int64)
    take = np.where(u < whole, sg, np.where(u < whole + none, 0, take))
    v = rng.random(nc)
    take[v < whole_lists] = sg[v < whole_lists]
    take[v > 1.0 - skip_lists] = 0
    within = np.arange(int(sg.sum())) - np.repeat(np.cumsum(sg.ravel()) - sg.ravel(), sg.ravel())
    return within >= np.repeat((sg - take).ravel(), sg.ravel())


def split_corpus(c, held):
    """Corpus dict c (tests/synth.py) without the rows of the boolean mask `held`: (the reduced corpus, the batch
    dict(list_idx, sub_idx, ids, codes, norm_codes) that holds them, in CSR order)."""
    lst, sub = rows_of(c["offsets"], c["subgroup_sizes"])
    keep = ~held
    nc, nsubc = c["subgroup_sizes"].shape
    sg = np.bincount(lst[keep] * nsubc + sub[keep], minlength=nc * nsubc).reshape(nc, nsubc).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(sg.sum(1))]).astype(np.uint64)
    codes = np.asarray(c["codes"]).reshape(len(c["ids"]), -1)
    part = dict(c, offsets=off, ids=c["ids"][keep].copy(), codes=np.ascontiguousarray(codes[keep]),
                norm_codes=c["norm_codes"][keep].copy(), subgroup_sizes=sg)
    batch = dict(list_idx=lst[held].astype(np.uint32), sub_idx=sub[held].astype(np.uint32), ids=c["ids"][held].copy(),
                 codes=np.ascontiguousarray(codes[held]), norm_codes=c["norm_codes"][held].copy())
    return part, batch


def without_groups(c, gone):
    """Corpus dict c with the groups of the boolean mask `gone` [nc] emptied: their rows leave the lists and their rows
    of the four grouping tables are zero.  Returns (the reduced corpus, the held rows' mask)."""
    lst, _ = rows_of(c["offsets"], c["subgroup_sizes"])
    held = gone[lst]
    part, _ = split_corpus(c, held)
    for k in ("alphas", "nn_centroid_idxs", "inter_centroid_dists"):
        t = c[k].copy()
        t[gone] = 0
        part[k] = t
    return part, held
