"""The lists after a removal by label (ivfhnsw_gpu_remove_ids, IndexIVF_HNSW::remove_ids), restated in
numpy: every code whose id is one of the labels leaves its list, the others keep their order; on Grouping lists each
sub-group loses the codes it held."""
import numpy as np


def filter_lists(offsets, ids, codes, norm_codes, labels, subgroup_sizes=None):
    """dict(offsets, ids, codes, norm_codes, removed [nc] [, subgroup_sizes [nc, nsubc]]) after remove_ids(labels)."""
    off = np.asarray(offsets, np.int64)
    nc = len(off) - 1
    ids = np.asarray(ids, np.uint32)
    drop = np.isin(ids, np.asarray(labels, np.uint32).ravel())
    keep = ~drop
    lid = np.repeat(np.arange(nc), np.diff(off))
    rem = np.bincount(lid[drop], minlength=nc).astype(np.uint32)
    noff = np.concatenate([[0], np.cumsum(np.diff(off) - rem)]).astype(np.uint64)
    codes = np.asarray(codes).reshape(len(ids), -1)
    out = dict(offsets=noff, ids=ids[keep], codes=np.ascontiguousarray(codes[keep]),
               norm_codes=np.asarray(norm_codes, np.uint8)[keep], removed=rem)
    if subgroup_sizes is not None:
        sg = np.asarray(subgroup_sizes, np.int64).reshape(nc, -1)
        sub_of_row = np.repeat(np.arange(sg.size), sg.ravel())  # flat (list, sub-group) of every row, in CSR order
        rsg = np.bincount(sub_of_row[drop], minlength=sg.size).reshape(sg.shape)
        out["subgroup_sizes"] = (sg - rsg).astype(np.uint32)
    return out


def filtered_corpus(c, labels):
    """Corpus dict c (tests/synth.py) with the labels removed from its lists: (corpus, filter_lists result)."""
    f = filter_lists(c["offsets"], c["ids"], c["codes"], c["norm_codes"], labels,
                     c.get("subgroup_sizes") if c.get("nsubc") else None)
    out = dict(c, offsets=f["offsets"], ids=f["ids"], codes=f["codes"], norm_codes=f["norm_codes"])
    if "subgroup_sizes" in f:
        out["subgroup_sizes"] = f["subgroup_sizes"]
    return out, f
