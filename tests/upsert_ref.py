"""The lists after an upsert (ivfhnsw_gpu_upsert_ivf), restated in numpy: remove_ref.filter_lists of the
batch's labels, then batch code i appended to the end of list list_idx[i], the batch codes of one list in ascending i."""
import numpy as np

import remove_ref


def upsert_lists(offsets, ids, codes, norm_codes, list_idx, new_ids, new_codes, new_norm_codes):
    """dict(offsets, ids, codes, norm_codes, removed [nc]) after upsert_ivf(list_idx, new_ids, new_codes, new_norm_codes)."""
    new_ids = np.asarray(new_ids, np.uint32).ravel()
    assert len(np.unique(new_ids)) == len(new_ids), "a label twice in one batch has no upsert"
    li = np.asarray(list_idx, np.int64).ravel()
    n = len(li)
    nc = len(offsets) - 1
    if len(ids):
        f = remove_ref.filter_lists(offsets, ids, codes, norm_codes, new_ids)
    else:           # an index without codes (filter_lists reads the code size off the resident codes): the batch alone
        f = dict(offsets=np.zeros(nc + 1, np.uint64), ids=np.zeros(0, np.uint32), codes=np.zeros((0, 0), np.uint8),
                 norm_codes=np.zeros(0, np.uint8), removed=np.zeros(nc, np.uint32))
    M = f["codes"].shape[1] if f["codes"].size else np.asarray(new_codes).reshape(n, -1).shape[1]
    new_codes = np.asarray(new_codes, np.uint8).reshape(n, M)
    new_norm = np.asarray(new_norm_codes, np.uint8).ravel()
    old_list = np.repeat(np.arange(nc), np.diff(f["offsets"].astype(np.int64)))
    # stable: old rows (in order) lead every list, the batch's rows (ascending i) follow
    lst = np.concatenate([old_list, li])
    order = np.argsort(lst, kind="stable")
    cnt = np.bincount(lst, minlength=nc)
    return dict(offsets=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64),
                ids=np.concatenate([f["ids"], new_ids])[order],
                codes=np.ascontiguousarray(np.concatenate([f["codes"].reshape(-1, M), new_codes])[order]),
                norm_codes=np.concatenate([f["norm_codes"], new_norm])[order], removed=f["removed"])


def upserted_corpus(c, list_idx, new_ids, new_codes, new_norm_codes):
    """Corpus dict c (tests/synth.py) after the upsert: (corpus, upsert_lists result)."""
    u = upsert_lists(c["offsets"], c["ids"], c["codes"], c["norm_codes"], list_idx, new_ids, new_codes, new_norm_codes)
    return dict(c, offsets=u["offsets"], ids=u["ids"], codes=u["codes"], norm_codes=u["norm_codes"]), u
