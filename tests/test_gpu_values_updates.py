"""Row values through in-place updates: one handle goes through set_values in pieces, appends, add,
removal, an upsert, re-valuing, un-valuing and clear_values; after every step search_values and range_search_values equal a
fresh handle that uploaded the lists the handle holds and set the values of the assignment as it stands, every result's
value lies in its query's interval, values_info / value_rows equal numpy counts, and memory_bytes moves by the contract's
formula around every set_values and clear_values."""
import numpy as np
import pytest

import values_ref as vr
from test_gpu_filter_slots import base
from test_gpu_remove import BASE, GROUPING, _upload, _same_search, _with_ids

pytestmark = pytest.mark.gpu

NONE = vr.NONE
EXTRA = [(7, 7), (150, 0x80000000), (NONE, NONE)]  # intervals counted beside the pattern's


def _set(asg, labels, values):
    """The assignment after set_values(labels, values): dict label -> value, NONE entries dropped."""
    for l, v in zip(np.asarray(labels).tolist(), np.asarray(values).tolist()):
        if v == NONE:
            asg.pop(l, None)
        else:
            asg[l] = v
    return asg


def _arrays(asg):
    labels = np.array(sorted(asg), np.uint32)
    return labels, np.array([asg[int(l)] for l in labels], np.uint32)


def _count(rv, r):
    v = rv.astype(np.uint64)
    return int(((v >= r[0]) & (v <= r[1])).sum())


def _set_values(g, labels, values, span):
    """g.set_values with memory_bytes checked against the formula; returns the new span."""
    had = g.values_info()
    mem = g.memory_bytes()
    g.set_values(labels, values)
    new = max(span, int(np.asarray(labels).max()) + 1)
    assert had[2] == span
    assert g.memory_bytes() - mem == 4 * (new - span) + (0 if span else 4 * max(had[1], 1))
    return new


def _check(gpu, g, c, asg, span, params=vr.IVF_PARAMS, prunings=(False,)):
    """g against a fresh handle on g's own lists with the assignment's values; span: label values g's table must cover."""
    labels, values = _arrays(asg)
    off, ids, codes, ncodes = g.download_ivf()
    f = gpu()
    f.upload_ivf(c["d"], c["code_size"], off, ids, codes, ncodes, c["centroid_norms"], c["pq_centroids"], c["norm_table"],
                 opq_A=c["opq_A"])
    if c.get("nsubc"):
        f.upload_grouping(c["nsubc"], *g.download_grouping_tables())
    gr = c["graph"]
    f.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    if len(labels):
        f.set_values(labels, values)
    rv = vr.row_values(ids, (labels, values)) if len(labels) else np.full(len(ids), NONE, np.uint32)
    assert g.values_info() == (int((rv != NONE).sum()), len(ids), span)
    for r in vr.PATTERN + EXTRA:
        assert g.value_rows(*r) == f.value_rows(*r) == _count(rv, r), r
    q = c["queries"]
    qr = vr.query_ranges(len(q))
    nprobe, mc, ef = params
    for pruning in prunings:
        for k, heap in ((1, False), (10, True)):
            got = g.search_values(q, k, qr, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=heap)
            assert g.last_scan_kernel().endswith("+values")
            assert _same_search(got, f.search_values(q, k, qr, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=heap)), \
                (pruning, k)
            lab = got[1]
            found = lab >= 0
            lv = np.full(lab.shape, NONE, np.uint64)
            if len(labels):
                lv[found] = vr.row_values(lab[found].astype(np.uint32), (labels, values))
            lo = np.broadcast_to(qr[:, :1].astype(np.uint64), lab.shape)
            hi = np.broadcast_to(qr[:, 1:].astype(np.uint64), lab.shape)
            assert ((lv >= lo) & (lv <= hi))[found].all(), "a result's value lies outside its query's interval"
        tenth = f.search(q, 10, nprobe, mc, efSearch=ef, do_pruning=pruning)[0][:, 9]
        radius = float(np.median(tenth))
        a = g.range_search_values(q, radius, qr, nprobe, mc, efSearch=ef, do_pruning=pruning)
        b = f.range_search_values(q, radius, qr, nprobe, mc, efSearch=ef, do_pruning=pruning)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    f.close()
    return got


def test_ivf_sequence(gpu, pkg):
    b = base(**BASE)
    rng = np.random.default_rng(31)
    nc, M = b["nc"], b["code_size"]
    g = _upload(gpu(), b)
    g.upload_codebooks(b["d"], M, b["pq_centroids"], b["norm_table"], b["opq_A"])
    full = vr.assignment(b)
    labels, values = vr.valued(full)
    asg, span = {}, 0
    # set_values in three incremental calls: each leaves the other labels' values alone
    for p in range(3):
        span = _set_values(g, labels[p::3], values[p::3], span)
        _set(asg, labels[p::3], values[p::3])
        _check(gpu, g, b, asg, span)
    band = vr.PATTERN[3]
    assert g.value_rows(*band) == int(vr.passing_rows(b, full, band).sum())
    # append_ivf: rows whose labels were given a value before they arrived ...
    n = 3000
    early = (np.arange(n) + 10 ** 6).astype(np.uint32)
    early_values = np.where(np.arange(n) % 2 == 0, 0x80000000, 0xfffffffe).astype(np.uint32)
    span = _set_values(g, early, early_values, span)
    _set(asg, early, early_values)
    assert span == 10 ** 6 + n and g.values_info()[2] == span
    before = g.value_rows(0x80000000, 0x80000000)

    def batch(ids):
        return (rng.integers(0, nc, len(ids)).astype(np.uint32), ids, rng.integers(0, 256, (len(ids), M)).astype(np.uint8),
                rng.integers(0, 255, len(ids)).astype(np.uint8))
    # a failing update leaves the values as they were
    def answers():
        return g.search_values(b["queries"], 10, vr.query_ranges(len(b["queries"])), *vr.IVF_PARAMS[:2], efSearch=vr.IVF_PARAMS[2])
    probe = answers()
    bad = batch(early)
    bad[0][n // 2] = nc
    with pytest.raises(pkg.IvfHnswError) as e:
        g.append_ivf(*bad)
    assert e.value.code == pkg.ERR_INVALID and g.value_rows(0x80000000, 0x80000000) == before
    assert _same_search(answers(), probe)
    g.append_ivf(*batch(early))
    assert g.value_rows(0x80000000, 0x80000000) == before + n // 2
    _check(gpu, g, b, asg, span)
    # ... and rows whose labels were not (beyond the table, and inside it)
    late = np.concatenate([np.arange(2 * 10 ** 6, 2 * 10 ** 6 + 1000), np.arange(500000, 501000)]).astype(np.uint32)
    without = g.value_rows(NONE, NONE)
    g.append_ivf(*batch(late))
    assert g.value_rows(NONE, NONE) == without + len(late)
    _check(gpu, g, b, asg, span)
    # add: the new labels get their values first, one small call
    x = b["base"][:2000] + np.float32(0.5)
    added = (np.arange(len(x)) + 3 * 10 ** 6).astype(np.uint32)
    span = _set_values(g, added[::4], np.full(len(added[::4]), 0x10000, np.uint32), span)
    _set(asg, added[::4], np.full(len(added[::4]), 0x10000, np.uint32))
    rows16 = g.value_rows(0x10000, 0x10000)
    g.add(x, added, efSearch=40)
    assert g.value_rows(0x10000, 0x10000) == rows16 + len(added[::4])
    _check(gpu, g, b, asg, span)
    # remove_ids: rows with and without a value alike; the labels keep their values (label space, not row space)
    ids_now = g.download_ivf()[1]
    gone = rng.choice(np.unique(ids_now), 6000, replace=False)
    assert g.remove_ids(gone)[0] == 6000
    _check(gpu, g, b, asg, span)
    # upsert_ivf: half of the labels resident, half new; the values stay with the labels
    ids_now = np.unique(g.download_ivf()[1])
    resident = rng.choice(ids_now, 1000, replace=False).astype(np.uint32)
    fresh = (np.arange(1000) + 4 * 10 ** 6).astype(np.uint32)  # beyond the table: no value
    both = np.concatenate([resident, fresh])
    # a label twice in the batch: refused, and the values answer as before
    twice = batch(np.concatenate([both, both[:1]]))
    counts = {r: g.value_rows(*r) for r in vr.PATTERN}
    probe = answers()
    with pytest.raises(pkg.IvfHnswError) as e:
        g.upsert_ivf(*twice)
    assert e.value.code == pkg.ERR_INVALID and {r: g.value_rows(*r) for r in vr.PATTERN} == counts
    assert _same_search(answers(), probe)
    rows_before = g.values_info()[1]
    assert g.upsert_ivf(*batch(both))[0] == 1000
    assert g.values_info()[1] == rows_before + 1000
    _check(gpu, g, b, asg, span)
    # re-valuing: 100 labels to another value, 100 to NONE
    mine = vr.labels_in(full, band)
    mine = mine[np.isin(mine, np.unique(g.download_ivf()[1]))][:200]
    assert len(mine) == 200
    new_values = np.concatenate([np.full(100, 7, np.uint32), np.full(100, NONE, np.uint32)])
    rows_band, rows7 = g.value_rows(*band), g.value_rows(7, 7)
    span = _set_values(g, mine, new_values, span)
    _set(asg, mine, new_values)
    assert g.value_rows(*band) == rows_band - 200 and g.value_rows(7, 7) == rows7 + 100
    _check(gpu, g, b, asg, span)
    # clear_values: the table and the row values of the rows as they stand now go
    rows_now = g.values_info()[1]
    mem = g.memory_bytes()
    g.clear_values()
    assert mem - g.memory_bytes() == 4 * span + 4 * rows_now
    g.clear_values()  # nothing to clear: succeeds
    _check(gpu, g, b, {}, 0)
    qr = vr.query_ranges(len(b["queries"]))
    got = g.search_values(b["queries"], 1, qr, *vr.IVF_PARAMS[:2], efSearch=vr.IVF_PARAMS[2])
    assert (got[1][qr[:, 1] != NONE] == -1).all() and (got[1][vr.mine(qr, vr.FULL)] >= 0).all()
    # upload_ivf drops the values too
    vr.install(g, full)
    assert g.values_info()[2] > 0
    _upload(g, b, graph=False)
    assert g.values_info() == (0, len(b["ids"]), 0)


def test_grouping_sequence(gpu):
    import grouping_append_ref as gar
    import test_gpu_add_groups as tg
    params = (tg.NPROBE, tg.MAX_CODES, tg.EF)
    # append_grouping and remove_ids
    c = base(**GROUPING[1])
    part, batch = gar.split_corpus(c, gar.tail_mask(c, np.random.default_rng(9)))
    g = _upload(gpu(), part)
    full = vr.assignment(c)
    labels, values = vr.valued(full)
    asg = _set({}, labels, values)
    span = _set_values(g, labels, values, 0)  # the tails' labels get their values before their rows arrive
    _check(gpu, g, c, asg, span, params=vr.GROUPING_PARAMS, prunings=(False, True))
    tg._append(g, batch)
    band = vr.PATTERN[3]
    assert g.values_info()[1] == len(c["ids"]) and g.value_rows(*band) == int(vr.passing_rows(c, full, band).sum())
    _check(gpu, g, c, asg, span, params=vr.GROUPING_PARAMS, prunings=(False, True))
    gone = np.random.default_rng(15).choice(c["ids"], len(c["ids"]) // 4, replace=False)
    g.remove_ids(gone)
    _check(gpu, g, c, asg, span, params=vr.GROUPING_PARAMS, prunings=(False, True))
    # add_groups
    c, g0, groups, gone, rng = tg._group_case(tg.SHAPES[1], 21)
    whole = tg._assemble(c, g0, groups)
    part, _ = gar.without_groups(whole, gone)
    part["subgroup_sizes"][gone] = 0
    g = tg._upload_for_add(gpu, c, g0, part)
    full = vr.assignment(whole, seed=0)
    labels, values = vr.valued(full)
    asg = _set({}, labels, values)
    span = _set_values(g, labels, values, 0)
    tg._add_groups(g, groups, rng.permutation(np.nonzero(gone)[0]))
    tg._assert_state(g, whole)
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    assert g.value_rows(*band) == int(vr.passing_rows(whole, full, band).sum())
    _check(gpu, g, dict(whole, queries=c["queries"], graph=c["graph"]), asg, span, params=params, prunings=(False, True))


def test_label_held_in_many_rows(gpu):
    b0 = base(**BASE)
    b = _with_ids(b0, b0["ids"] % 700)  # every label in ~40 rows spread over many lists
    g = _upload(gpu(), b)
    labels = np.arange(700, dtype=np.uint32)
    values = np.where(labels % 3 == 0, 0x80000000 + labels, np.where(labels % 3 == 1, 0, NONE)).astype(np.uint32)
    g.set_values(labels[values != NONE], values[values != NONE])
    rv = values[b["ids"]]
    assert g.values_info() == (int((rv != NONE).sum()), len(rv), 700)
    assert g.value_rows(0x80000000, 0x800000ff) == int(((rv >= 0x80000000) & (rv <= 0x800000ff)).sum()) > 3000
    _check(gpu, g, b, _set({}, labels, values), 700)


def test_user_view_before_and_after_set_values(gpu, pkg):
    """A view reads what its parent held when the view was made: none before set_values, the values after it."""
    b = base(**BASE)
    g = _upload(gpu(), b)
    q = b["queries"]
    qr = vr.query_ranges(len(q))
    early = g.view()
    bare = g.search_values(q, 1, qr, *vr.IVF_PARAMS[:2], efSearch=vr.IVF_PARAMS[2])
    vr.install(g, vr.assignment(b))
    late = g.view()
    assert late.values_info() == g.values_info() and late.value_rows(77, 77) == g.value_rows(77, 77) > 0
    assert early.values_info() == (0, len(b["ids"]), 0)
    for k in (1, 10):
        want = g.search_values(q, k, qr, *vr.IVF_PARAMS[:2], efSearch=vr.IVF_PARAMS[2])
        assert _same_search(late.search_values(q, k, qr, *vr.IVF_PARAMS[:2], efSearch=vr.IVF_PARAMS[2]), want)
        assert late.last_scan_kernel().endswith("+values")
    assert not _same_search(bare, g.search_values(q, 1, qr, *vr.IVF_PARAMS[:2], efSearch=vr.IVF_PARAMS[2]))
    assert _same_search(early.search_values(q, 1, qr, *vr.IVF_PARAMS[:2], efSearch=vr.IVF_PARAMS[2]), bare)
    early.close()
    late.close()


def test_dev_forms_and_upsert_from_vectors(gpu):
    """The _dev forms of the updates and upsert from raw vectors go through the same hook: append_ivf_dev, add_dev, upsert,
    upsert_dev and remove_ids_dev each leave the handle answering as a fresh upload of its lists with the same values."""
    import torch
    dev = torch.device("cuda", 0)
    b = base(**BASE)
    rng = np.random.default_rng(77)
    nc, M = b["nc"], b["code_size"]
    g = _upload(gpu(), b)
    g.upload_codebooks(b["d"], M, b["pq_centroids"], b["norm_table"], b["opq_A"])
    full = vr.assignment(b)
    labels, values = vr.valued(full)
    asg = _set({}, labels, values)
    # labels that arrive later: half of each batch has a value before its rows exist
    new = {name: (np.arange(600) + first).astype(np.uint32) for name, first in
           (("append", 10 ** 6), ("add", 2 * 10 ** 6), ("upsert", 3 * 10 ** 6), ("upsert_dev", 4 * 10 ** 6))}
    early = np.concatenate([ids[::2] for ids in new.values()])
    early_values = (0x7fffff80 + np.arange(len(early)) % 256).astype(np.uint32)  # inside the band across the sign bit
    span = _set_values(g, np.concatenate([labels, early]), np.concatenate([values, early_values]), 0)
    _set(asg, early, early_values)
    band = vr.PATTERN[3]

    def t32(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)

    # append_ivf_dev
    n = 600
    li, codes, ncodes = (rng.integers(0, nc, n).astype(np.uint32), rng.integers(0, 256, (n, M)).astype(np.uint8),
                         rng.integers(0, 255, n).astype(np.uint8))
    d_li, d_ids, d_codes, d_nc = t32(li), t32(new["append"]), torch.from_numpy(codes).to(dev), torch.from_numpy(ncodes).to(dev)
    torch.cuda.synchronize(dev)
    rows_band = g.value_rows(*band)
    g.append_ivf_dev(n, d_li, d_ids, d_codes, d_nc)
    g.sync()
    assert g.value_rows(*band) == rows_band + 300
    _check(gpu, g, b, asg, span)
    # add_dev
    x = (b["base"][:n] + np.float32(0.5)).astype(np.float32)
    d_x, d_ids = torch.from_numpy(x).to(dev), t32(new["add"])
    torch.cuda.synchronize(dev)
    rows_band = g.value_rows(*band)
    g.add_dev(n, d_x, d_ids, efSearch=40)
    g.sync()
    assert g.value_rows(*band) == rows_band + 300
    _check(gpu, g, b, asg, span)
    # upsert from raw vectors: 600 new labels and 600 resident ones, whose values stay with the labels
    resident = rng.choice(np.unique(b["ids"]), 600, replace=False).astype(np.uint32)
    both = np.concatenate([new["upsert"], resident])
    x2 = (b["base"][rng.integers(0, len(b["base"]), len(both))] + rng.normal(0, 3.0, (len(both), b["d"]))).astype(np.float32)
    rows_before = g.values_info()[1]
    assert g.upsert(x2, both, efSearch=40)[3] == 600
    assert g.values_info()[1] == rows_before + 600
    _check(gpu, g, b, asg, span)
    # upsert_dev: the same labels' vectors replaced once more, and 600 new labels
    both = np.concatenate([new["upsert_dev"], resident])
    d_x, d_ids = torch.from_numpy(x2[::-1].copy()).to(dev), t32(both)
    torch.cuda.synchronize(dev)
    assert g.upsert_dev(len(both), d_x, d_ids, efSearch=40) == 600
    g.sync()
    assert g.values_info()[1] == rows_before + 1200
    _check(gpu, g, b, asg, span)
    # remove_ids_dev: the labels keep their values, the rows go
    gone = np.concatenate([new["append"][:300], resident[:300]])
    d_gone = t32(gone)
    torch.cuda.synchronize(dev)
    assert g.remove_ids_dev(len(gone), d_gone) == 600
    g.sync()
    assert g.values_info()[1] == rows_before + 600
    _check(gpu, g, b, asg, span)
