"""Row tags through in-place updates: one handle goes through set_tags in pieces, appends, add, removal,
re-tagging and clear_tags; after every step search_tags and range_search_tags equal a fresh handle that uploaded the lists
the handle holds and set the tags of the assignment as it stands, and tags_info / tag_rows equal numpy counts."""
import numpy as np
import pytest

import tags_ref as tr
from test_gpu_filter_slots import base
from test_gpu_remove import BASE, GROUPING, _upload, _same_search, _with_ids

pytestmark = pytest.mark.gpu

NONE = tr.NONE


def _set(asg, labels, tags):
    """The assignment after set_tags(labels, tags): dict label -> tag, NONE entries dropped."""
    for l, t in zip(np.asarray(labels).tolist(), np.asarray(tags).tolist()):
        if t == NONE:
            asg.pop(l, None)
        else:
            asg[l] = t
    return asg


def _arrays(asg):
    labels = np.array(sorted(asg), np.uint32)
    return labels, np.array([asg[int(l)] for l in labels], np.uint16)


def _check(gpu, g, c, asg, span, params=tr.IVF_PARAMS, prunings=(False,)):
    """g against a fresh handle on g's own lists with the assignment's tags; span: label values g's table must cover."""
    labels, tags = _arrays(asg)
    off, ids, codes, ncodes = g.download_ivf()
    f = gpu()
    f.upload_ivf(c["d"], c["code_size"], off, ids, codes, ncodes, c["centroid_norms"], c["pq_centroids"], c["norm_table"],
                 opq_A=c["opq_A"])
    if c.get("nsubc"):
        f.upload_grouping(c["nsubc"], *g.download_grouping_tables())
    gr = c["graph"]
    f.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    if len(labels):
        f.set_tags(labels, tags)
    rt = tr.row_tags(ids, (labels, tags)) if len(labels) else np.full(len(ids), NONE, np.uint16)
    assert g.tags_info() == (int((rt != NONE).sum()), len(ids), span)
    for t in sorted(set(tr.PATTERN) | {7}):
        assert g.tag_rows(t) == f.tag_rows(t) == int((rt == t).sum()), t
    q = c["queries"]
    qt = tr.query_tags(len(q))
    nprobe, mc, ef = params
    for pruning in prunings:
        for k, heap in ((1, False), (10, True)):
            got = g.search_tags(q, k, qt, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=heap)
            assert g.last_scan_kernel().endswith("+tags")
            assert _same_search(got, f.search_tags(q, k, qt, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=heap)), \
                (pruning, k)
            lab = got[1]
            found = lab >= 0
            want = np.broadcast_to(qt[:, None], lab.shape)
            lt = np.full(lab.shape, NONE, np.uint16)
            if len(labels):
                lt[found] = tr.row_tags(lab[found].astype(np.uint32), (labels, tags))
            assert ((lt == want) | (want == NONE))[found].all(), "a result carries another tag than its query's"
        tenth = f.search(q, 10, nprobe, mc, efSearch=ef, do_pruning=pruning)[0][:, 9]
        radius = float(np.median(tenth))
        a = g.range_search_tags(q, radius, qt, nprobe, mc, efSearch=ef, do_pruning=pruning)
        b = f.range_search_tags(q, radius, qt, nprobe, mc, efSearch=ef, do_pruning=pruning)
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
    full = tr.assignment(b)
    labels, tags = tr.tagged(full)
    asg, span = {}, 0
    # set_tags in three incremental calls: each leaves the other labels' tags alone
    for p in range(3):
        g.set_tags(labels[p::3], tags[p::3])
        _set(asg, labels[p::3], tags[p::3])
        span = max(span, int(labels[p::3].max()) + 1)
        _check(gpu, g, b, asg, span)
    assert g.tag_rows(0) == int(tr.passing_rows(b, full, 0).sum())
    # append_ivf: rows whose labels were tagged before they arrived ...
    n = 3000
    early = (np.arange(n) + 10 ** 6).astype(np.uint32)
    early_tags = np.where(np.arange(n) % 2 == 0, 0, 0xfffe).astype(np.uint16)
    g.set_tags(early, early_tags)
    _set(asg, early, early_tags)
    span = 10 ** 6 + n
    assert g.tags_info()[2] == span
    before0 = g.tag_rows(0)

    def batch(ids):
        return (rng.integers(0, nc, len(ids)).astype(np.uint32), ids, rng.integers(0, 256, (len(ids), M)).astype(np.uint8),
                rng.integers(0, 255, len(ids)).astype(np.uint8))
    # a failing update leaves the tags as they were
    bad = batch(early)
    bad[0][n // 2] = nc
    with pytest.raises(pkg.IvfHnswError) as e:
        g.append_ivf(*bad)
    assert e.value.code == pkg.ERR_INVALID and g.tag_rows(0) == before0
    g.append_ivf(*batch(early))
    assert g.tag_rows(0) == before0 + n // 2
    _check(gpu, g, b, asg, span)
    # ... and rows whose labels were not (beyond the table, and inside it)
    late = np.concatenate([np.arange(2 * 10 ** 6, 2 * 10 ** 6 + 1000), np.arange(500000, 501000)]).astype(np.uint32)
    untagged = g.tag_rows(NONE)
    g.append_ivf(*batch(late))
    assert g.tag_rows(NONE) == untagged + len(late)
    _check(gpu, g, b, asg, span)
    # add: the new labels are tagged first, one small call
    x = b["base"][:2000] + np.float32(0.5)
    added = (np.arange(len(x)) + 3 * 10 ** 6).astype(np.uint32)
    g.set_tags(added[::4], np.full(len(added[::4]), 256, np.uint16))
    _set(asg, added[::4], np.full(len(added[::4]), 256, np.uint16))
    span = int(added[::4].max()) + 1
    rows256 = g.tag_rows(256)
    g.add(x, added, efSearch=40)
    assert g.tag_rows(256) == rows256 + len(added[::4])
    _check(gpu, g, b, asg, span)
    # remove_ids: tagged and untagged rows alike; the labels keep their tags (label space, not row space)
    ids_now = g.download_ivf()[1]
    gone = rng.choice(np.unique(ids_now), 6000, replace=False)
    assert g.remove_ids(gone)[0] == 6000
    _check(gpu, g, b, asg, span)
    # re-tagging: 100 labels to another tag, 100 to NONE (the soft delete)
    mine = tr.labels_of(full, 0)
    mine = mine[~np.isin(mine, gone)][:200]
    new_tags = np.concatenate([np.full(100, 255, np.uint16), np.full(100, NONE, np.uint16)])
    rows0 = g.tag_rows(0)
    g.set_tags(mine, new_tags)
    _set(asg, mine, new_tags)
    assert g.tag_rows(0) == rows0 - 200
    _check(gpu, g, b, asg, span)
    # clear_tags
    g.clear_tags()
    g.clear_tags()  # nothing to clear: succeeds
    _check(gpu, g, b, {}, 0)
    got = g.search_tags(b["queries"], 1, tr.query_tags(len(b["queries"])), *tr.IVF_PARAMS[:2], efSearch=tr.IVF_PARAMS[2])
    assert (got[1][tr.query_tags(len(b["queries"])) != NONE] == -1).all()
    # upload_ivf drops the tags too
    tr.install(g, full)
    assert g.tags_info()[2] > 0
    _upload(g, b, graph=False)
    assert g.tags_info() == (0, len(b["ids"]), 0)


def test_grouping_sequence(gpu):
    import grouping_append_ref as gar
    import test_gpu_add_groups as tg
    params = (tg.NPROBE, tg.MAX_CODES, tg.EF)
    # append_grouping and remove_ids
    c = base(**GROUPING[1])
    part, batch = gar.split_corpus(c, gar.tail_mask(c, np.random.default_rng(9)))
    g = _upload(gpu(), part)
    full = tr.assignment(c)
    labels, tags = tr.tagged(full)
    asg = _set({}, labels, tags)
    g.set_tags(labels, tags)  # the tails' labels are tagged before their rows arrive
    span = int(labels.max()) + 1
    _check(gpu, g, c, asg, span, params=tr.GROUPING_PARAMS, prunings=(False, True))
    tg._append(g, batch)
    assert g.tags_info()[1] == len(c["ids"]) and g.tag_rows(0) == int(tr.passing_rows(c, full, 0).sum())
    _check(gpu, g, c, asg, span, params=tr.GROUPING_PARAMS, prunings=(False, True))
    gone = np.random.default_rng(15).choice(c["ids"], len(c["ids"]) // 4, replace=False)
    g.remove_ids(gone)
    _check(gpu, g, c, asg, span, params=tr.GROUPING_PARAMS, prunings=(False, True))
    # add_groups
    c, g0, groups, gone, rng = tg._group_case(tg.SHAPES[1], 21)
    whole = tg._assemble(c, g0, groups)
    part, _ = gar.without_groups(whole, gone)
    part["subgroup_sizes"][gone] = 0
    g = tg._upload_for_add(gpu, c, g0, part)
    full = tr.assignment(whole, seed=0)
    labels, tags = tr.tagged(full)
    asg = _set({}, labels, tags)
    g.set_tags(labels, tags)
    span = int(labels.max()) + 1
    tg._add_groups(g, groups, rng.permutation(np.nonzero(gone)[0]))
    tg._assert_state(g, whole)
    gr = c["graph"]
    g.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    assert g.tag_rows(0) == int(tr.passing_rows(whole, full, 0).sum())
    _check(gpu, g, dict(whole, queries=c["queries"], graph=c["graph"]), asg, span, params=params, prunings=(False, True))


def test_label_held_in_many_rows(gpu):
    b0 = base(**BASE)
    b = _with_ids(b0, b0["ids"] % 700)  # every label in ~40 rows spread over many lists
    g = _upload(gpu(), b)
    labels = np.arange(700, dtype=np.uint32)
    tags = np.where(labels % 3 == 0, 0, np.where(labels % 3 == 1, 0xfffe, NONE)).astype(np.uint16)
    g.set_tags(labels[tags != NONE], tags[tags != NONE])
    rt = tags[b["ids"]]
    assert g.tags_info() == (int((rt != NONE).sum()), len(rt), 700) and g.tag_rows(0) == int((rt == 0).sum()) > 9000
    _check(gpu, g, b, _set({}, labels, tags), 700)


def test_user_view_answers_as_its_parent(gpu, pkg):
    b = base(**BASE)
    g = tr.install(_upload(gpu(), b), tr.assignment(b))
    q = b["queries"]
    qt = tr.query_tags(len(q))
    v = g.view()
    assert v.tags_info() == g.tags_info() and v.tag_rows(255) == g.tag_rows(255)
    for k in (1, 10):
        assert _same_search(v.search_tags(q, k, qt, *tr.IVF_PARAMS[:2], efSearch=tr.IVF_PARAMS[2]),
                            g.search_tags(q, k, qt, *tr.IVF_PARAMS[:2], efSearch=tr.IVF_PARAMS[2]))
        assert v.last_scan_kernel().endswith("+tags")
    v.close()
