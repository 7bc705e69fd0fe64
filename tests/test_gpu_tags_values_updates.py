"""Tag AND value through in-place updates: one handle goes through set_tags / set_values in parts, appends,
add, removal, an upsert, re-tagging and re-valuing, clear_tags and clear_values; after every step search_tags_values and
range_search_tags_values equal a fresh handle that uploaded the lists the handle holds and set the tags and values of the
assignment as it stands, every result passes its query's pair, and tag_value_rows equals numpy counts.  The call keeps no
state of its own, so what is checked here is that it reads the two row arrays every update re-derives."""
import numpy as np
import pytest

import tags_values_ref as tv
from test_gpu_filter_slots import base
from test_gpu_remove import BASE, GROUPING, _upload, _same_search

pytestmark = pytest.mark.gpu

TNONE, VNONE = tv.TAG_NONE, tv.VALUE_NONE
EXTRA = [(0, (0x80000000, 0x80000000)), (7, (7, 7)), (TNONE, (VNONE, VNONE)), (0xfffe, tv.VALUED)]  # counted beside the pattern's


def _set(d, labels, xs, none):
    """The map after a set call: dict label -> tag or value, NONE entries dropped."""
    for l, x in zip(np.asarray(labels).tolist(), np.asarray(xs).tolist()):
        if x == none:
            d.pop(l, None)
        else:
            d[l] = x
    return d


def _asg(tags, values):
    """The assignment as it stands; with neither map one label no row bears, so that every row reads NONE."""
    labels = np.array(sorted(set(tags) | set(values)) or [0xfffffffe], np.uint32)
    return (labels, np.array([tags.get(int(l), TNONE) for l in labels], np.uint16),
            np.array([values.get(int(l), VNONE) for l in labels], np.uint32))


def _rows(ids, asg, p):
    return int(tv.passing_rows({"ids": np.asarray(ids)}, asg, p).sum())


def _check(gpu, g, c, tags, values, params=tv.IVF_PARAMS, prunings=(False,)):
    """g against a fresh handle on g's own lists with the tags and values as they stand."""
    asg = _asg(tags, values)
    off, ids, codes, ncodes = g.download_ivf()
    f = gpu()
    f.upload_ivf(c["d"], c["code_size"], off, ids, codes, ncodes, c["centroid_norms"], c["pq_centroids"], c["norm_table"],
                 opq_A=c["opq_A"])
    if c.get("nsubc"):
        f.upload_grouping(c["nsubc"], *g.download_grouping_tables())
    gr = c["graph"]
    f.upload_quantizer(gr.counts, gr.links, gr.vectors, gr.enterpoint)
    if tags:
        f.set_tags(np.array(sorted(tags), np.uint32), np.array([tags[l] for l in sorted(tags)], np.uint16))
    if values:
        f.set_values(np.array(sorted(values), np.uint32), np.array([values[l] for l in sorted(values)], np.uint32))
    for p in tv.PATTERN + EXTRA:
        t, (lo, hi) = tv.key(p)
        assert g.tag_value_rows(t, lo, hi) == f.tag_value_rows(t, lo, hi) == _rows(ids, asg, p), p
    q = c["queries"]
    qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
    nprobe, mc, ef = params
    for pruning in prunings:
        for k, heap in ((1, False), (10, True)):
            got = g.search_tags_values(q, k, qt, qr, nprobe, mc, efSearch=ef, do_pruning=pruning, heap_order=heap)
            assert g.last_scan_kernel().endswith("+tags+values")
            assert _same_search(got, f.search_tags_values(q, k, qt, qr, nprobe, mc, efSearch=ef, do_pruning=pruning,
                                                          heap_order=heap)), (pruning, k)
            for p in tv.PATTERN:
                lab = got[1][tv.mine(qt, qr, p)]
                lab = lab[lab >= 0].astype(np.uint32)
                assert tv.passing_rows({"ids": lab}, asg, p).all(), ("a result does not pass its query's pair", p)
        tenth = f.search(q, 10, nprobe, mc, efSearch=ef, do_pruning=pruning)[0][:, 9]
        radius = float(np.median(tenth))
        a = g.range_search_tags_values(q, radius, qt, qr, nprobe, mc, efSearch=ef, do_pruning=pruning)
        b = f.range_search_tags_values(q, radius, qt, qr, nprobe, mc, efSearch=ef, do_pruning=pruning)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    f.close()
    return got


def _tables(b):
    full = tv.assignment(b)
    m = full[1] != TNONE
    tl, tg = full[0][m], full[1][m]
    m = full[2] != VNONE
    return full, tl, tg, full[0][m], full[2][m]


def test_ivf_sequence(gpu, pkg):
    b = base(**BASE)
    rng = np.random.default_rng(31)
    nc, M = b["nc"], b["code_size"]
    g = _upload(gpu(), b)
    g.upload_codebooks(b["d"], M, b["pq_centroids"], b["norm_table"], b["opq_A"])
    full, tl, tg, vl, vv = _tables(b)
    tags, values = {}, {}
    _check(gpu, g, b, tags, values)  # neither table yet
    # set_tags and set_values in parts, interleaved: the call answers on only tags, then on both as they grow
    for p in range(2):
        g.set_tags(tl[p::2], tg[p::2])
        _set(tags, tl[p::2], tg[p::2], TNONE)
        _check(gpu, g, b, tags, values)
        g.set_values(vl[p::2], vv[p::2])
        _set(values, vl[p::2], vv[p::2], VNONE)
        _check(gpu, g, b, tags, values)
    for p in tv.PATTERN:
        t, (lo, hi) = tv.key(p)
        assert g.tag_value_rows(t, lo, hi) == int(tv.passing_rows(b, full, p).sum())
    # append_ivf: rows whose labels were given a tag and a value before they arrived ...
    n = 3000
    early = (np.arange(n) + 10 ** 6).astype(np.uint32)
    early_tags = np.where(np.arange(n) % 3 == 0, 0, 0xfffe).astype(np.uint16)
    early_values = np.where(np.arange(n) % 2 == 0, 0x80000000, 0xfffffffe).astype(np.uint32)
    g.set_tags(early, early_tags)
    g.set_values(early, early_values)
    _set(tags, early, early_tags, TNONE)
    _set(values, early, early_values, VNONE)
    before = g.tag_value_rows(0, 0x80000000, 0x80000000)

    def batch(ids):
        return (rng.integers(0, nc, len(ids)).astype(np.uint32), ids, rng.integers(0, 256, (len(ids), M)).astype(np.uint8),
                rng.integers(0, 255, len(ids)).astype(np.uint8))

    def answers():
        q = b["queries"]
        return g.search_tags_values(q, 10, tv.query_tags(len(q)), tv.query_ranges(len(q)), *tv.IVF_PARAMS[:2],
                                    efSearch=tv.IVF_PARAMS[2])
    # a failing update leaves the answers as they were
    probe = answers()
    bad = batch(early)
    bad[0][n // 2] = nc
    with pytest.raises(pkg.IvfHnswError) as e:
        g.append_ivf(*bad)
    assert e.value.code == pkg.ERR_INVALID and g.tag_value_rows(0, 0x80000000, 0x80000000) == before
    assert _same_search(answers(), probe)
    g.append_ivf(*batch(early))
    assert g.tag_value_rows(0, 0x80000000, 0x80000000) == before + int(((np.arange(n) % 3 == 0) & (np.arange(n) % 2 == 0)).sum())
    _check(gpu, g, b, tags, values)
    # ... and rows whose labels carry neither (beyond the tables, and inside them)
    late = np.concatenate([np.arange(2 * 10 ** 6, 2 * 10 ** 6 + 1000), np.arange(500000, 501000)]).astype(np.uint32)
    bare = g.tag_value_rows(TNONE, VNONE, VNONE)
    g.append_ivf(*batch(late))
    assert g.tag_value_rows(TNONE, VNONE, VNONE) == bare + len(late)
    _check(gpu, g, b, tags, values)
    # add: every fourth new label gets tag 255 and the value 0 first
    x = b["base"][:2000] + np.float32(0.5)
    added = (np.arange(len(x)) + 3 * 10 ** 6).astype(np.uint32)
    g.set_tags(added[::4], np.full(len(added[::4]), 255, np.uint16))
    g.set_values(added[::4], np.zeros(len(added[::4]), np.uint32))
    _set(tags, added[::4], np.full(len(added[::4]), 255, np.uint16), TNONE)
    _set(values, added[::4], np.zeros(len(added[::4]), np.uint32), VNONE)
    rows = g.tag_value_rows(255, 0, 0)
    g.add(x, added, efSearch=40)
    assert g.tag_value_rows(255, 0, 0) == rows + len(added[::4])
    _check(gpu, g, b, tags, values)
    # remove_ids: the labels keep tag and value (label space, not row space)
    gone = rng.choice(np.unique(g.download_ivf()[1]), 6000, replace=False)
    assert g.remove_ids(gone)[0] == 6000
    _check(gpu, g, b, tags, values)
    # upsert_ivf: half of the labels resident, half new; a label twice in the batch is refused and nothing changes
    ids_now = np.unique(g.download_ivf()[1])
    resident = rng.choice(ids_now, 1000, replace=False).astype(np.uint32)
    fresh = (np.arange(1000) + 4 * 10 ** 6).astype(np.uint32)
    both = np.concatenate([resident, fresh])
    counts = {tv.key(p): g.tag_value_rows(tv.key(p)[0], *tv.key(p)[1]) for p in tv.PATTERN}
    probe = answers()
    with pytest.raises(pkg.IvfHnswError) as e:
        g.upsert_ivf(*batch(np.concatenate([both, both[:1]])))
    assert e.value.code == pkg.ERR_INVALID
    assert {tv.key(p): g.tag_value_rows(tv.key(p)[0], *tv.key(p)[1]) for p in tv.PATTERN} == counts
    assert _same_search(answers(), probe)
    assert g.upsert_ivf(*batch(both))[0] == 1000
    _check(gpu, g, b, tags, values)
    # re-tagging and re-valuing: of the resident labels that pass (0, band), 100 change tag, 100 change value, 100 lose both
    band = (0, tv.BAND31)
    mine = tv.labels_in(_asg(tags, values), band)
    mine = mine[np.isin(mine, np.unique(g.download_ivf()[1]))][:300]
    assert len(mine) == 300
    rows_band = g.tag_value_rows(0, *tv.BAND31)
    held = np.isin(g.download_ivf()[1], mine).sum()
    g.set_tags(mine[:100], np.full(100, 7, np.uint16))
    g.set_values(mine[100:200], np.full(100, 7, np.uint32))
    g.set_tags(mine[200:], np.full(100, TNONE, np.uint16))
    g.set_values(mine[200:], np.full(100, VNONE, np.uint32))
    _set(tags, mine[:100], np.full(100, 7, np.uint16), TNONE)
    _set(values, mine[100:200], np.full(100, 7, np.uint32), VNONE)
    _set(tags, mine[200:], np.full(100, TNONE, np.uint16), TNONE)
    _set(values, mine[200:], np.full(100, VNONE, np.uint32), VNONE)
    assert g.tag_value_rows(0, *tv.BAND31) == rows_band - held
    _check(gpu, g, b, tags, values)
    # clear_tags: only the values decide; clear_values: only (NONE, (.., 0xffffffff)) finds anything
    g.clear_tags()
    _check(gpu, g, b, {}, values)
    g.clear_values()
    got = _check(gpu, g, b, {}, {})
    q = b["queries"]
    qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
    every = (qt == TNONE) & (qr[:, 1] == VNONE) & (qr[:, 0] <= qr[:, 1])
    assert (got[1][~every] == -1).all() and (got[1][every] >= 0).any()


def test_grouping_sequence(gpu):
    import grouping_append_ref as gar
    import test_gpu_add_groups as tg
    c = base(**GROUPING[1])
    part, batch = gar.split_corpus(c, gar.tail_mask(c, np.random.default_rng(9)))
    g = _upload(gpu(), part)
    full, tl, tgs, vl, vv = _tables(c)
    tags, values = _set({}, tl, tgs, TNONE), _set({}, vl, vv, VNONE)
    g.set_tags(tl, tgs)  # the tails' labels get tag and value before their rows arrive
    g.set_values(vl, vv)
    _check(gpu, g, c, tags, values, params=tv.GROUPING_PARAMS, prunings=(False, True))
    tg._append(g, batch)
    for p in tv.PATTERN:
        t, (lo, hi) = tv.key(p)
        assert g.tag_value_rows(t, lo, hi) == int(tv.passing_rows(c, full, p).sum()), p
    _check(gpu, g, c, tags, values, params=tv.GROUPING_PARAMS, prunings=(False, True))
    gone = np.random.default_rng(15).choice(c["ids"], len(c["ids"]) // 4, replace=False)
    g.remove_ids(gone)
    _check(gpu, g, c, tags, values, params=tv.GROUPING_PARAMS, prunings=(False, True))


def test_user_view_before_and_after_the_tables(gpu):
    """A view reads what its parent held when the view was made: neither table before, both after."""
    b = base(**BASE)
    g = _upload(gpu(), b)
    q = b["queries"]
    qt, qr = tv.query_tags(len(q)), tv.query_ranges(len(q))
    args = (qt, qr) + tuple(tv.IVF_PARAMS[:2])
    early = g.view()
    bare = g.search_tags_values(q, 1, *args, efSearch=tv.IVF_PARAMS[2])
    asg = tv.assignment(b)
    tv.install(g, asg, values=False)
    middle = g.view()
    tags_only = g.search_tags_values(q, 1, *args, efSearch=tv.IVF_PARAMS[2])
    tv.install(g, asg, tags=False)
    late = g.view()
    for p in tv.PATTERN:
        t, (lo, hi) = tv.key(p)
        assert late.tag_value_rows(t, lo, hi) == g.tag_value_rows(t, lo, hi) == int(tv.passing_rows(b, asg, p).sum()), p
        assert early.tag_value_rows(t, lo, hi) == int(tv.passing_rows(b, tv.without(asg, False, False), p).sum()), p
        assert middle.tag_value_rows(t, lo, hi) == int(tv.passing_rows(b, tv.without(asg, values=False), p).sum()), p
    for k in (1, 10):
        want = g.search_tags_values(q, k, *args, efSearch=tv.IVF_PARAMS[2])
        assert _same_search(late.search_tags_values(q, k, *args, efSearch=tv.IVF_PARAMS[2]), want)
        assert late.last_scan_kernel().endswith("+tags+values")
    both = g.search_tags_values(q, 1, *args, efSearch=tv.IVF_PARAMS[2])
    assert not _same_search(bare, tags_only) and not _same_search(tags_only, both)
    assert _same_search(early.search_tags_values(q, 1, *args, efSearch=tv.IVF_PARAMS[2]), bare)
    assert _same_search(middle.search_tags_values(q, 1, *args, efSearch=tv.IVF_PARAMS[2]), tags_only)
    for v in (early, middle, late):
        v.close()
