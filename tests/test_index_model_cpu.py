"""The host model and the schedules of tests/index_model.py, checked without a GPU: the model against a from-scratch build
of the lists, its filter expectation against brute force, and the conditions that keep tests/test_gpu_sequences.py from
quietly testing little (every ordered pair of step classes occurs; the fixtures distinguish right from wrong answers)."""
import numpy as np
import pytest

import grouping_append_ref as gar
import index_model as im
import range_ref
import recon_ref
import synth

FLAVOURS = tuple(im.FLAVOURS)


# ---- 1. the model against a from-scratch build ------------------------------------------------------------------------
class _Rows:
    """Every row ever inserted, tagged (list, sub-group, insertion counter); the lists are rebuilt from the tags."""

    def __init__(self, c):
        self.reset(c)

    def reset(self, c):
        n = len(c["ids"])
        self.nc, self.nsubc, self.M = c["nc"], c["nsubc"], c["code_size"]
        if self.nsubc:
            lst, sub = gar.rows_of(c["offsets"], c["subgroup_sizes"])
        else:
            lst, sub = recon_ref.row_lists(c["offsets"], np.arange(n)), np.zeros(n, np.int64)
        self.t = [np.asarray(lst, np.int64), np.asarray(sub, np.int64), np.arange(n, dtype=np.int64), c["ids"].astype(np.uint32),
                  np.asarray(c["codes"]).reshape(n, -1), c["norm_codes"]]
        self.ctr = n

    def insert(self, lst, sub, ids, codes, ncodes):
        n = len(ids)
        new = [np.asarray(lst, np.int64), np.asarray(sub, np.int64), self.ctr + np.arange(n), ids, codes.reshape(n, self.M), ncodes]
        self.t = [np.concatenate([a, b]) for a, b in zip(self.t, new)]
        self.ctr += n

    def drop(self, labels):
        keep = ~np.isin(self.t[3], labels)
        self.t = [a[keep] for a in self.t]

    def csr(self):
        lst, sub, ctr, ids, codes, ncodes = self.t
        order = np.lexsort((ctr, sub, lst))
        off = np.concatenate([[0], np.cumsum(np.bincount(lst, minlength=self.nc))]).astype(np.uint64)
        out = (off, ids[order], codes[order], ncodes[order])
        if self.nsubc:
            out += (np.bincount(lst * self.nsubc + sub, minlength=self.nc * self.nsubc).reshape(self.nc, self.nsubc),)
        return out


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_model_equals_from_scratch_build(flavour):
    for seed in im.SEEDS[:3]:
        m = im.IndexModel(flavour)
        rows = _Rows(m.c)
        updates = 0
        for i, (kind, a) in enumerate(im.schedule(flavour, seed)):
            if kind in ("append_ivf", "append_grouping"):
                rows.insert(a["list_idx"], a.get("sub_idx", np.zeros(len(a["ids"]), np.int64)), a["ids"], a["codes"], a["norm_codes"])
            elif kind == "add":
                ox = synth.oracle_index(m.corpora[m.which])     # the encoder reads the tables, not the lists
                ox.set_params(1, 0, im.EF)
                idx, codes, ncodes, _ = ox.add_batch_encode(a["x"])
                rows.insert(idx, np.zeros(len(idx), np.int64), a["ids"], codes, ncodes)
            elif kind == "add_groups":
                lst, sub = gar.rows_of(m.full["offsets"], m.full["subgroup_sizes"])
                pick = np.isin(lst, a["which"])
                rows.insert(lst[pick], sub[pick], m.full["ids"][pick], np.asarray(m.full["codes"])[pick], m.full["norm_codes"][pick])
            elif kind in ("remove_ids", "empty_index"):
                rows.drop(a["labels"])
            got = im.apply(m, kind, a)
            if kind == "reupload":
                rows.reset(m.c)
            if kind in im.UPDATE_KINDS:
                updates += 1
                for x, y in zip(m.csr(), rows.csr()):
                    assert np.array_equal(x, y), (flavour, seed, i, kind)
            if kind == "remove_ids":
                assert got[0] == int(got[1].sum()) > 0
        assert updates >= 4


# ---- 2. the filter expectation against brute force ---------------------------------------------------------------------
@pytest.mark.parametrize("deny", [False, True])
def test_filter_expectation_equals_brute_force(deny):
    m = im.IndexModel("ivf_pq16")
    rng = np.random.default_rng(3)
    passing = rng.choice(m.c["ids"], m.n // 50, replace=False).astype(np.uint32)
    m.set_filter(np.setdiff1d(m.c["ids"], passing) if deny else passing, deny)
    q = m.c["queries"]
    sc = range_ref.scored_batch(m.c, q, im.NPROBE, 300, im.EF)   # k >= ncode: every scored code with its distance
    for k in (1, 10):
        d, lab = m.expect_search(q, k, max_codes=300)[:2]
        d, lab = d.reshape(len(q), k), lab.reshape(len(q), k)
        short = 0
        for i in range(len(q)):
            keep = np.isin(sc["labels"][i], passing)
            bl, bd = sc["labels"][i][keep], sc["dists"][i][keep]
            o = np.lexsort((bl, bd))[:k]
            want_l = np.concatenate([bl[o], np.full(k - len(o), -1)])
            want_d = np.concatenate([bd[o], np.full(k - len(o), im.FLT_MAX, np.float32)])
            o2 = np.lexsort((np.where(lab[i] < 0, 2 ** 40, lab[i]), d[i]))
            assert np.array_equal(lab[i][o2], want_l) and np.array_equal(d[i][o2].view(np.uint32), want_d.view(np.uint32)), (k, i)
            short += len(o) < k
        assert k == 1 or short > 0     # a fiftieth of 300 codes leaves some query fewer than ten


# ---- 3. coverage --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_ordered_pair_of_classes_occurs(flavour):
    classes, queries = im.CLASSES[flavour], im.QUERY_CLASSES[flavour]
    seen = set()
    for seed in im.SEEDS:
        cl = im.classes_of(im.schedule(flavour, seed))
        assert len(cl) == im.NSTEPS and set(cl) <= set(classes)
        seen |= set(zip(cl[:-1], cl[1:]))
        for first in ("U", "F", "R"):   # every query class after each of them within this schedule
            if first in classes:
                at = cl.index(first)
                assert set(queries) <= set(cl[at + 1:]), (flavour, seed, first)
    missing = [(a, b) for a in classes for b in queries if (a, b) not in seen]
    assert not missing, missing
    print("%s: %d steps, %d of %d required ordered pairs, %d distinct pairs in all"
          % (flavour, im.NSEEDS * im.NSTEPS, len(classes) * len(queries) - len(missing), len(classes) * len(queries), len(seen)))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_kind_and_form_occurs(flavour):
    """Over the committed seeds: every kind of step of the flavour, in each of its forms."""
    seen = set()
    for seed in im.SEEDS:
        for kind, a in im.schedule(flavour, seed):
            seen.add(kind)
            seen |= {"%s:%s=%s" % (kind, k, a[k]) for k in ("dev", "coarse", "deny", "what", "heap", "k", "nq", "permille", "value",
                                                            "pruning", "max_codes", "key") if k in a}
            if kind in ("qr", "view"):
                seen.add("qr:finite" if np.isfinite(a["radius"]) else "qr:inf")
            if kind == "set_filter" and a["labels"].min() >= 4 * 10 ** 6:
                seen.add("set_filter:none")
    want = {"remove_ids", "empty_index", "set_filter:deny=True", "set_filter:deny=False", "clear_filter", "qr:finite", "qr:inf",
            "q1:dev=True", "q1:dev=False", "q1:coarse=True", "q1:nq=7", "q1:nq=48", "qk:heap=True", "qk:heap=False"}
    want |= {"q1:max_codes=%d" % x for x in (1, 300, 2000, 10 ** 9)} | {"qk:k=%d" % k for k in (2, 10, 100, 1000)}
    if flavour != "base_store":
        want |= {"prepare_latency", "scan_pipe:value=0", "scan_pipe:value=1", "scan_pipe:value=-1", "set_profiling", "qb", "view",
                 "qx", "set_filter:none"}
        want |= {"set_batch_split:permille=%d" % x for x in (0, 300, 1000)} | {"ql:nq=%d" % x for x in (1, 2, 8)}
        want |= {"refused:what=%s" % w for w in ("ef_below_nprobe", "nprobe_0", "one_coarse_array", "nan_radius", "bad_option")}
    if flavour == "grouping":
        want |= {"append_grouping", "add_groups", "q1:pruning=True", "q1:pruning=False", "qr:pruning=True", "qk:pruning=True",
                 "refused:what=append_ivf_on_grouping"}
    else:
        want |= {"append_ivf:dev=True", "append_ivf:dev=False", "add"}
    if flavour.startswith("ivf"):
        want |= {"reupload", "refused:what=append_bad_list"}
    if flavour == "base_store":
        want |= {"upload_base", "set_base_filter:deny=True", "set_base_filter:deny=False", "clear_base_filter", "rerank",
                 "search_rerank", "exact_range"} | {"exact_search:k=%d" % k for k in (1, 10, 100)}
        want |= {"exact_option:key=%s" % k for k in ("exact_range_map", "exact_filter_form", "exact_splits")}
    assert want <= seen, sorted(want - seen)


def test_schedule_is_a_pure_function_and_a_prefix_replays():
    im.schedule.cache_clear()
    a = im.schedule("ivf_pq16", 1)
    im.schedule.cache_clear()
    b = im.schedule("ivf_pq16", 1)
    assert [k for k, _ in a] == [k for k, _ in b]
    for (_, x), (_, y) in zip(a, b):
        assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
    short = im.schedule("ivf_pq16", 1, 12)
    assert [k for k, _ in short] == [k for k, _ in a[:12]]
    for (_, x), (_, y) in zip(short, a):
        assert all(np.array_equal(x[k], y[k]) for k in x)


# ---- 4. fixture conditions (schedule() asserts most of them while it builds; these replay the model to look again) --------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_fixture_conditions(flavour):
    for seed in im.SEEDS:
        steps = im.schedule(flavour, seed)
        m = im.IndexModel(flavour)
        kinds = [k for k, _ in steps]
        assert kinds.count("empty_index") == 1
        both_sides = False
        for i, (kind, a) in enumerate(steps):
            where = (flavour, seed, i, kind)
            if kind in ("qr", "view"):
                q = m.c["queries"][a["qi"]]
                sc = m.scored(q, max_codes=a["max_codes"], pruning=a["pruning"])
                per = np.array([(d < a["radius"]).sum() for d in sc["dists"]])   # the oracle's answer, no filter
                if np.isfinite(a["radius"]):
                    assert (per == 0).any() and (per > 0).any(), where
                else:
                    assert np.array_equal(per, sc["ncode"]), where
            if kind in ("q1", "ql", "qk") and m.filter is not None and m.pass_rows().any():
                q = m.c["queries"][a["qi"]]
                kw = dict(max_codes=a.get("max_codes", im.MAX_CODES), pruning=a["pruning"])
                assert (m.expect_search(q, a.get("k", 1), **kw)[1] !=
                        m.expect_search(q, a.get("k", 1), filtered=False, **kw)[1]).any(), where
            if kind == "qk" and a["k"] == 1000:
                ncode = m.scored(m.c["queries"][a["qi"]], max_codes=a["max_codes"], pruning=a["pruning"])["ncode"]
                both_sides |= bool((ncode < 1000).any() and (ncode > 1000).any())
            if kind in ("append_ivf", "append_grouping", "add"):
                assert not np.isin(a["ids"], m.c["ids"]).any() and len(np.unique(a["ids"])) == len(a["ids"]), where
            im.apply(m, kind, a)
            if kind == "empty_index":
                assert m.n == 0 and kinds[i + 1] in ("append_ivf", "append_grouping"), where
                d, lab = m.expect_search(m.c["queries"][a["qi"]], 1)[:2]
                assert (lab == -1).all() and (d == im.FLT_MAX).all(), where
            else:
                assert m.n > 0, where
            assert (m.c["norm_codes"] <= 254).all(), where
        assert both_sides, (flavour, seed)
