"""A host model of one long-lived device handle, and seeded random schedules of calls on it (no GPU, no HIP).

IndexModel holds what the handle should hold after any order of updates: the lists as a corpus dict of the form
synth.make_corpus returns (so that synth.oracle_index(model.c) works), the Grouping tables, the label filter, the uint8 base
store and its filter.  Its mutations restate the updates with the references the suite already trusts (_csr_append,
grouping_append_ref.merge_lists, remove_ref.filter_lists, the oracle's encoders); its expectations are the oracle and the
numpy restatements on that state.  schedule(flavour, seed, nsteps) is a pure function of its arguments: it draws steps
(kind, arguments) that mix updates, filter changes, knobs, refused calls and every kind of query, and asserts while it
builds them the conditions that keep a schedule from testing little (see the asserts in _Gen)."""
import functools

import numpy as np

from conftest import corpus
import exact_filter_ref
import exact_range_ref
import exact_ref
import filter_ref
import grouping_append_ref as gar
import range_ref
import recon_ref
import remove_ref
import rerank_ref
import synth
from test_gpu_append import _csr_append

NPROBE, MAX_CODES, EF = 16, 2000, 40
FLT_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
NSEEDS, NSTEPS = 8, 40
SEEDS = tuple(range(NSEEDS))

PQ16 = dict(seed=301, nc=128, d=128, M=16, n_base=8000, nq=48, efConstruction=60)
OPQ12 = dict(seed=302, nc=96, d=96, M=12, opq=True, n_base=6000, nq=48, efConstruction=60)
GROUP = dict(seed=303, nc=96, d=96, M=16, n_base=8000, nsubc=8, nq=48, efConstruction=60)
FLAVOURS = {"ivf_pq16": dict(start=PQ16, other=OPQ12), "ivf_opq_rt": dict(start=OPQ12, other=PQ16),
            "grouping": dict(start=GROUP), "base_store": dict(start=PQ16, base=True)}
BASE_EXTRA = 4000          # rows of the base store beyond the corpus: the labels appends may take
FIRST_NEW_ID = 10 ** 6     # fresh labels of the flavours without a base store

# step classes (the issue's table); the query classes are the second member of every ordered pair that must occur
LIST_QUERIES = ("Q1", "QL", "QK", "QR", "QX", "QB", "V")
EXACT_QUERIES = ("XS", "XR", "RR", "SR")
CLASSES = {"ivf_pq16": ("U", "F", "R", "K", "E") + LIST_QUERIES, "ivf_opq_rt": ("U", "F", "R", "K", "E") + LIST_QUERIES,
           "grouping": ("U", "F", "K", "E") + LIST_QUERIES, "base_store": ("U", "F", "UB", "Q1", "QK", "QR") + EXACT_QUERIES}
QUERY_CLASSES = {f: (EXACT_QUERIES if f == "base_store" else LIST_QUERIES) for f in FLAVOURS}
KIND_CLASS = {"append_ivf": "U", "add": "U", "remove_ids": "U", "append_grouping": "U", "add_groups": "U", "empty_index": "U",
              "set_filter": "F", "clear_filter": "F", "reupload": "R", "prepare_latency": "K", "set_batch_split": "K",
              "scan_pipe": "K", "set_profiling": "K", "refused": "E", "q1": "Q1", "ql": "QL", "qk": "QK", "qr": "QR", "qx": "QX",
              "qb": "QB", "view": "V", "upload_base": "UB", "set_base_filter": "UB", "clear_base_filter": "UB",
              "exact_option": "UB", "exact_search": "XS", "exact_range": "XR", "rerank": "RR", "search_rerank": "SR"}
UPDATE_KINDS = ("append_ivf", "add", "remove_ids", "append_grouping", "add_groups", "empty_index", "reupload")


# ---- start states (shared, never changed: the model copies what it changes) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _start(name):
    return filter_ref.clipped(corpus(**{"PQ16": PQ16, "OPQ12": OPQ12}[name]))


@functools.lru_cache(maxsize=None)
def _grouping_start():
    """(the start corpus with some groups held out, the whole index add_group builds, the held-out groups' mask).  Only
    groups whose rows all carry a norm code <= 254 are held out: add_groups stores what the encoder gives, and
    filter_ref.poisoned needs 255 free."""
    import test_gpu_add_groups as tg
    c = corpus(**GROUP)
    full = tg._assemble(c, tg._build_graph(c), tg._groups_of(c))
    lst, _ = gar.rows_of(full["offsets"], full["subgroup_sizes"])
    has255 = np.bincount(lst[full["norm_codes"] == 255], minlength=c["nc"]) > 0
    gone = (np.random.default_rng(5).random(c["nc"]) < 0.3) & ~has255
    lens = np.diff(full["offsets"].astype(np.int64))
    assert (gone & (lens > 0)).sum() >= 8 and (gone & (lens == 0)).any()
    part, _ = gar.without_groups(full, gone)
    part["subgroup_sizes"][gone] = 0
    return filter_ref.clipped(part), full, gone


@functools.lru_cache(maxsize=None)
def _base_rows():
    c = _start("PQ16")
    extra = synth.sift_like(np.random.default_rng(77), BASE_EXTRA, c["d"])
    return np.clip(np.rint(np.concatenate([c["base"], extra])), 0, 255).astype(np.uint8)


def queries_u8(q):
    return np.clip(np.rint(q), 0, 255).astype(np.uint8)


def first_rows(ids, labels):
    """(lowest row bearing each label or -1, number of rows bearing it), plain numpy."""
    labels = np.asarray(labels, np.uint32)
    if not len(ids):
        return np.full(len(labels), -1, np.int64), np.zeros(len(labels), np.uint32)
    order = np.argsort(ids, kind="stable")
    s = ids[order]
    a, b = np.searchsorted(s, labels, side="left"), np.searchsorted(s, labels, side="right")
    rows = np.where(b > a, order[np.minimum(a, len(ids) - 1)], -1).astype(np.int64)
    return rows, (b - a).astype(np.uint32)


class IndexModel:
    def __init__(self, flavour):
        self.flavour = flavour
        f = FLAVOURS[flavour]
        self.full = self.gone = self.base = None
        if flavour == "grouping":
            part, self.full, gone = _grouping_start()
            self.c, self.gone = dict(part), gone.copy()
            for k in ("alphas", "nn_centroid_idxs", "inter_centroid_dists", "subgroup_sizes"):
                self.c[k] = part[k].copy()
        else:
            self.corpora = [_start("PQ16" if kw is PQ16 else "OPQ12") for kw in (f["start"], f.get("other")) if kw]
            self.which = 0
            self.c = dict(self.corpora[0])
        if f.get("base"):
            self.base = _base_rows().copy()
        self.filter = None          # (labels, deny)
        self.base_filter = None
        self.latency = False        # prepare_latency since the last upload_quantizer
        self.split = 1000
        self.removed = np.zeros(0, np.uint32)
        self.next_id = FIRST_NEW_ID

    # ---- state -------------------------------------------------------------------------------------------------------
    nc = property(lambda self: self.c["nc"])
    M = property(lambda self: self.c["code_size"])
    grouping = property(lambda self: bool(self.c["nsubc"]))
    n = property(lambda self: len(self.c["ids"]))

    def _lists(self):
        return (self.c["offsets"], self.c["ids"], np.asarray(self.c["codes"]).reshape(self.n, self.M), self.c["norm_codes"])

    def _set(self, off, ids, codes, ncodes, sg=None):
        self.c.update(offsets=np.asarray(off, np.uint64), ids=np.asarray(ids, np.uint32),
                      codes=np.ascontiguousarray(codes, np.uint8).reshape(len(ids), self.M), norm_codes=np.asarray(ncodes, np.uint8))
        if sg is not None:
            self.c["subgroup_sizes"] = np.asarray(sg, np.uint32)

    def csr(self):
        """What download_ivf must return (and download_grouping, fifth, on a Grouping handle)."""
        return self._lists() + ((self.c["subgroup_sizes"],) if self.grouping else ())

    def pass_rows(self):
        return np.ones(self.n, bool) if self.filter is None else filter_ref.passing(self.c["ids"], *self.filter)

    def filter_info(self):
        if self.filter is None:
            return (-1, self.n, self.n)
        return (1 if self.filter[1] else 0, int(self.pass_rows().sum()), self.n)

    def base_mask(self):
        if self.base_filter is None:
            return np.ones(len(self.base), bool)
        return exact_filter_ref.pass_mask(len(self.base), *self.base_filter)

    def base_filter_info(self):
        m = self.base_mask()
        return (-1 if self.base_filter is None else (1 if self.base_filter[1] else 0), int(m.sum()), len(m))

    # ---- mutations ---------------------------------------------------------------------------------------------------
    def append(self, list_idx, ids, codes, norm_codes):
        assert not self.grouping and not np.isin(ids, self.c["ids"]).any() and len(np.unique(ids)) == len(ids)
        self._set(*_csr_append(self._lists(), self.nc, np.asarray(list_idx, np.uint32), ids, codes.reshape(len(ids), -1),
                               norm_codes))

    def encode(self, x):
        """(list, codes, norm codes) add gives the vectors x: the oracle's add_batch encoder on this state's tables."""
        ox = synth.oracle_index(self.c)
        ox.set_params(1, 0, EF)
        idx, codes, ncodes, _ = ox.add_batch_encode(np.ascontiguousarray(x, np.float32))
        return idx, codes, ncodes

    def add(self, x, ids):
        idx, codes, ncodes = self.encode(x)
        self.append(idx, ids, codes, ncodes)
        return idx, codes, ncodes

    def append_grouping(self, list_idx, sub_idx, ids, codes, norm_codes):
        assert self.grouping and not np.isin(ids, self.c["ids"]).any() and not self.gone[list_idx].any()
        if not self.n:   # an index that holds no code (merge_lists reads the code size off the resident codes): the batch alone
            nc, nsubc = self.c["subgroup_sizes"].shape
            li, si = np.asarray(list_idx, np.int64), np.asarray(sub_idx, np.int64)
            o = np.lexsort((np.arange(len(li)), si, li))   # list, then sub-group, then arrival order
            sg = np.bincount(li * nsubc + si, minlength=nc * nsubc).reshape(nc, nsubc)
            return self._set(np.concatenate([[0], np.cumsum(sg.sum(1))]), ids[o], codes.reshape(len(li), -1)[o], norm_codes[o], sg)
        m = gar.merge_lists(*self._lists(), self.c["subgroup_sizes"], list_idx, sub_idx, ids, codes, norm_codes)
        self._set(m["offsets"], m["ids"], m["codes"], m["norm_codes"], m["subgroup_sizes"])

    def group_batch(self, which):
        """add_groups' arguments for the held-out groups `which`: (offsets u64 [G + 1], points, ids)."""
        import test_gpu_add_groups as tg
        groups = tg._groups_of(corpus(**GROUP))
        xs = [groups[int(cc)][0] for cc in which]
        off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
        x = np.concatenate(xs) if off[-1] else np.zeros((0, self.c["d"]), np.float32)
        return off, x, np.concatenate([groups[int(cc)][1] for cc in which]).astype(np.uint32)

    def add_groups(self, which):
        """Held-out groups come back as add_group built them: their rows and their rows of the four tables."""
        which = [int(cc) for cc in which]
        assert all(self.gone[cc] for cc in which)
        off, foff = self.c["offsets"].astype(np.int64), self.full["offsets"].astype(np.int64)
        cur, full = self._lists(), (None, self.full["ids"], np.asarray(self.full["codes"]).reshape(len(self.full["ids"]), -1),
                                    self.full["norm_codes"])
        assert all(off[cc + 1] == off[cc] for cc in which)
        parts = [[], [], []]
        for cc in range(self.nc):
            src, a, b = (full, foff[cc], foff[cc + 1]) if cc in which else (cur, off[cc], off[cc + 1])
            for j in range(3):
                parts[j].append(src[j + 1][a:b])
        for k in ("alphas", "nn_centroid_idxs", "inter_centroid_dists", "subgroup_sizes"):
            self.c[k][which] = self.full[k][which]
        self.gone[which] = False
        sg = self.c["subgroup_sizes"]
        self._set(np.concatenate([[0], np.cumsum(sg.sum(1, dtype=np.int64))]), *[np.concatenate(p) for p in parts], sg)
        assert (self.c["norm_codes"] <= 254).all()

    def remove(self, labels):
        """remove_ids: returns (rows removed, rows removed per list)."""
        f = remove_ref.filter_lists(*self._lists(), labels, self.c["subgroup_sizes"] if self.grouping else None)
        gone = np.intersect1d(self.c["ids"], np.asarray(labels, np.uint32))
        self.removed = np.union1d(self.removed, gone).astype(np.uint32)
        self._set(f["offsets"], f["ids"], f["codes"], f["norm_codes"], f.get("subgroup_sizes"))
        return int(f["removed"].sum()), f["removed"]

    def reupload(self):
        """upload_ivf of the other corpus with its quantizer: the filter and the latency graph go with the old tables."""
        self.which ^= 1
        self.c = dict(self.corpora[self.which])
        self.filter, self.latency = None, False

    def set_filter(self, labels, deny=False):
        self.filter = (np.asarray(labels, np.uint32), bool(deny))

    def clear_filter(self):
        self.filter = None

    def set_base_filter(self, labels, deny=False):
        self.base_filter = (np.asarray(labels, np.uint32), bool(deny))

    def clear_base_filter(self):
        self.base_filter = None

    def upload_base(self, first, rows):
        self.base[first:first + len(rows)] = rows

    # ---- expectations ------------------------------------------------------------------------------------------------
    def search_corpus(self):
        return self.c if self.filter is None else filter_ref.poisoned(self.c, self.pass_rows())

    def expect_search(self, q, k, nprobe=NPROBE, max_codes=MAX_CODES, ef=EF, pruning=False, filtered=True):
        """(distances, labels, coarse ids, coarse distances, stats) of the oracle: faiss's heap array for k > 1."""
        ox = synth.oracle_index(self.search_corpus() if filtered else self.c)
        ox.set_params(nprobe, max_codes, ef, do_pruning=pruning)
        return ox.search_batch(np.ascontiguousarray(q, np.float32), k=k)

    def scored(self, q, nprobe=NPROBE, max_codes=MAX_CODES, ef=EF, pruning=False):
        return range_ref.scored_batch(self.c, q, nprobe, max_codes, ef, pruning)

    def expect_range(self, q, radius, nprobe=NPROBE, max_codes=MAX_CODES, ef=EF, pruning=False, sc=None):
        """IVFADC: ("ivf", (lims, distances, labels)) in scan order.  Grouping has no restated scan order:
        ("sets", per query the sorted (label, distance bits) pairs).  Either way with the codes scored: sc["ncode"]."""
        sc = self.scored(q, nprobe, max_codes, ef, pruning) if sc is None else sc
        passing = self.c["ids"][self.pass_rows()]
        if self.grouping:
            sets = [range_ref.expected_set(sc, i, radius) for i in range(len(q))]
            return "sets", [s[np.isin(s[:, 0], passing)] for s in sets], sc
        res = range_ref.expected_ivf(self.c, sc, max_codes, radius)
        return "ivf", (range_ref.filtered(res, passing) if self.filter is not None else res), sc

    def expect_locate(self, labels):
        return first_rows(self.c["ids"], labels)

    def expect_reconstruct(self, labels):
        """(ROTATED-space vectors, labels no row bears)."""
        rows, counts = self.expect_locate(labels)
        return recon_ref.recon_rotated(self.c, rows), int((counts == 0).sum())

    def expect_exact(self, qu8, k):
        if self.base_filter is None:
            return exact_ref.search(self.base, qu8, k)
        return exact_filter_ref.search(self.base, qu8, k, self.base_mask())

    def expect_exact_range(self, qu8, radius):
        if self.base_filter is None:
            return exact_range_ref.search(self.base, qu8, radius)
        return exact_filter_ref.range_search(self.base, qu8, radius, self.base_mask())

    def expect_rerank(self, q, cand, k):
        return rerank_ref.rerank(self.base, q, cand, k)


def apply(model, kind, a):
    """The model's side of an update step; returns what the handle's call must return."""
    if kind == "append_ivf":
        return model.append(a["list_idx"], a["ids"], a["codes"], a["norm_codes"])
    if kind == "add":
        return model.add(a["x"], a["ids"])
    if kind == "append_grouping":
        return model.append_grouping(a["list_idx"], a["sub_idx"], a["ids"], a["codes"], a["norm_codes"])
    if kind == "add_groups":
        return model.add_groups(a["which"])
    if kind in ("remove_ids", "empty_index"):
        return model.remove(a["labels"])
    if kind == "reupload":
        return model.reupload()
    if kind == "set_filter":
        return model.set_filter(a["labels"], a["deny"])
    if kind == "clear_filter":
        return model.clear_filter()
    if kind == "prepare_latency":
        model.latency = True
    elif kind == "set_batch_split":
        model.split = a["permille"]
    elif kind == "upload_base":
        model.upload_base(a["first"], a["rows"])
    elif kind == "set_base_filter":
        model.set_base_filter(a["labels"], a["deny"])
    elif kind == "clear_base_filter":
        model.clear_base_filter()


# ---- the schedule ----------------------------------------------------------------------------------------------------------
def class_sequence(flavour, seed, nsteps=NSTEPS):
    """The classes of a schedule's steps.  The required ordered pairs (any class, then a query class) are dealt out over
    the NSEEDS committed seeds and chained; U, F and R open the schedule so that every query class follows each of them."""
    rng = np.random.default_rng([seed, 17])
    classes, queries = CLASSES[flavour], QUERY_CLASSES[flavour]
    pairs = [(a, b) for a in classes for b in queries]
    mine = pairs[seed % NSEEDS::NSEEDS]
    rng.shuffle(mine)
    head = [c for c in ("U", "F", "K", "R") if c in classes]   # K: prepare_latency, so that one R follows it
    seq = list(head)
    for a, b in mine:
        if seq[-1] != a:
            seq.append(a)
        seq.append(b)
    seq += [c for c in queries + classes if c not in seq[len(head):]]   # every class occurs, the query classes behind the head
    seq += ["EMPTY", "U"]                   # the one step that empties the index, and the append that follows it
    assert len(seq) <= max(nsteps, NSTEPS), (flavour, seed, len(seq))
    fill = [c for c in classes if c not in ("QB", "R")]   # the large batch and the re-upload occur where a pair needs them
    while len(seq) < nsteps:
        seq.append(str(rng.choice(fill)))
    return seq[:nsteps]   # a shorter schedule is a prefix of the longer one


class _Gen:
    def __init__(self, flavour, seed):
        self.m = IndexModel(flavour)
        self.rng = np.random.default_rng([seed, 1])
        self.flavour, self.seed, self.nknob = flavour, seed, 0
        self.took_largest = False
        self.qk_both = False
        self.after_latency_reupload = False
        self.uploads = 0                    # re-uploads so far; the first K step after each upload prepares the latency walk
        self.prepared_for = -1
        self.saved = None                   # the rows the empty-index step removed: the next append brings them back

    # -- helpers --
    def queries(self, nq):
        q = self.m.c["queries"]
        return (int(self.rng.integers(0, len(q))) + np.arange(nq)) % len(q)

    def differing(self, nq, k, max_codes, pruning):
        """Query rows whose filtered oracle answer differs from the unfiltered one (condition of every filtered step under
        a non-empty filter); any rows without such a filter."""
        m = self.m
        qi = self.queries(nq)
        if m.filter is None or not m.pass_rows().any():
            return qi
        q = m.c["queries"]
        a = m.expect_search(q, k, max_codes=max_codes, pruning=pruning)[1]
        b = m.expect_search(q, k, max_codes=max_codes, pruning=pruning, filtered=False)[1]
        diff = np.nonzero((a != b).any(1))[0]
        assert len(diff), "fixture: the filter changes no query's answer"
        for s in range(len(q)):
            if np.isin((qi + s) % len(q), diff).any():
                return (qi + s) % len(q)

    def fresh_ids(self, n):
        m, rng = self.m, self.rng
        if m.base is not None:          # labels are rows of the base store
            pool = np.setdiff1d(np.arange(len(m.base), dtype=np.uint32), m.c["ids"])
            return rng.choice(pool, min(n, len(pool)), replace=False).astype(np.uint32)
        reuse = np.setdiff1d(m.removed, m.c["ids"])
        k = min(len(reuse), n // 3) if rng.random() < 0.4 else 0   # now and then labels an earlier step removed
        new = np.arange(m.next_id, m.next_id + n - k, dtype=np.uint32)
        m.next_id += n - k
        return rng.permutation(np.concatenate([rng.choice(reuse, k, replace=False).astype(np.uint32), new]))

    def pruning(self):
        return bool(self.m.grouping and self.rng.random() < 0.5)

    # -- one step of each class --
    def U(self):
        m, rng = self.m, self.rng
        if self.saved is not None:      # after the empty index: its rows again, shuffled, under their old labels
            kind, a = self.saved
            self.saved = None
            return kind, a
        r = rng.random() if self.took_largest else 0.3   # a schedule's first update is the removal that takes the largest list
        if m.grouping and r < 0.2 and m.gone.any():
            cand = np.nonzero(m.gone)[0]
            return "add_groups", dict(which=rng.choice(cand, min(len(cand), int(rng.integers(1, 5))), replace=False))
        if r < 0.45:
            return self.removal()
        n = int(rng.choice([1, 37, 500, 1500]))
        ids = self.fresh_ids(n)
        n = len(ids)
        if not m.grouping and m.c["opq_A"] is None and rng.random() < 0.5 and n:
            x = (m.c["base"][rng.integers(0, len(m.c["base"]), n)] + rng.normal(0, 3.0, (n, m.c["d"]))).astype(np.float32)
            keep = m.encode(x)[2] <= 254       # the encoder's norm code 255 would collide with filter_ref.poisoned's
            return "add", dict(x=np.ascontiguousarray(x[keep]), ids=ids[keep])
        lists = np.nonzero(~m.gone)[0] if m.grouping else np.arange(m.nc)
        a = dict(list_idx=rng.choice(lists, n).astype(np.uint32), ids=ids,
                 codes=rng.integers(0, 256, (n, m.M)).astype(np.uint8), norm_codes=rng.integers(0, 255, n).astype(np.uint8))
        if m.grouping:
            return "append_grouping", dict(a, sub_idx=rng.integers(0, m.c["nsubc"], n).astype(np.uint32))
        return "append_ivf", dict(a, dev=bool(rng.random() < 0.5))

    def removal(self):
        m, rng = self.m, self.rng
        ids, off = m.c["ids"], m.c["offsets"].astype(np.int64)
        lab = [rng.choice(ids, min(len(ids) // 2, int(rng.choice([1, 50, 1000]))), replace=False)]
        lab.append(np.arange(3 * 10 ** 6, 3 * 10 ** 6 + 20, dtype=np.uint32))         # absent
        lab.append(lab[0][::2])                                                       # repeated
        if not self.took_largest:                                                     # once: every row of the largest list
            big = int(np.argmax(np.diff(off)))
            lab.append(ids[off[big]:off[big + 1]])
            self.took_largest = True
        elif rng.random() < 0.25:                                                     # now and then a whole list
            cc = int(rng.integers(0, m.nc))
            lab.append(ids[off[cc]:off[cc + 1]])
        lab = rng.permutation(np.concatenate(lab).astype(np.uint32))
        assert (~np.isin(ids, lab)).any(), "only the dedicated step empties the index"
        return "remove_ids", dict(labels=lab)

    def EMPTY(self):
        m = self.m
        ids, n = m.c["ids"], m.n
        p = self.rng.permutation(n)
        a = dict(ids=ids[p], codes=m._lists()[2][p], norm_codes=m.c["norm_codes"][p])
        if m.grouping:
            lst, sub = gar.rows_of(m.c["offsets"], m.c["subgroup_sizes"])
            self.saved = ("append_grouping", dict(a, list_idx=lst[p].astype(np.uint32), sub_idx=sub[p].astype(np.uint32)))
        else:
            lst = recon_ref.row_lists(m.c["offsets"], np.arange(n))
            self.saved = ("append_ivf", dict(a, list_idx=lst[p].astype(np.uint32), dev=False))
        assert n > 0 and len(np.unique(ids)) == n
        return "empty_index", dict(labels=self.rng.permutation(ids), qi=self.queries(48))

    def F(self):
        m, rng = self.m, self.rng
        ids = m.c["ids"]
        r = rng.random()
        if m.filter is not None and r < 0.35:
            return "clear_filter", {}
        if r > 0.85:                                              # an allow set naming no resident row
            return "set_filter", dict(labels=np.arange(4 * 10 ** 6, 4 * 10 ** 6 + 50, dtype=np.uint32), deny=False)
        frac = float(rng.choice([0.5, 0.1, 0.01]))
        passing = rng.choice(ids, max(1, int(frac * len(ids))), replace=False).astype(np.uint32)
        # half of the labels appends will take next
        future = np.arange(m.next_id, m.next_id + 400, 2, dtype=np.uint32) if m.base is None else \
            np.arange(len(m.base) - BASE_EXTRA, len(m.base), 2, dtype=np.uint32)
        if rng.random() < 0.5:
            return "set_filter", dict(labels=rng.permutation(np.concatenate([passing, future])), deny=False)
        return "set_filter", dict(labels=rng.permutation(np.concatenate([np.setdiff1d(ids, passing), future])).astype(np.uint32),
                                  deny=True)

    def R(self):
        self.uploads += 1
        return "reupload", {}

    def K(self):
        m, rng = self.m, self.rng
        if not m.latency and (self.prepared_for < 0 or rng.random() < 0.3):   # a schedule's first K step: one R follows it
            self.prepared_for = self.uploads
            return "prepare_latency", {}
        knobs = [("set_batch_split", dict(permille=0)), ("scan_pipe", dict(value=0)), ("set_profiling", dict(on=True)),
                 ("set_batch_split", dict(permille=300)), ("scan_pipe", dict(value=1)), ("set_profiling", dict(on=False)),
                 ("set_batch_split", dict(permille=1000)), ("scan_pipe", dict(value=-1))]
        self.nknob += 1     # in turn, from a start that differs by seed: the committed seeds together set every value
        return knobs[(self.seed + self.nknob) % len(knobs)]

    def E(self):
        grouping = ("append_ivf_on_grouping",) if self.m.grouping else ("append_bad_list",)
        return "refused", dict(what=str(self.rng.choice(("ef_below_nprobe", "nprobe_0", "one_coarse_array", "nan_radius",
                                                         "bad_option") + grouping)))

    def Q1(self):
        rng = self.rng
        a = dict(nq=int(rng.choice([7, 48])), dev=bool(rng.random() < 0.5), max_codes=int(rng.choice([1, 300, 2000, 10 ** 9])),
                 coarse=bool(rng.random() < 0.25), pruning=self.pruning())
        return "q1", dict(a, qi=self.differing(a["nq"], 1, a["max_codes"], a["pruning"]))

    def QL(self):
        a = dict(nq=int(self.rng.choice([1, 2, 8])), pruning=self.pruning())
        return "ql", dict(a, qi=self.differing(a["nq"], 1, MAX_CODES, a["pruning"]))

    def QK(self):
        m, rng = self.m, self.rng
        k = 1000 if not self.qk_both else int(rng.choice([2, 10, 100, 1000]))
        a = dict(k=k, heap=bool(rng.random() < 0.5), pruning=self.pruning(), max_codes=MAX_CODES)
        if k == 1000 and not self.qk_both:   # a query that scores fewer than k codes and one that scores more
            for pruning, mc in [(p, mc) for p in (a["pruning"], False) for mc in (MAX_CODES, 1100, 900, 700)]:
                ncode = m.scored(m.c["queries"], max_codes=mc, pruning=pruning)["ncode"]   # pruning scores a few hundred codes
                if (ncode < k).any() and (ncode > k).any():
                    a["max_codes"], a["pruning"], self.qk_both = mc, pruning, True
                    break
        return "qk", dict(a, qi=self.differing(48, k, a["max_codes"], a["pruning"]))

    def QR(self):
        m, rng = self.m, self.rng
        a = dict(max_codes=int(rng.choice([300, 2000])), pruning=self.pruning(), qi=self.queries(48))
        want = rng.choice(["0.0005", "0.1", "inf"])
        if want == "inf":
            return "qr", dict(a, radius=INF)
        sc = m.scored(m.c["queries"][a["qi"]], max_codes=a["max_codes"], pruning=a["pruning"])
        for quant in ([0.0005, 0.1] if want == "0.0005" else [0.1, 0.0005]):   # the other quantile where one leaves no query empty
            r = range_ref.pooled_quantile(sc, quant)
            per = np.array([(d < r).sum() for d in sc["dists"]])
            if (per == 0).any() and (per > 0).any():
                return "qr", dict(a, radius=r)
        raise AssertionError("fixture: no finite radius leaves both empty and non-empty queries")

    def QX(self):
        m, rng = self.m, self.rng
        lab = [rng.choice(m.c["ids"], 40), m.removed[:20], np.arange(m.next_id - 10, m.next_id + 10, dtype=np.uint32),
               np.array([0xffffffff, 5 * 10 ** 6], np.uint32)]
        return "qx", dict(labels=rng.permutation(np.concatenate(lab).astype(np.uint32)), k=int(rng.choice([1, 10])),
                          qi=self.queries(48), pruning=self.pruning())

    def QB(self):
        return "qb", dict(n=8192, pruning=self.pruning())

    def V(self):
        _, qr = self.QR()
        return "view", dict(qr, nq=int(self.rng.choice([7, 48])))

    # -- base store --
    def UB(self):
        m, rng = self.m, self.rng
        n = len(m.base)
        r = int(rng.integers(0, 4))
        if r == 0:
            first, count = int(rng.integers(1, n - 600)), int(rng.choice([1, 33, 600]))
            return "upload_base", dict(first=first, rows=rng.integers(0, 256, (count, m.base.shape[1])).astype(np.uint8))
        if r == 1:
            frac = float(rng.choice([0.5, 0.03]))
            lab = np.flatnonzero(rng.random(n) < frac).astype(np.uint32)
            return "set_base_filter", dict(labels=np.concatenate([lab, lab[:3], [n, n + 37]]).astype(np.uint32),
                                           deny=bool(rng.random() < 0.5))
        if r == 2 and m.base_filter is not None:
            return "clear_base_filter", {}
        key = str(rng.choice(["exact_range_map", "exact_filter_form", "exact_splits"]))
        return "exact_option", dict(key=key, value=int(rng.choice([-1, 1, 3] if key == "exact_splits" else [-1, 0, 1])))

    def XS(self):
        return "exact_search", dict(k=int(self.rng.choice([1, 10, 100])), qi=self.queries(48))

    def XR(self):
        m = self.m
        qi = self.queries(48)
        dist = exact_ref.distances(m.base, queries_u8(m.c["queries"][qi]))[:, m.base_mask()]
        radius = np.float32(np.quantile(dist, 0.002)) if dist.size else np.float32(1.0)
        return "exact_range", dict(radius=radius, qi=qi)

    def RR(self):
        return "rerank", dict(kc=int(self.rng.choice([10, 100])), k=int(self.rng.choice([1, 10])), qi=self.queries(48))

    def SR(self):
        return "search_rerank", dict(kc=int(self.rng.choice([10, 100])), k=int(self.rng.choice([1, 10])), qi=self.queries(48))


@functools.lru_cache(maxsize=None)
def schedule(flavour, seed, nsteps=NSTEPS):
    """The steps [(kind, arguments)] of one schedule: a pure function of its arguments."""
    g = _Gen(flavour, seed)
    steps = []
    for cls in class_sequence(flavour, seed, nsteps):
        if cls == "R" and g.m.latency:
            g.after_latency_reupload = True
        kind, a = getattr(g, cls)()
        steps.append((kind, a))
        apply(g.m, kind, a)
        if kind in UPDATE_KINDS:   # labels stay unique: range_ref.expected_ivf needs that
            assert len(np.unique(g.m.c["ids"])) == g.m.n
            assert g.m.n > 0 or kind == "empty_index"
    if nsteps >= NSTEPS:
        assert g.qk_both, "fixture: no k = 1000 step with queries on both sides of k"
        assert g.took_largest
        assert g.after_latency_reupload or "R" not in CLASSES[flavour]
    return steps


def classes_of(steps):
    return [KIND_CLASS[kind] for kind, _ in steps]
