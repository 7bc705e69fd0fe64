"""One long-lived handle through a seeded schedule that mixes upserts (every form) with appends, removals, a filter and
queries.  The host model is tests/index_model.py's, unchanged: an upsert is model.remove of the batch's
labels followed by model.append of the batch.  At every query step the handle's lists equal the model's byte for byte and
the answers equal the oracle's on the model's state; at the end a fresh handle that uploads the model's state answers the
probe set with the same bits."""
import numpy as np
import pytest

import index_model as im
from index_model import EF
from test_gpu_sequences import _dev, against_fresh, check_range, check_search, check_state, upload_state

pytestmark = pytest.mark.gpu

PATTERN = ("upsert", "q1", "append", "upsert_dev", "qk", "remove", "upsert_x", "qr", "upsert", "q1",
           "set_filter", "upsert_dev", "q1", "upsert_x", "qk", "clear_filter", "remove", "upsert", "qr", "append",
           "upsert_all_of_a_list", "q1", "upsert_dev", "qk", "remove", "upsert_x", "q1", "upsert", "qr", "qk")


def _batch(m, rng, n, labels=None):
    """An upsert's batch on the model's state: half resident labels, half new ones, random lists."""
    if labels is None:
        k = min(n // 2, m.n)
        labels = np.concatenate([rng.choice(m.c["ids"], k, replace=False), np.arange(m.next_id, m.next_id + n - k, dtype=np.uint32)])
        m.next_id += n - k
        labels = rng.permutation(labels.astype(np.uint32))
    n = len(labels)
    return dict(list_idx=rng.integers(0, m.nc, n).astype(np.uint32), ids=np.asarray(labels, np.uint32),
                codes=rng.integers(0, 256, (n, m.M)).astype(np.uint8), norm_codes=rng.integers(0, 255, n).astype(np.uint8))


def _model_upsert(m, a):
    want = m.remove(a["ids"])
    m.append(a["list_idx"], a["ids"], a["codes"], a["norm_codes"])
    return want


def _step(g, m, rng, kind):
    q = m.c["queries"]
    keys = ("list_idx", "ids", "codes", "norm_codes")
    if kind in ("upsert", "upsert_dev", "upsert_all_of_a_list") or (kind == "upsert_x" and m.c["opq_A"] is not None):
        labels = None
        if kind == "upsert_all_of_a_list":
            off = m.c["offsets"].astype(np.int64)
            big = int(np.argmax(np.diff(off)))
            labels = m.c["ids"][off[big]:off[big + 1]].copy()
        a = _batch(m, rng, int(rng.choice([1, 37, 600, 1500])), labels)
        if kind == "upsert_dev":
            import torch
            d_per = torch.full((m.nc,), -1, dtype=torch.int32, device=torch.device("cuda", 0))
            d = [_dev(a[k]) for k in keys]
            torch.cuda.synchronize(d_per.device)
            got = (g.upsert_ivf_dev(len(a["ids"]), *d, d_removed_per_list=d_per), d_per.cpu().numpy().view(np.uint32))
        else:
            got = g.upsert_ivf(*[a[k] for k in keys])
        want = _model_upsert(m, a)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), "what upsert_ivf returns"
    elif kind == "upsert_x":
        n = int(rng.choice([33, 700]))
        x = (m.c["base"][rng.integers(0, len(m.c["base"]), n)] + rng.normal(0, 3.0, (n, m.c["d"]))).astype(np.float32)
        idx, codes, ncodes = m.encode(x)
        keep = ncodes <= 254                      # the encoder's norm code 255 would collide with filter_ref.poisoned's
        x, idx, codes, ncodes = np.ascontiguousarray(x[keep]), idx[keep], codes[keep], ncodes[keep]
        a = _batch(m, rng, len(x))
        a.update(list_idx=idx, codes=codes, norm_codes=ncodes)
        got = g.upsert(x, a["ids"], efSearch=EF)
        want = _model_upsert(m, a)
        assert np.array_equal(got[0], idx) and np.array_equal(got[1], codes) and np.array_equal(got[2], ncodes), "what upsert returns"
        assert got[3] == want[0]
    elif kind == "append":
        n = int(rng.choice([1, 500]))
        a = _batch(m, rng, n, labels=np.arange(m.next_id, m.next_id + n, dtype=np.uint32))
        m.next_id += n
        g.append_ivf(*[a[k] for k in keys])
        m.append(*[a[k] for k in keys])
    elif kind == "remove":
        lab = rng.choice(m.c["ids"], min(m.n // 3, 400), replace=False)
        got, want = g.remove_ids(lab), m.remove(lab)
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
    elif kind == "set_filter":
        passing = rng.choice(m.c["ids"], m.n // 2, replace=False)
        future = np.arange(m.next_id, m.next_id + 4000, 2, dtype=np.uint32)
        lab = np.concatenate([passing, future]).astype(np.uint32)
        g.set_filter(lab)
        m.set_filter(lab, False)
    elif kind == "clear_filter":
        g.clear_filter()
        m.clear_filter()
    else:   # a query step: the layout, then the answers
        check_state(g, m)
        if kind == "q1":
            check_search(g, m, q, 1, int(rng.choice([300, 2000])))
        elif kind == "qk":
            check_search(g, m, q, 10, heap=True)
        else:
            assert kind == "qr"
            sc = m.scored(q)
            check_range(g, m, q, im.range_ref.pooled_quantile(sc, 0.05), im.MAX_CODES, False)


@pytest.mark.parametrize("flavour", ["ivf_pq16", "ivf_opq_rt"])
def test_upsert_sequence(gpu, pkg, flavour):
    m = im.IndexModel(flavour)
    rng = np.random.default_rng([41, len(flavour)])
    g = upload_state(gpu(), m)
    i, kind = -1, "upload"
    try:
        check_state(g, m)
        for i, kind in enumerate(PATTERN):
            _step(g, m, rng, kind)
            assert len(np.unique(m.c["ids"])) == m.n
        kind = "probe set against a fresh handle"
        check_state(g, m)
        against_fresh(gpu, pkg, g, m)
    except Exception as e:
        raise AssertionError("%s, step %d (%s): %s: %s" % (flavour, i, kind, type(e).__name__, e)) from e
    finally:
        g.close()
