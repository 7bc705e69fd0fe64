"""Every row width of the float16 base store: the four kernel families of kernels_exact_f16.hip
are instantiated for d / 16 = 1 .. 16 and the k-searches for three selection shapes besides, and each instantiation runs
here.  Integer rows 0..127, where every operation is exact: the k-searches bit for bit exact_ref / exact_tags_ref, the range
searches exact_range_ref / exact_tags_ref.

One shape for every d: n = 300 rows -- nine full tiles of 32 columns and one of 12, and under exact_splits = 3 every split
ends in a partial tile -- and nq = 70 queries -- two full strips of 32 and one of 6, two workgroups where a workgroup is 2
waves.  Base tags arange(n) % 3; query tags cycle 0, 1, 2, NONE and a tag no row carries, so one tagged call runs the Dense
launch (staged tiles) and the Indirect launch (a wave per strip, operand B in two unequal parts at odd d / 16 above 8)."""
import itertools

import numpy as np
import pytest

import exact_ref
import exact_range_ref
import exact_tags_ref as tr

pytestmark = pytest.mark.gpu

F = np.float32
DS = tuple(range(16, 257, 16))
N, NQ = 300, 70
ABSENT = 7


def _same(got, want):
    assert np.array_equal(got[1], want[1]), np.nonzero((got[1] != want[1]).any(1))[0][:5]
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _same_range(got, want):
    assert np.array_equal(got[0], want[0]), np.nonzero(got[0] != want[0])[0][:5]
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


_STORES, _WANT = {}, {}


@pytest.fixture(scope="module")
def store(pkg):
    """Per d, made once: rows, queries, base tags, query tags, the int64 distances, the pairs a tagged query may return, and a
    handle with rows and tags installed; closed with the module."""
    def get(d):
        if d not in _STORES:
            rng = np.random.default_rng(7000 + d)
            x, q = rng.integers(0, 128, (N, d), dtype=np.uint8), rng.integers(0, 128, (NQ, d), dtype=np.uint8)
            q[0] = x[N // 2]  # a zero distance; row 150 carries tag 0, as query 0 does
            btags = (np.arange(N) % 3).astype(np.uint16)
            qtags = np.array([0, 1, 2, tr.NONE, ABSENT], np.uint16)[np.arange(NQ) % 5]
            g = pkg.GpuIndex(0)
            g.upload_base_f16(x.astype(F))
            g.set_base_tags(np.arange(N, dtype=np.uint32), btags)
            mine = np.stack([tr.tag_mask(btags, t) for t in qtags])
            _STORES[d] = dict(x=x, q=q, qf=q.astype(F), btags=btags, qtags=qtags, D=exact_ref.distances(x, q), mine=mine, g=g)
        return _STORES[d]
    yield get
    for s in _STORES.values():
        s["g"].close()
    _STORES.clear()
    _WANT.clear()


def _want(key, make):
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


KSEARCH = list(itertools.product(DS, (16, 32, 100), (1, 3)))  # k: one of each selection shape (CAP 48, 64, 136)


@pytest.mark.parametrize("d,k,splits", KSEARCH)
def test_exact_search_f16(store, d, k, splits):
    s = store(d)
    s["g"].set_option("exact_splits", splits)
    _same(s["g"].exact_search_f16(s["qf"], k), _want(("k", d, k), lambda: exact_ref.search(s["x"], s["q"], k)))


@pytest.mark.parametrize("d,k,splits", KSEARCH)
def test_exact_search_f16_tags(store, d, k, splits):
    s = store(d)
    s["g"].set_option("exact_splits", splits)
    want = _want(("kt", d, k), lambda: tr.search_blocked(s["x"], s["q"], k, s["btags"], s["qtags"]))
    assert (want[1][s["qtags"] == ABSENT] == -1).all() and (want[1][s["qtags"] == 0] >= 0).all()  # (k = 100: a tag's every row)
    _same(s["g"].exact_search_f16_tags(s["qf"], k, s["qtags"]), want)


def _radii(dist):
    """An integer that some of the pairs given sit ON (strict <), their lower 5 % quantile, and the value half way to the
    next integer, which takes those pairs in."""
    low = float(np.sort(dist, axis=None)[dist.size // 20])
    return low, low + 0.5


@pytest.mark.parametrize("d,use_map", list(itertools.product(DS, (0, 1))))
def test_exact_range_search_f16(store, d, use_map):
    s = store(d)
    s["g"].set_option("exact_splits", 3)
    s["g"].set_option("exact_range_map", use_map)
    sizes = []
    for radius in _radii(s["D"]):
        want = _want(("r", d, radius), lambda: exact_range_ref.from_distances(s["D"], radius))
        sizes.append(int(want[0][-1]))
        _same_range(s["g"].exact_range_search_f16(s["qf"], radius), want)
    assert 0 < sizes[0] < sizes[1]  # pairs sat on the first radius


@pytest.mark.parametrize("d,use_map", list(itertools.product(DS, (0, 1))))
def test_exact_range_search_f16_tags(store, d, use_map):
    s = store(d)
    s["g"].set_option("exact_splits", 3)
    s["g"].set_option("exact_range_map", use_map)
    sizes = []
    for radius in _radii(s["D"][s["mine"]]):
        want = _want(("rt", d, radius), lambda: tr.range_blocked(s["x"], s["q"], radius, s["btags"], s["qtags"]))
        sizes.append(int(want[0][-1]))
        _same_range(s["g"].exact_range_search_f16_tags(s["qf"], radius, s["qtags"]), want)
    assert 0 < sizes[0] < sizes[1]
