"""Expected values of filtered searches without new oracle code.

From a corpus c: b = c with norm_codes clipped to <= 254, p = b with norm_table[255] = +inf and norm_codes = 255 on
every row that does not pass.  A search of p never admits such a row (inf < FLT_MAX is false) and visits what a search
of b visits, so the oracle on p, or an unfiltered handle that uploaded p, is what a filtered search of b must return."""
import numpy as np


def clipped(c):
    return dict(c, norm_codes=np.minimum(c["norm_codes"], 254).astype(np.uint8))


def passing(ids, labels, deny=False):
    """Row mask: ids in labels (deny: not in labels)."""
    m = np.isin(ids, np.asarray(labels, np.uint32))
    return ~m if deny else m


def poisoned(b, pass_rows):
    assert not pass_rows.any() or b["norm_codes"][pass_rows].max() <= 254  # a passing row must keep a finite norm
    nt = b["norm_table"].copy()
    nt[255] = np.inf
    nc = b["norm_codes"].copy()
    nc[~pass_rows] = 255
    return dict(b, norm_table=nt, norm_codes=nc)
