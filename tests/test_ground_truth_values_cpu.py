"""tools/ground_truth.py --values / --query-ranges, what needs no GPU: the files it accepts and refuses
(integers that fit 32 bits unsigned, of any shape), the sizes it checks against the store and the queries before anything
is installed, and the option combinations the command line refuses before a library is loaded."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ground_truth  # noqa: E402


def _save(tmp_path, name, a):
    p = str(tmp_path / name)
    np.save(p, a)
    return p


def test_read_values_accepts_integers_of_32_bits_and_any_shape(tmp_path):
    v = ground_truth.read_values(_save(tmp_path, "v.npy", np.array([0, 1, 0x80000000, 0xfffffffe, 0xffffffff], np.uint32)))
    assert v.dtype == np.uint32 and v.tolist() == [0, 1, 0x80000000, 0xfffffffe, 0xffffffff]
    qr = ground_truth.read_values(_save(tmp_path, "qr.npy", np.array([[0, 0xffffffff], [7, 3]], np.int64)))
    assert qr.dtype == np.uint32 and qr.tolist() == [0, 0xffffffff, 7, 3]  # [nq, 2] comes back flat, an inverted pair as it is
    assert ground_truth.read_values(_save(tmp_path, "e.npy", np.zeros(0, np.uint32))).size == 0


@pytest.mark.parametrize("bad", [np.array([1.0, 2.0]), np.array([0, 1 << 32], np.int64), np.array([-1, 5], np.int64),
                                 np.array([True, False])])
def test_read_values_refuses_what_is_no_uint32(tmp_path, bad):
    with pytest.raises(ValueError):
        ground_truth.read_values(_save(tmp_path, "bad.npy", bad))


class _Handle:
    def __init__(self):
        self.calls = []

    def set_base_values(self, rows, values):
        self.calls.append((np.asarray(rows), np.asarray(values)))


def test_install_values_checks_the_sizes_before_it_installs():
    g = _Handle()
    vals = np.arange(5, dtype=np.uint32)
    ground_truth.install_values(g, 5, 3, vals, np.zeros(6, np.uint32))
    assert len(g.calls) == 1 and g.calls[0][0].tolist() == [0, 1, 2, 3, 4] and g.calls[0][0].dtype == np.uint32
    assert np.array_equal(g.calls[0][1], vals)
    for n, nq, v, qr in ((6, 3, vals, np.zeros(6, np.uint32)),    # a value short of the store
                         (5, 3, vals, np.zeros(3, np.uint32)),    # one number per query, not a pair
                         (5, 4, vals, np.zeros(6, np.uint32))):   # a pair short of the queries
        with pytest.raises(ValueError):
            ground_truth.install_values(g, n, nq, v, qr)
    assert len(g.calls) == 1


@pytest.mark.parametrize("extra", [["--values", "v.npy"], ["--query-ranges", "qr.npy"],
                                   ["--values", "v.npy", "--query-ranges", "qr.npy", "--allow", "a.npy"],
                                   ["--values", "v.npy", "--query-ranges", "qr.npy", "--deny", "a.npy"],
                                   ["--values", "v.npy", "--query-ranges", "qr.npy", "--tags", "t.npy", "--query-tags", "qt.npy"]])
def test_command_line_refuses_half_a_pair_and_a_second_predicate(extra, capsys):
    with pytest.raises(SystemExit) as e:
        ground_truth.main(["--base", "x.bvecs", "--queries", "q.bvecs", "--out", "gt.ivecs"] + extra)
    assert e.value.code == 2  # argparse's usage error, before any file is read or a library loaded
    assert "--values and --query-ranges go together" in capsys.readouterr().err
