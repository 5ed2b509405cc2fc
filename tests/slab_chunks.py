"""What the slab-chunk tests of the row-per-lane units share (tests/test_gpu_schnorr.py, test_gpu_ecvrf.py, test_gpu_pairing.py).

Every variable-base launch and every pairing launch cuts its batch into chunks whose per-row slab stays under 1 GB: more than
2^17 rows, so no test of a few hundred rows would ever reach a chunk after the first, where the kernels index the slab by the
row within the chunk and everything else by the row of the batch.  GH_TEST_SLAB_ROWS=128 caps a chunk at 128 rows: N = 261 rows
are then chunks of 128, 128 and 5, a full later chunk and a short tail.  While the knob is set each launch function says on
stderr how it cut its batch, so a test can tell that the chunks ran."""
import re

import numpy as np

KNOB = "GH_TEST_SLAB_ROWS"
N = 261
SAMPLE = (0, 127, 128, 129, 255, 256, 260)          # the rows compared with the Python restatement: both sides of every chunk edge
THREE = [(N, 128, 3)]                               # the chunk line of one launch of N rows


def chunk_lines(err, loop):
    """the (n, rows per chunk, chunks) of every chunk line that the launch function `loop` wrote"""
    pat = r"^\[gh\] slab chunks: %s n=(\d+) rows=(\d+) chunks=(\d+)$" % re.escape(loop)
    return [tuple(int(x) for x in m.groups()) for m in re.finditer(pat, err, re.M)]


def plain_and_cut(monkeypatch, capfd, fn):
    """fn() without the knob, then under GH_TEST_SLAB_ROWS=128 -> (result, result under the knob, stderr under the knob).
    Without the knob nothing is printed."""
    monkeypatch.delenv(KNOB, raising=False)
    capfd.readouterr()
    plain = fn()
    assert "slab chunks" not in capfd.readouterr().err
    monkeypatch.setenv(KNOB, "128")
    cut = fn()
    err = capfd.readouterr().err
    monkeypatch.delenv(KNOB)
    return plain, cut, err


def identical(a, b):
    """bit-identical arrays, or tuples of them"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(identical(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and np.array_equal(a, b)


def assert_rows_differ(*columns):
    """every column (one hashable input per row) has N pairwise distinct entries: in particular row i differs from rows
    i - 128 and i - 256 in every input, so a kernel that read an input by the row within the chunk could not pass"""
    for col in columns:
        assert len(col) == N and len(set(col)) == N
