"""GPU suite: concat_copy (csrc/nc_copy.h), the one device body behind every ragged, session and stream copy, alone.

nc_op_concat_copy runs a table of descriptors (a_off, na, b_off, nb, s0, dst_off, n) as ONE launch, grid.y = the table's length:
dst[dst_off + j] = (a[a_off : a_off + na] ++ b[b_off : b_off + nb] ++ zeros)[s0 + j] for j < n.  The body splits a destination run at its
first 16-byte boundary (scalar head, 16-byte stores, scalar tail) and loads a vector whole where it lies 16-byte aligned in one piece,
so the table crosses every misalignment of destination and pieces with piece lengths around the vector width V = 16 / itemsize.  The
expectation is numpy's concatenate, pad and slice, compared bit for bit; dst is pre-filled with a sentinel that must survive everywhere
outside the descriptors' [dst_off, dst_off + n) -- the off-by-one the split can make."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from neuralcodecs_amd import ops  # noqa: E402

SRC_LEN = 8192


def _table(dtype):
    """-> (a, b, descriptors [n, 7]); destinations laid out one behind the other with gaps, every one at its own misalignment"""
    V = 16 // np.dtype(dtype).itemsize
    lens = (0, 1, V - 1, V, V + 1, 2 * V + 1)
    desc, cursor, k = [], V, 0

    def add(dm, am, bm, na, nb, s0, n):
        nonlocal cursor, k
        a_off = V * (1 + k % 5) + am                   # the pieces start at several vectors of their arrays, misaligned by am / bm
        b_off = V * (2 + k % 3) + bm
        dst_off = (cursor + V - 1) // V * V + dm       # behind the last destination, at least one untouched element in between
        desc.append((a_off, na, b_off, nb, s0, dst_off, n))
        cursor = dst_off + n + 1
        k += 1

    for dm, am, bm, na, nb, z, s0 in itertools.product(range(V), range(V), range(V), lens, lens, (0, 1, V + 1), (0, 1, V)):
        if s0 < na + nb:
            add(dm, am, bm, na, nb, s0, na + nb - s0 + z)
    for dm in range(1, V):                             # runs that end inside the head or exactly with it: the head consumes the run
        for n in range(1, V - dm + 1):
            add(dm, 1, 0, 2 * V + 1, V, 1, n)          # ... out of the first piece
            add(dm, 0, 1, 0, 2 * V + 1, 0, n)          # ... out of the second
            add(dm, 0, 0, 0, 0, 0, n)                  # ... of zeros alone
    add(1, 1, V - 1, 2501, 2600, 3, 2501 + 2600 - 3 + 7)   # about 5000 elements: more than one block strides along x
    rng = np.random.default_rng(5)
    a = rng.integers(1, 1 << 20, SRC_LEN).astype(dtype)    # no element is zero or the sentinel
    b = -rng.integers(1, 1 << 20, SRC_LEN).astype(dtype)
    return a, b, np.array(desc, np.int64), cursor + V


@pytest.mark.parametrize("dtype", [np.float32, np.int64], ids=["float32", "int64"])
def test_concat_copy_every_alignment_and_length_in_one_launch(dtype):
    a, b, desc, dst_n = _table(dtype)
    assert 2000 < len(desc) <= 65535
    sentinel = dtype(-77)
    dst = np.full(dst_n, sentinel, dtype)
    want = dst.copy()
    covered = np.zeros(dst_n, bool)
    for a_off, na, b_off, nb, s0, dst_off, n in desc:
        cat = np.concatenate([a[a_off:a_off + na], b[b_off:b_off + nb]])
        cat = np.pad(cat, (0, max(0, s0 + n - cat.size)))
        assert not covered[dst_off:dst_off + n].any(), "the test's own layout: destinations must not overlap"
        covered[dst_off:dst_off + n] = True
        want[dst_off:dst_off + n] = cat[s0:s0 + n]
    assert not covered.all() and not covered[desc[:, 5] - 1].any() and not covered[desc[:, 5] + desc[:, 6]].any()   # a gap on both sides of every run
    got = ops.concat_copy(a, b, dst, desc)
    assert got.dtype == dst.dtype
    assert np.array_equal(got[~covered], want[~covered]), "an element outside every descriptor lost the sentinel"
    assert np.array_equal(got, want)
