"""BaselineLayout's station-pair index table on the CPU: each layout gets
a table that describes ITS pair order, whatever an earlier layout of the
same (N, Nbase) left in the cache. Nothing here touches the extension."""
import numpy as np
import torch

from sagecal_amd.ops import hip_host
from sagecal_amd.ops.hip_host import BaselineLayout

N = 6
CANON = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
NBASE = len(CANON)


def mixed_table():
    """Odd-numbered pairs stored (q, p), rows in a fixed permutation."""
    t = CANON.copy()
    t[1::2] = t[1::2, ::-1]
    return t[np.random.default_rng(1).permutation(NBASE)]


def layout(table, T=2):
    bb = torch.tensor(np.tile(table, (T, 1)))
    return BaselineLayout(bb, len(table), T, 1, N, 'cpu')


def check_own_table(lay, table):
    """pidx[min, max] == b for every unflagged pair b of the layout."""
    assert lay.pairs.tolist() == table.tolist()
    for b, (p, q) in enumerate(table):
        if p < 0:
            continue
        assert int(lay.pidx[min(p, q), max(p, q)]) == b, (b, p, q)


def test_each_layout_gets_its_own_pair_order():
    hip_host._pidx_cache.clear()
    mixed = mixed_table()
    assert mixed.tolist() != CANON.tolist()
    first = layout(CANON)
    check_own_table(first, CANON)
    second = layout(mixed)
    check_own_table(second, mixed)
    # the first layout keeps the table it was built with
    check_own_table(first, CANON)
    third = layout(CANON)
    check_own_table(third, CANON)
    assert torch.equal(third.pidx, first.pidx)


def test_same_tensor_after_another_layout():
    """The same bb tensor object, used again after a different table took
    the cache slot, still gets its own table."""
    hip_host._pidx_cache.clear()
    bb = torch.tensor(np.tile(CANON, (2, 1)))
    a = BaselineLayout(bb, NBASE, 2, 1, N, 'cpu')
    layout(mixed_table())
    b = BaselineLayout(bb, NBASE, 2, 1, N, 'cpu')
    check_own_table(b, CANON)
    assert torch.equal(a.pidx, b.pidx)
    # edited in place: the table follows the contents, not the object
    bb[:] = torch.tensor(np.tile(mixed_table(), (2, 1)))
    check_own_table(BaselineLayout(bb, NBASE, 2, 1, N, 'cpu'),
                    mixed_table())


def test_flagged_rows_reuse_the_full_table():
    """A table that differs from the cached one only by flagged (-1) rows
    reuses it: the table still lists the flagged pairs, whose slots the
    kernels skip through `pairs`."""
    hip_host._pidx_cache.clear()
    full = layout(CANON)
    flagged = CANON.copy()
    flagged[[3, 7]] = -1
    lay = layout(flagged)
    check_own_table(lay, flagged)
    assert lay.pidx is full.pidx
    p, q = CANON[7]
    assert int(lay.pidx[p, q]) == 7 and int(lay.pairs[7, 0]) == -1


def test_full_table_after_a_flagged_one():
    """The other order: the cached table lacks the flagged pairs, so the
    full layout cannot reuse it."""
    hip_host._pidx_cache.clear()
    flagged = CANON.copy()
    flagged[[3, 7]] = -1
    lay = layout(flagged)
    p, q = CANON[7]
    assert int(lay.pidx[p, q]) == -1
    check_own_table(layout(CANON), CANON)


def test_all_rows_flagged():
    hip_host._pidx_cache.clear()
    lay = layout(np.full_like(CANON, -1))
    assert int(lay.pidx.max()) == -1
    check_own_table(layout(CANON), CANON)
