"""GPU tier: one slot table for every forward (one_table_cases.py).  The engine skips writing the device table when the next forward's table
is the one it already holds; one engine driven through every mode in turn -- tables of different content and length, the same table twice --
must give, call for call, the bits of the same call on a fresh engine.  smoke()'s shape (64 x 64, full widths, K = 2, n_blocks 0), max_batch 3."""
import pytest

import one_table_cases as tc

pytestmark = pytest.mark.gpu


def test_no_stale_table():
    tc.check_stale_table(tc.Net(n_blocks=0, ngf=64, size=(64, 64), dev="cuda"))
