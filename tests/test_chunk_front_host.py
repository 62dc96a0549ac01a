"""The seam batch of tests/chunk_inputs.py holds what it promises: checked on the arrays it returns, so that an edit to the
builder cannot silently lose a seam.  No GPU."""
import numpy as np
import pytest

import chunk_inputs as ci
import graph_model as gm

KS = (5, 31, 32, 33, 63)


@pytest.mark.parametrize("k", KS)
def test_seam_batch_holds_every_seam(k):
    bases, offs = ci.seam_batch(k)
    o = offs.astype(np.int64)
    n = len(bases)
    assert bases.dtype == np.uint8 and offs.dtype == np.uint64 and o[0] == 0 and o[-1] == n and (np.diff(o) >= 0).all()
    assert 5 * ci.CHUNK < n < 5 * ci.CHUNK + 200 and n % ci.LANE != 0
    lens = np.diff(o)
    acgt = np.isin(bases, np.frombuffer(b"ACGT", np.uint8))
    # a stretch of at least 1024 positions cut into reads of 0 to 8 bases: several hundred starts in one chunk
    tiny = np.flatnonzero(o[:-1] < ci.CHUNK)
    assert o[tiny[-1] + 1] == ci.CHUNK and lens[tiny].max() <= 8 and lens[tiny].min() == 0
    assert len(tiny) >= 200 and len(tiny) > 3 * ci.HELD
    # a run of at least 70 empty reads at one position
    at, run = np.unique(o[:-1][lens == 0], return_counts=True)
    assert run.max() >= 70 and run.max() > ci.HELD and at[run.argmax()] % ci.CHUNK != 0
    # a read that starts exactly at 1024 and one at 2048 + 16, both with bases; a read that ends exactly at 3072
    nonempty_starts = set(o[:-1][lens > 0].tolist())
    assert ci.CHUNK in nonempty_starts and 2 * ci.CHUNK + ci.LANE in nonempty_starts
    assert 3 * ci.CHUNK in set(o[1:][lens > 0].tolist())
    # non-ACGT bytes: at 1023, at 1024, and in the first position of a window that straddles 2048 inside one read
    bad = np.flatnonzero(~acgt).tolist()
    assert bad == sorted(ci.bad_positions(k)) and ci.CHUNK - 1 in bad and ci.CHUNK in bad
    first = [p for p in bad if p < 2 * ci.CHUNK <= p + k - 1]
    assert len(first) == 1
    r = int(np.searchsorted(o, first[0], side="right")) - 1
    assert o[r] <= first[0] and first[0] + k <= o[r + 1] and acgt[first[0] + 1:first[0] + k].all()
    # one read of at least 2 * 1024 + k bases, free of breaks, over two chunk edges
    lr = int(lens.argmax())
    a, b = int(o[lr]), int(o[lr + 1])
    assert b - a >= 2 * ci.CHUNK + k and acgt[a:b].all() and (b - 1) // ci.CHUNK - a // ci.CHUNK >= 2
    # counts above 1 occur
    table = gm.count_table(ci.reads_of(bases, offs), k, True)
    assert max(table.values()) > 1 and len(table) > (500 if k > 5 else 100)
