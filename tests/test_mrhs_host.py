"""CPU: the host helpers of the multi-vector interface.  pack_columns lays 1 to 8
vectors out as the n x k row-major array an amg_mvec holds, padded with zero columns
to the next allowed width; unpack_columns takes the columns out again."""
import numpy as np
import pytest


@pytest.mark.parametrize("count,width", [(1, 2), (2, 2), (3, 4), (5, 8), (8, 8)])
def test_pack_unpack_round_trip(amg, count, width):
    n = 37
    vecs = [np.random.default_rng(100 + j).uniform(-1, 1, n) for j in range(count)]
    a = amg.pack_columns(vecs)
    assert a.shape == (n, width) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    for j, v in enumerate(vecs):  # element (i, j) at i * k + j
        assert np.array_equal(a.ravel()[j::width].view(np.uint64), v.view(np.uint64))
    assert np.all(a[:, count:].view(np.uint64) == 0), "padding columns are exactly +0.0"
    back = amg.unpack_columns(a, count)
    assert len(back) == count
    for v, w in zip(vecs, back):
        assert w.flags["C_CONTIGUOUS"] and np.array_equal(v.view(np.uint64), w.view(np.uint64))


def test_pack_refuses_bad_input(amg):
    with pytest.raises(ValueError):
        amg.pack_columns([])
    with pytest.raises(ValueError):
        amg.pack_columns([np.zeros(3)] * 9)
    with pytest.raises(ValueError):
        amg.pack_columns([np.zeros(3), np.zeros(4)])
    with pytest.raises(ValueError):
        amg.unpack_columns(np.zeros((3, 2)), 3)
