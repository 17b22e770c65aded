"""Argument handling of the test hooks hbec_set_vec_chunk_tiles and
hbec_set_vec_grid_cap (CPU only: they set process-wide launch parameters and
touch no device), and the store depth report."""
import pytest

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B


@pytest.fixture(autouse=True)
def _restore():
    yield
    B.set_vec_chunk_tiles(0)
    B.set_vec_grid_cap(0)


def test_defaults_and_zero_restores_them():
    tiles0, cap0 = B.vec_launch_config()
    assert tiles0 > 0 and cap0 == 0
    B.set_vec_chunk_tiles(12)
    B.set_vec_grid_cap(3)
    assert B.vec_launch_config() == (12, 3)
    B.set_vec_chunk_tiles(0)
    assert B.vec_launch_config() == (tiles0, 3)
    B.set_vec_grid_cap(0)
    assert B.vec_launch_config() == (tiles0, 0)


def test_bounds():
    tiles0, _ = B.vec_launch_config()
    B.set_vec_chunk_tiles(1 << 31)
    assert B.vec_launch_config()[0] == 1 << 31
    assert N.lib().hbec_set_vec_chunk_tiles((1 << 31) + 1) != 0
    assert B.vec_launch_config()[0] == 1 << 31  # a refused value changes nothing
    assert N.lib().hbec_set_vec_grid_cap(-1) != 0
    assert B.vec_launch_config()[1] == 0
    with pytest.raises(Exception):
        B.set_vec_grid_cap(-5)
    B.set_vec_chunk_tiles(0)
    assert B.vec_launch_config()[0] == tiles0


def test_store_depth_report():
    t, run = B.pipe2_store_depth(4, 2)
    assert t >= 1 and (t > 1 or not run)
    # the depth is staged per lane in at most 128 registers (4 per 16-B result)
    assert t * 2 * 4 <= 128
    for k, r in [(1, 1), (2, 1), (3, 2), (4, 1), (4, 3), (8, 3), (16, 4)]:
        assert B.pipe2_store_depth(k, r) == (1, False), (k, r)
    assert N.lib().hbec_pipe2_store_depth(0, 2, None, None) != 0
    assert N.lib().hbec_pipe2_store_depth(4, 5, None, None) != 0
