"""tests/tile_loop.py's table of tile sizes against the library, without a GPU.  tests/test_gpu_tile_loop.py sizes its
batches by that table so that workgroups walk past their first tile; a stale entry would not fail there, the batches
would only stop wrapping.  CPU only."""
import pytest

from tile_loop import GRID_BLOCKS, SIREN_ROWS, batch_sizes


@pytest.fixture(scope="module")
def lib():
    from mri_interpolation_amd import _lib
    from mri_interpolation_amd.build import build
    build()
    return _lib.load()


@pytest.mark.parametrize("hidden", sorted(SIREN_ROWS))
def test_siren_tile_rows_are_the_librarys(lib, hidden):
    """One sine layer has no weight-gradient term: mri_siren_backward_workspace_bytes(n, hidden, 1) is chain_blocks x
    SirenBwdSlab::floats() rounded to 256 bytes (siren_chain.hip slab_region_bytes), chain_blocks = min(ceil(n / R), 256).  So
    it still grows from n = 255 R to 256 R and no longer from there.  A table entry below the library's R is still
    under the cap at 256 R, where one more row adds a workgroup: the equalities fail.  An entry above it is at the cap
    at 255 R already: the inequality fails."""
    rows = SIREN_ROWS[hidden]
    need = lambda n: lib.mri_siren_backward_workspace_bytes(n, hidden, 1)  # noqa: E731
    t = GRID_BLOCKS * rows
    assert 0 < need(t - rows) < need(t)
    assert need(t) == need(t + 1) == need(2 * t)
    assert need(t - rows) > need(t - 2 * rows) and need(t - rows + 1) == need(t)  # 255 tiles + 1 row: the 256th tile


def test_batch_sizes():
    assert batch_sizes(64) == {"T": 16384, "T+1": 16385, "T+R+3": 16451, "2T+R+3": 32835}
