"""CPU: the one argument contract of the streaming score calls (rank_of, the softmax over the corpus, range search) without a device -- the
leading-dimension rule of a score matrix, which every scores_* wrapper of rails_amd.engine takes from one function."""
import pytest

from rails_amd import engine as E


@pytest.mark.parametrize("rows,n,stride0,ld", [(1, 70, 1, 70), (1, 70, 128, 128), (2, 70, 128, 128), (0, 70, 70, 70)])
def test_a_single_row_goes_as_a_row_of_at_least_n(rows, n, stride0, ld):
    """More than one row: the rows lie where their stride says.  One row or none: the stride is whatever the view it was cut from carries, and
    the kernels (ld >= n) are given at least n."""
    assert E.score_matrix_ld(rows, n, stride0) == ld
