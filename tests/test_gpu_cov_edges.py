"""The coverage engine of `paffy tile` and `paffy to_bed` on its edges: the cigar reader of k_cov_bitmap in both workgroup shapes (numbers
across a round and a lane boundary, the serial walk, the halo, the first tile), its LDS window against the straight path into HBM, the
slice walk, the runs and lines of k_bed_runs / k_bed_lines and the median of k_cov_merge. Every comparison is byte equality with the
oracle plus the same error code and record; the inputs are cov_edges_lib's, and test_cov_edges_cpu.py shows on the oracle and the
predictor that they hit their cases."""
import os

import pytest

import cov_edges_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


@pytest.mark.parametrize("batch", L.error_free_batches(), ids=lambda b: b.name)
def test_error_free_cases(eng, batch):
    """to_bed, to_bed -n and tile of every error-free batch (groups 1 to 4, 6, 7, 9 to 11), + and - records, both shapes"""
    L.check(eng, batch.data)


@pytest.mark.parametrize("batch", L.failing_batches(), ids=lambda b: b.name)
def test_failing_cases(eng, batch):
    """group 5 and the length that wraps negative: the reference's error, its record, nothing written"""
    L.check(eng, batch.data)


@pytest.mark.parametrize("batch", L.error_free_batches(), ids=lambda b: b.name)
def test_chunks_and_batches_give_the_same_bytes(eng, batch):
    """group 8: the walk cut into chunks of entries (a bitmap budget of 1 MiB) and the text held as small batches -- every cg_off & 15 and
    every bitmap base changes, the bytes do not"""
    os.environ["PAFFY_COV_BITMAP_MB"] = "1"
    try:
        L.check(eng, batch.data)
        L.check(eng, batch.data, batch_bytes=50_000)
    finally:
        del os.environ["PAFFY_COV_BITMAP_MB"]
    L.check(eng, batch.data, batch_bytes=23_456)


def test_runs_under_binary(eng):
    """group 9 again with -b: a run breaks where covered meets uncovered, and still at every sequence boundary"""
    data = L.runs_batch().data
    for kw in (dict(binary=True), dict(binary=True, exclude_unaligned=True)):
        L.check(eng, data, modes=("bed", "bed_n"), **kw)
    L.check(eng, L.boundary_batch(64).data, modes=("bed", "bed_n"), binary=True)


def test_lines_under_every_option(eng):
    """group 10: waves of 64 lines below, at and above the LDS stage, with min_size / exclude_aligned / exclude_unaligned dropping some, all
    but a few, or all of a wave's lines"""
    data = L.lines_batch().data
    for kw in L.LINE_OPTS:
        L.check(eng, data, modes=("bed", "bed_n"), **kw)


def test_coordinates_of_ten_digits(eng):
    L.check(eng, L.ten_digit_batch().data, modes=("bed",))
    L.check(eng, L.ten_digit_batch().data, modes=("bed",), exclude_unaligned=True)
