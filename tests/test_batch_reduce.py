"""CPU: sums over the items of a device-resident batch (Evaluator_SumItems / Evaluator_DotPlainDevice) with the kernels emulated.
Against the REAL reference (oracle/_ref) where it is built, against the per-object forms on batches of one everywhere, and against
Python-integer arithmetic around the flush intervals of the lazy accumulators."""
import pytest

import sealref

needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
SIZES = [(8, [30, 30, 30]), (1024, [60, 40, 60]), (4096, [60, 40, 40, 60])]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", SIZES)
def test_parity(emu, scheme, n, bits):
    """g = 1, 2 (two output items) and the whole batch"""
    import batch_reduce_cases as BR
    BR.case_parity(scheme, n, bits, batch=4, groups=(1, 2, 4))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_group_not_a_power_of_two(emu, scheme):
    import batch_reduce_cases as BR
    BR.case_parity(scheme, 1024, [60, 40, 60], batch=15, groups=(5,), sizes=(2,))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1"""
    import batch_reduce_cases as BR
    BR.case_parity(scheme, 1024, [60, 40, 60], batch=4, groups=(2, 4), sizes=(2,), ci=0)


def test_flush_groups_come_from_the_intervals():
    import batch_reduce_cases as BR
    assert BR.flush_groups() == [15, 16, 17, 255, 256, 257, 515]


@pytest.mark.parametrize("group", [15, 16, 17, 255, 256, 257, 515])
def test_flush_boundaries(emu, group):
    """60-bit and 40-bit primes in one level; the ring is small because a thread's schedule does not depend on N"""
    import batch_reduce_cases as BR
    BR.case_flush(64, [60, 40, 40, 60], group)


def test_flush_boundaries_small_ring(emu):
    import batch_reduce_cases as BR
    BR.case_flush(8, [30, 30, 30], 257, out_items=2)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_sliced(emu, scheme):
    """a group of 23 items in 1, 2, 3, 4, 5 and 23 slices: most do not divide it"""
    import batch_reduce_cases as BR
    BR.case_sliced(scheme, 1024, [60, 40, 60], batch=46, group=23, slice_counts=(2, 3, 4, 5, 23))


@pytest.mark.parametrize("n,bits", SIZES[:2])
def test_plane_counts(emu, n, bits):
    """sizes 1, 4 and 5, in one launch and in two slices of a group of three"""
    import batch_reduce_cases as BR
    BR.case_plane_counts(n, bits)


def test_natural_slices(emu):
    """N = 1024, K = 2: 1024 output pairs per item, so one group of 16 is cut and 128 of them are not"""
    import batch_reduce_cases as BR
    BR.case_natural_slices("ckks", 1024, [60, 40, 60], group=16)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(emu, scheme):
    import batch_reduce_cases as BR
    BR.case_out_of_place(scheme, 1024, [60, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import batch_reduce_cases as BR
    BR.case_errors(scheme, 1024, [60, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(emu, scheme):
    import batch_reduce_cases as BR
    BR.case_transparent_check(scheme, 1024, [60, 40, 60])


def test_pending_state(emu):
    """N = 8192 is the smallest ring at which the library defers tails and products"""
    import batch_reduce_cases as BR
    BR.case_pending(8192, [50, 40, 40, 60], batch=2, group=2)


@needs_ref
def test_pipeline_ckks(emu):
    import batch_reduce_cases as BR
    BR.case_pipeline_ckks(1024, [60, 40, 40, 60], batch=5)


@needs_ref
def test_pipeline_bfv(emu):
    import batch_reduce_cases as BR
    BR.case_pipeline_bfv(1024, [60, 40, 60], batch=5)
