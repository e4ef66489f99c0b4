"""CPU: the ciphertext x ciphertext reduction over the items of two batches (Evaluator_DotItems) with the kernels emulated, small
rings.  Against multiply + add_many on batches of one everywhere, against the REAL reference (oracle/_ref) where it is built, and
against Python-integer arithmetic across the flush interval of the lazy accumulators."""
import pytest

SCHEMES = ["ckks", "bgv"]
SIZES = [(8, [30, 30, 30]), (1024, [60, 40, 60])]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", SIZES)
def test_parity(emu, scheme, n, bits):
    """g = 1 (equals multiply), 2 (two output items) and the whole batch"""
    import dot_items_cases as DI
    DI.case_parity(scheme, n, bits, batch=4, groups=(1, 2, 4))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_square(emu, scheme):
    import dot_items_cases as DI
    DI.case_square(scheme, 1024, [60, 40, 60])


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (64, [60, 40, 40, 60])])
def test_flush_boundaries(emu, n, bits):
    """one item past the interval; 60-bit and 40-bit primes in one level at N = 64 (a thread's schedule does not depend on N)"""
    import dot_items_cases as DI
    DI.case_flush(n, bits, 129)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_sliced(emu, scheme):
    """a group of 23 items in 1, 2, 3, 4, 5 and 23 slices: most do not divide it"""
    import dot_items_cases as DI
    DI.case_sliced(scheme, 1024, [60, 40, 60], batch=46, group=23, slice_counts=(2, 3, 4, 5, 23))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import dot_items_cases as DI
    DI.case_errors(scheme, 1024, [60, 40, 60])


def test_errors_bfv_refused(emu):
    import dot_items_cases as DI
    DI.case_bfv_refused(1024, [60, 40, 60])
