"""GPU: the ciphertext x ciphertext reduction over the items of two batches (Evaluator_DotItems) on the gfx950 kernels: N = 8192
(a 60-bit and sub-2^50 primes in one level), the C5 chain at N = 65536 once, the N = 8 ring and K = 1.  Against multiply + add_many
on batches of one, against the REAL reference (oracle/_ref) where it is built, and against Python-integer arithmetic around the
flush interval of the lazy accumulators."""
import pytest

import sealref

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bgv"]
C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_parity(gpu, scheme):
    """g = 1 (equals multiply), 2 (two output items) and the whole batch"""
    import dot_items_cases as DI
    DI.case_parity(scheme, *MID, batch=4, groups=(1, 2, 4))


def test_group_not_a_power_of_two(gpu):
    """B = 15, g = 5: by the documented rule this launch is not cut, test_sliced and test_natural_slices cover the cut"""
    import dot_items_cases as DI
    DI.case_parity("ckks", *MID, batch=15, groups=(5,))


def test_lowest_level(gpu):
    """K = 1"""
    import dot_items_cases as DI
    DI.case_parity("ckks", *MID, batch=4, groups=(2, 4), ci=0)


def test_small_ring(gpu):
    """rows shorter than a wavefront"""
    import dot_items_cases as DI
    DI.case_parity("ckks", 8, [30, 30, 30], batch=4, groups=(1, 2, 4))


def test_parity_c5(gpu):
    import dot_items_cases as DI
    DI.case_parity("ckks", *C5, batch=3, groups=(3,))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_square(gpu, scheme):
    import dot_items_cases as DI
    DI.case_square(scheme, *MID)


@pytest.mark.parametrize("group", [127, 128, 129, 257])
def test_flush_boundaries(gpu, group):
    import dot_items_cases as DI
    assert group in (DI.DOT_ITEMS_FLUSH - 1, DI.DOT_ITEMS_FLUSH, DI.DOT_ITEMS_FLUSH + 1, 2 * DI.DOT_ITEMS_FLUSH + 1)
    DI.case_flush(*MID, group, patterns=("max", "alternating", "half") if group > 129 else ("max", "alternating", "half", "random"))


def test_flush_boundaries_small_ring(gpu):
    import dot_items_cases as DI
    DI.case_flush(8, [30, 30, 30], 257, out_items=2)


def test_sliced(gpu):
    """a group of 23 items in 1, 2, 3, 4, 5 and 23 slices: most do not divide it"""
    import dot_items_cases as DI
    DI.case_sliced("ckks", *MID, batch=46, group=23, slice_counts=(2, 3, 4, 5, 23))


def test_natural_slices(gpu):
    """N = 8192, K = 3: 12288 output pairs per item, so one group of 16 is cut and 11 of them are not (asserted inside)"""
    import dot_items_cases as DI
    DI.case_natural_slices("ckks", *MID, group=16)


def test_out_of_place_and_reuse(gpu):
    import dot_items_cases as DI
    DI.case_out_of_place_and_reuse("ckks", *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import dot_items_cases as DI
    DI.case_errors(scheme, *MID)


def test_errors_bfv_refused(gpu):
    import dot_items_cases as DI
    DI.case_bfv_refused(*MID)


def test_transparent_check(gpu):
    import dot_items_cases as DI
    DI.case_transparent_check("ckks", *MID)


def test_pending_state(gpu):
    """N = 8192 is the smallest ring at which the library defers tails and products"""
    import dot_items_cases as DI
    DI.case_pending(8192, [50, 40, 40, 60], batch=4, group=2)


def test_capture(gpu):
    """groups of 8 into two output items: by the documented rule the recorded call is cut and uses pool scratch"""
    import batch_reduce_cases as BR
    import dot_items_cases as DI
    assert BR.rule_slices(2 * 3 * 8192 // 2, 8) == 2
    DI.case_capture(*MID, batch=16, group=8)


@needs_ref
def test_pipeline_ckks(gpu):
    import dot_items_cases as DI
    DI.case_pipeline_ckks(*MID, batch=6, group=3)
