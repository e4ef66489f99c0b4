"""CPU: item maps (ItemMap_Create; Evaluator_SumItemsMapped / DotPlainMapped / DotItemsMapped; shl_reduce_mapped) with the kernels
emulated.  Against the REAL reference (oracle/_ref) where it is built, against the per-object forms on batches of one holding the
named items everywhere, and against Python-integer arithmetic around the flush intervals and across the cuts.  (Capture and replay
are in the GPU suite only: the emulator does not replay graphs.)"""
import pytest

import sealref

needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
# N = 8: every lane of a wave in another row; 64: a wave spans two rows; 128: the first ring on the wave-uniform path
SIZES = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), (1024, [60, 40, 60])]
SMALL = (1024, [60, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", SIZES)
def test_parity(emu, scheme, n, bits):
    import item_map_cases as IM
    IM.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1"""
    import item_map_cases as IM
    IM.case_parity(scheme, *SMALL, sizes=(2,), ci=0)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [SIZES[0], SIZES[2]])
def test_gather(emu, scheme, n, bits):
    import item_map_cases as IM
    IM.case_gather(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_identity_map_is_the_contiguous_form(emu, scheme):
    import item_map_cases as IM
    IM.case_identity(scheme, *SMALL)


def test_flush_lengths_come_from_the_intervals():
    import item_map_cases as IM
    assert IM.FLUSH_LENGTHS == [1, 15, 16, 17, 255, 256, 257, 515] and IM.DOT_ITEMS_LENGTHS == [127, 128, 129]


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 40, 60])])
def test_ragged_flush_boundaries(emu, n, bits):
    """per lane (N = 8: all rows in one wave; N = 64) and per wave (N = 128); 60-bit and 40-bit primes in one level"""
    import item_map_cases as IM
    IM.case_flush(n, bits)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), SMALL])
def test_ragged_cuts(emu, n, bits):
    import item_map_cases as IM
    IM.case_cuts(n, bits)


def test_natural_slices(emu):
    """N = 1024, K = 2: 4096 output pairs for four rows - the map of mean row 10 is cut, the one of mean row 5 is not"""
    import item_map_cases as IM
    IM.case_natural_slices(*SMALL)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(emu, scheme):
    import item_map_cases as IM
    IM.case_out_of_place(scheme, *SMALL)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(emu, scheme):
    import item_map_cases as IM
    IM.case_transparent_check(scheme, *SMALL)


def test_pending_state(emu):
    """N = 8192 is the smallest ring at which the library defers tails and products"""
    import item_map_cases as IM
    IM.case_pending(8192, [50, 40, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_map_destroyed_after_the_call(emu, scheme):
    import item_map_cases as IM
    IM.case_destroy_after_call(scheme, *SMALL)


def test_create_errors(emu):
    import item_map_cases as IM
    IM.case_create_errors("ckks", *SMALL)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import item_map_cases as IM
    IM.case_errors(scheme, *SMALL)


@needs_ref
def test_pipeline_sparse_matrix(emu):
    import item_map_cases as IM
    IM.case_pipeline_sparse_matrix(1024, [60, 40, 40, 60])


@needs_ref
def test_pipeline_pairs(emu):
    import item_map_cases as IM
    IM.case_pipeline_pairs(1024, [60, 40, 40, 60])
