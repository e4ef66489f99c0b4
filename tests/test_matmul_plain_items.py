"""CPU: a matrix of plaintexts times a matrix of ciphertexts (Evaluator_MatMulPlainItems; shl_matmul_plain_items) with the kernels
emulated.  Exact word equality and the metadata triple: against DotPlainMapped over the dense map, against multiply_plain_device +
sum_items, against multiply_plain_inplace + add_many on batches of one and the REAL reference (oracle/_ref) where it is built, and
against Python-integer arithmetic around the flush interval, across the cuts and for every built tile.  (Capture and replay are in
the GPU suite only: the emulator does not replay graphs.)"""
import pytest


SCHEMES = ["ckks", "bgv", "bfv"]
# N = 8: the lanes of a wave in different rows of the grid; 64: a wave spans rows; 128: the first ring where a wave stays in its row;
# the last ring has both arithmetic classes (60- and 40-bit primes) in one level
MID = (1024, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])   # the smallest ring at which the library defers tails and products


def test_shapes_come_from_the_tile(emu):
    import matmul_plain_items_cases as MP
    TP, TC, flush = MP.info()
    assert (TP, TC) in MP.TILES and flush == 256
    assert MP.shapes() == [(1, 1), (TP - 1 or 1, TC + 1), (TP, TC), (TP + 1, TC - 1 or 1), (2 * TP + 1, 2 * TC + 1)]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(emu, scheme, n, bits):
    import matmul_plain_items_cases as MP
    MP.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1"""
    import matmul_plain_items_cases as MP
    MP.case_parity(scheme, *MID, sizes=(2,), ci=0)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_degenerate_forms(emu, scheme):
    import matmul_plain_items_cases as MP
    MP.case_degenerate(scheme, *MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(emu, n, bits):
    import matmul_plain_items_cases as MP
    MP.case_flush(n, bits)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(emu, n, bits):
    import matmul_plain_items_cases as MP
    MP.case_cuts("ckks", n, bits)


def test_natural_slices(emu):
    import matmul_plain_items_cases as MP
    MP.case_natural_slices("bgv", *MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60]), MID])
def test_every_built_tile(emu, n, bits):
    """(the largest ring with one plane and the random words only: its results are tens of megabytes per launch)"""
    import matmul_plain_items_cases as MP
    if (n, bits) == MID:
        MP.case_tiles(n, bits, size=1, patterns=("random",))
    else:
        MP.case_tiles(n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(emu, scheme):
    import matmul_plain_items_cases as MP
    MP.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(emu, scheme):
    import matmul_plain_items_cases as MP
    MP.case_transparent_check(scheme, *DEFERS)


def test_pending_state(emu):
    import matmul_plain_items_cases as MP
    MP.case_pending(*DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(emu, scheme):
    import matmul_plain_items_cases as MP
    MP.case_errors(scheme, *DEFERS)


def test_pipeline_bgv(emu):
    import matmul_plain_items_cases as MP
    MP.case_pipeline_bgv()


def test_pipeline_ckks(emu):
    import matmul_plain_items_cases as MP
    MP.case_pipeline_ckks(1024, [60, 40, 40, 60])
