"""GPU: a matrix of plaintexts times a matrix of ciphertexts (Evaluator_MatMulPlainItems; shl_matmul_plain_items) on the gfx950
kernel: the N = 8 and N = 64 rings, N = 128 (the first ring where a wave stays in its row), N = 8192 (both arithmetic classes in one
level), K = 1 and the C5 chain at N = 65536 once.  Exact word equality and the metadata triple: against DotPlainMapped over the
dense map, against multiply_plain_device + sum_items, against multiply_plain_inplace + add_many on batches of one and the REAL
reference (oracle/_ref) where it is built, and against Python-integer arithmetic around the flush interval, across the cuts and for
every built tile."""
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ["ckks", "bgv", "bfv"]
C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])


def test_shapes_come_from_the_tile(gpu):
    import matmul_plain_items_cases as MP
    TP, TC, flush = MP.info()
    assert (TP, TC) in MP.TILES and flush == 256
    assert MP.shapes() == [(1, 1), (TP - 1 or 1, TC + 1), (TP, TC), (TP + 1, TC - 1 or 1), (2 * TP + 1, 2 * TC + 1)]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(gpu, scheme, n, bits):
    import matmul_plain_items_cases as MP
    MP.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import matmul_plain_items_cases as MP
    MP.case_parity(scheme, *MID, sizes=(2,), ci=0)


def test_parity_c5(gpu):
    """rows 2, inner 2, cols 3 against the mapped route only"""
    import matmul_plain_items_cases as MP
    MP.case_parity("ckks", *C5, sizes=(2,), inner=2, shape_list=[(2, 3)], per_object=False)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_degenerate_forms(gpu, scheme):
    import matmul_plain_items_cases as MP
    MP.case_degenerate(scheme, *MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(gpu, n, bits):
    import matmul_plain_items_cases as MP
    MP.case_flush(n, bits)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(gpu, n, bits):
    import matmul_plain_items_cases as MP
    MP.case_cuts("ckks", n, bits)


def test_natural_slices(gpu):
    import matmul_plain_items_cases as MP
    MP.case_natural_slices("bgv", *MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60]), MID])
def test_every_built_tile(gpu, n, bits):
    """(the largest ring with one plane and the random words only: its results are tens of megabytes per launch)"""
    import matmul_plain_items_cases as MP
    if (n, bits) == MID:
        MP.case_tiles(n, bits, size=1, patterns=("random",))
    else:
        MP.case_tiles(n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(gpu, scheme):
    import matmul_plain_items_cases as MP
    MP.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(gpu, scheme):
    import matmul_plain_items_cases as MP
    MP.case_transparent_check(scheme, *DEFERS)


def test_pending_state(gpu):
    import matmul_plain_items_cases as MP
    MP.case_pending(*DEFERS)


def test_capture(gpu):
    """inner = 16 at TP x (TC + 1): by the documented rule the recorded call is cut and uses pool scratch (asserted inside)"""
    import matmul_plain_items_cases as MP
    MP.case_capture(*MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import matmul_plain_items_cases as MP
    MP.case_errors(scheme, *DEFERS)


def test_pipeline_bgv(gpu):
    import matmul_plain_items_cases as MP
    MP.case_pipeline_bgv()


def test_pipeline_ckks(gpu):
    import matmul_plain_items_cases as MP
    MP.case_pipeline_ckks(8192, [60, 40, 40, 60])
