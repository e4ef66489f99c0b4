"""GPU: a dense matrix of scalar plaintexts times a batch (CKKSEncoder_EncodeScalars / _EncodeIntegerScalars, Evaluator_LiftScalars,
Evaluator_DotScalarsDevice; shl_dot_scalars) on the gfx950 kernel: the N = 8 and N = 64 rings (per-lane weights), N = 128 (the
first ring with the weights in SGPRs), N = 8192 (both arithmetic classes in one level), K = 1 and the C5 chain at N = 65536 once.
Exact word equality: against DotPlainMapped over the dense map with expanded plaintexts, against the per-object forms on batches of
one, against the REAL reference (oracle/_ref) where it is built, and against Python-integer arithmetic around the flush interval
and across the cuts."""
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ["ckks", "bfv", "bgv"]
C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])


def test_row_counts_come_from_the_tile(gpu):
    import dot_scalars_cases as DS
    R, flush = DS.info()
    assert R in (2, 4, 8) and flush == 256
    assert DS.row_counts() == sorted({1, R - 1, R, R + 1, 2 * R + 1})


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(gpu, scheme, n, bits):
    import dot_scalars_cases as DS
    DS.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import dot_scalars_cases as DS
    DS.case_parity(scheme, *MID, sizes=(2,), ci=0)


def test_parity_c5(gpu):
    """rows = 3, B = 2"""
    import dot_scalars_cases as DS
    DS.case_parity("ckks", *C5, sizes=(2,), batch=2, rows_list=[3])


def test_encode_scalars(gpu):
    import dot_scalars_cases as DS
    DS.case_encode_scalars()


def test_encode_integer_scalars(gpu):
    import dot_scalars_cases as DS
    DS.case_encode_integer_scalars()


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
@pytest.mark.parametrize("bits,tbits,fast", [([40, 40, 60], 20, True), ([30, 30, 60], 40, False)])
def test_lift_scalars(gpu, scheme, bits, tbits, fast):
    import dot_scalars_cases as DS
    DS.case_lift_scalars(scheme, 1024, bits, tbits, fast)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(gpu, n, bits):
    import dot_scalars_cases as DS
    DS.case_flush(n, bits)


@pytest.mark.parametrize("row_tile", [2, 4, 8])
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries_every_tile(gpu, n, bits, row_tile):
    """every built row tile, per lane (N = 8) and per wave (N = 128): the accumulators carry the running residue across the flush"""
    import dot_scalars_cases as DS
    DS.case_flush(n, bits, batches=[DS.DOT_FLUSH - 1, DS.DOT_FLUSH, DS.DOT_FLUSH + 1, 2 * DS.DOT_FLUSH + 3], patterns=("max", "random"),
                  row_tile=row_tile)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(gpu, n, bits):
    import dot_scalars_cases as DS
    DS.case_cuts(n, bits)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60]), MID])
def test_every_built_tile(gpu, n, bits):
    """R = 2, 4 and 8 on the per-lane and on the wave-uniform path"""
    import dot_scalars_cases as DS
    DS.case_tiles(n, bits)


def test_natural_slices(gpu):
    import dot_scalars_cases as DS
    DS.case_natural_slices("ckks", *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(gpu, scheme):
    import dot_scalars_cases as DS
    DS.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(gpu, scheme):
    import dot_scalars_cases as DS
    DS.case_transparent_check(scheme, *DEFERS)


def test_pending_state(gpu):
    import dot_scalars_cases as DS
    DS.case_pending(*DEFERS)


def test_capture(gpu):
    """B = 16, R + 1 rows: by the documented rule the recorded call is cut and uses pool scratch (asserted inside)"""
    import dot_scalars_cases as DS
    DS.case_capture(*MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import dot_scalars_cases as DS
    DS.case_errors(scheme, *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_producer_errors(gpu, scheme):
    import dot_scalars_cases as DS
    DS.case_producer_errors(scheme, *MID)
