"""GPU: a sparse matrix of scalar weights times a batch over an item map (Evaluator_DotScalarsMapped; shl_dot_scalars_mapped) on
the gfx950 kernel, wide ([K] words per weight) and narrow (one signed 32-bit integer per weight): the N = 8 and N = 64 rings (lists
and weights loaded per lane, the lanes of a wave in rows of different length), N = 128 (the first ring where a wave stays in its row
and lists and weights are scalar loads), N = 8192 (both arithmetic classes in one level), K = 1 and the C5 chain at N = 65536 once.
Exact word equality and the metadata triple: against DotPlainMapped with the same map on the expanded plaintexts, DotScalarsDevice
over the dense map, Conv2dScalarsItems over the map of the in-image taps, the per-object forms and the REAL reference (oracle/_ref)
where it is built, and against Python-integer arithmetic for the shapes only this call has, around both flush intervals and across
the cuts; the words next to the raw input, weights and result stay as they were."""
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ["ckks", "bgv", "bfv"]
C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(gpu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_parity(scheme, n, bits, per_object=(n, bits) == MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import dot_scalars_mapped_cases as DM
    DM.case_parity(scheme, *MID, sizes=(2,), ci=0, per_object=False)


def test_parity_c5(gpu):
    """a source of 4 items and 3 short rows, against DotPlainMapped only"""
    import dot_scalars_mapped_cases as DM
    DM.case_parity("ckks", *C5, sizes=(2,), source=4, rows=[[2], [0, 3, 3], [1, 0]], second=[[1], [0, 2, 2], [2, 0]], per_object=False)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_dense_map_is_dot_scalars_device(gpu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_dense(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_tap_map_is_conv2d(gpu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_conv(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 60]), MID])
def test_depthwise_dilated_pooling(gpu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_only_here(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [40, 40, 40]), (128, [60, 40, 60]), MID])
def test_narrow_equals_wide(gpu, scheme, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_narrow_equals_wide(scheme, n, bits)


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(gpu, n, bits, narrow):
    import dot_scalars_mapped_cases as DM
    DM.case_flush(n, bits, narrow)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(gpu, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_cuts(n, bits)


def test_natural_slices(gpu):
    import dot_scalars_mapped_cases as DM
    DM.case_natural_slices(*MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 60]), MID])
def test_untouched_neighbours(gpu, n, bits):
    import dot_scalars_mapped_cases as DM
    DM.case_neighbours("bfv", n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(gpu, scheme):
    import dot_scalars_mapped_cases as DM
    DM.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(gpu, scheme):
    import dot_scalars_mapped_cases as DM
    DM.case_transparent_check(scheme, *DEFERS)


def test_pending_state(gpu):
    import dot_scalars_mapped_cases as DM
    DM.case_pending(*DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_destroy_after_call(gpu, scheme):
    import dot_scalars_mapped_cases as DM
    DM.case_destroy_after_call(scheme, *MID)


def test_capture(gpu):
    """two maps, wide and narrow: by the documented rule the calls over the long rows are cut and use pool scratch (asserted inside)"""
    import dot_scalars_mapped_cases as DM
    DM.case_capture(*MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import dot_scalars_mapped_cases as DM
    DM.case_errors(scheme, *DEFERS)
