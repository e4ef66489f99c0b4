"""GPU: a 2-D convolution of scalar weights over a grid of ciphertexts (Evaluator_Conv2dScalarsItems; shl_conv2d_scalars) on the
gfx950 kernel, wide ([K] words per weight) and narrow (one signed 32-bit integer per weight): the N = 8 and N = 64 rings (weights
loaded per lane), N = 128 (the first ring where a wave stays at its output position and the weights are scalar loads), N = 8192
(both arithmetic classes in one level), K = 1 and the C5 chain at N = 65536 once.  Exact word equality and the metadata triple:
against DotPlainMapped over the map of the taps inside the image on the expanded plaintexts, MatMulScalarsItems where the shape
degenerates, the per-object forms and the REAL reference (oracle/_ref) where it is built, and against Python-integer arithmetic
around both flush intervals, across the cuts and for every built row tile and hint; the words next to the raw input and result
stay as they were."""
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ["ckks", "bgv", "bfv"]
C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])
RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (128, [60, 40, 60]), MID]
DEFERS = (8192, [50, 40, 40, 60])


def test_shape_list(gpu):
    import conv2d_scalars_cases as CV
    import matmul_scalars_cases as MS
    for narrow in (False, True):
        R = MS.row_tile(narrow)
        got = CV.shapes(R)
        assert len(got) == 7 and {s.out_channels for s in got} == set(MS.row_counts(R))
    assert CV.shape_of(CV.ASYMMETRIC, 1).out_size() == (3, 7)
    s = CV.shape_of(CV.REMAINDER, 1)
    assert s.out_size() == (3, 2) and (s.height + 2 * s.pad_h - s.kernel_h) % s.stride_h and (s.width + 2 * s.pad_w - s.kernel_w) % s.stride_w
    assert sorted({len(r) for r in CV.tap_rows(CV.shape_of(CV.SAME_3X3, 1))}) == [8, 12, 18], "corner, edge, interior"


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", RINGS)
def test_parity(gpu, scheme, n, bits):
    import conv2d_scalars_cases as CV
    CV.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import conv2d_scalars_cases as CV
    CV.case_parity(scheme, *MID, sizes=(2,), ci=0, per_object=False)


def test_parity_c5(gpu):
    """C = 2, a 3 x 3 image, a 2 x 2 kernel, OC = 3, against DotPlainMapped only"""
    import conv2d_scalars_cases as CV
    CV.case_parity("ckks", *C5, sizes=(2,), shape_list=[CV.Conv2dShape(2, 3, 3, 3, 2, 2, 1, 1, 0, 0)], per_object=False)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", [(8, [40, 40, 40]), (128, [60, 40, 60]), MID])
def test_narrow_equals_wide(gpu, scheme, n, bits):
    import conv2d_scalars_cases as CV
    CV.case_narrow_equals_wide(scheme, n, bits)


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_flush_boundaries(gpu, n, bits, narrow):
    import conv2d_scalars_cases as CV
    CV.case_flush(n, bits, narrow)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), MID])
def test_cuts(gpu, n, bits):
    import conv2d_scalars_cases as CV
    CV.case_cuts("ckks", n, bits)


def test_natural_slices(gpu):
    import conv2d_scalars_cases as CV
    CV.case_natural_slices("bgv", *MID)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 40, 60])])
def test_every_built_tile_and_hint(gpu, n, bits):
    """the per-lane and the wave-uniform path"""
    import conv2d_scalars_cases as CV
    CV.case_tiles(n, bits)


@pytest.mark.parametrize("n,bits", [(8, [30, 30, 30]), (128, [60, 40, 60]), MID])
def test_untouched_neighbours(gpu, n, bits):
    import conv2d_scalars_cases as CV
    CV.case_neighbours("bfv", n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(gpu, scheme):
    import conv2d_scalars_cases as CV
    CV.case_out_of_place(scheme, *DEFERS)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(gpu, scheme):
    import conv2d_scalars_cases as CV
    CV.case_transparent_check(scheme, *DEFERS)


def test_pending_state(gpu):
    import conv2d_scalars_cases as CV
    CV.case_pending(*DEFERS)


@pytest.mark.parametrize("narrow", [False, True])
def test_capture(gpu, narrow):
    """C = 2, a 2 x 2 image, a 3 x 3 kernel, pad 1 at one tile of channels: by the documented rule the recorded call is cut and uses
    pool scratch (asserted inside)"""
    import conv2d_scalars_cases as CV
    CV.case_capture(*MID, narrow)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import conv2d_scalars_cases as CV
    CV.case_errors(scheme, *DEFERS)
