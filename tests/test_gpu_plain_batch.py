"""GPU: one plaintext per item of a device-resident batch (Evaluator_AddPlainDevice / SubPlainDevice / MultiplyPlainDevice /
TransformPlainToNTTDevice) on the gfx950 kernels: N = 8192 (both arithmetic classes in one level) and 32768, the C5 chain at
N = 65536 for CKKS - the smallest shapes that reach every engine plan of the transforms the BFV / BGV paths call.  Against the REAL
reference (oracle/_ref) where it is built and against the per-object forms on batches of one."""
import pytest

import sealref

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
C5 = (65536, [60] + [50] * 14 + [60])
SIZES = [(8192, [60, 40, 40, 60], 5), (32768, [60, 50, 50, 50, 60], 5)]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits,batch", SIZES)
def test_parity(gpu, scheme, n, bits, batch):
    import plain_batch_cases as PB
    PB.case_parity(scheme, n, bits, batch)


def test_parity_c5(gpu):
    import plain_batch_cases as PB
    PB.case_parity("ckks", *C5, batch=3)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import plain_batch_cases as PB
    PB.case_parity(scheme, 8192, [60, 40, 40, 60], batch=5, sizes=(2,), ci=0)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_small_ring(gpu, scheme):
    import plain_batch_cases as PB
    PB.case_parity(scheme, 8, [30, 30, 30], batch=3)


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_branches_fast_lift(gpu, scheme):
    """t (20 bits) below every prime of the level: the monomial items' words differ from the generic path's"""
    import plain_batch_cases as PB
    assert PB.case_branches(scheme, 8192, [60, 40, 40, 60])


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_branches_general_lift(gpu, scheme):
    """t (40 bits) above the 30-bit primes of the level: the increment per prime.  The context builder accepts these parameters at
    N = 8192 (t only has to stay below the level's whole modulus, 90 bits here)."""
    import plain_batch_cases as PB
    assert not PB.case_branches(scheme, 8192, [30, 30, 30, 60], tbits=40)


@needs_ref
@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
@pytest.mark.parametrize("bits,tbits,fast", [([40, 40, 60], 20, True), ([30, 30, 60], 40, False)])
def test_shared_plaintext(gpu, scheme, bits, tbits, fast):
    """one Plaintext of 1, 5, N - 1 and N coefficients for a batch of 3 at N = 64, two primes, against the reference item by item;
    t below every prime (fast plain lift) and above them (general lift)"""
    import plain_batch_cases as PB
    assert PB.case_shared_plaintext(scheme, 64, bits, tbits) == fast


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_transform(gpu, scheme):
    import plain_batch_cases as PB
    PB.case_transform(scheme, 8192, [60, 40, 40, 60], batch=5)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_out_of_place(gpu, scheme):
    import plain_batch_cases as PB
    PB.case_out_of_place(scheme, 8192, [60, 40, 40, 60])


def test_natural_chunks(gpu):
    """BGV on the C5 chain: an item's lifted plaintext is 15 x 65536 words, so the 256 MiB rule makes chunks of 34 items and a
    batch of 40 runs as 34 + 6 (asserted from the rule inside the case)"""
    import plain_batch_cases as PB
    PB.case_natural_chunks("bgv", *C5, batch=40)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import plain_batch_cases as PB
    PB.case_errors(scheme, 8192, [60, 40, 40, 60])


@needs_ref
@pytest.mark.parametrize("n,bits,batch", [(8192, [60, 40, 40, 60], 5)])
def test_pipeline_ckks(gpu, n, bits, batch):
    import plain_batch_cases as PB
    PB.case_pipeline_ckks(n, bits, batch)


@needs_ref
def test_pipeline_bfv(gpu):
    import plain_batch_cases as PB
    PB.case_pipeline_bfv(8192, [60, 40, 40, 60], batch=5)


def test_capture(gpu):
    import plain_batch_cases as PB
    PB.case_capture(8192, [60, 40, 40, 60], batch=5)
