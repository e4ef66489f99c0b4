"""GPU: Galois sets (GaloisSet_Create / CreateFromSteps; Evaluator_ApplyGaloisSet) on the gfx950 kernels.  Each result item against
the per-object call on a batch of one holding the source item and, where oracle/_ref is built, against the REAL reference with the
same keys.  The small rings take the loop over the entries; N = 8192 the one-batch route on each of its sub-routes, chunked, K = 1;
the C5 chain at N = 65536 once; capture and replay."""
import pytest

import sealref

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
C5 = (65536, [60] + [50] * 14 + [60])
LOOP_RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (1024, [60, 40, 60])]
MID = (8192, [60, 40, 40, 60])
SMALL = (1024, [60, 40, 60])


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", LOOP_RINGS)
def test_parity_loop_route(gpu, scheme, n, bits):
    import galois_set_cases as GS
    GS.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("split", [None, 1, 3])
def test_parity_one_batch_route(gpu, scheme, split):
    import galois_set_cases as GS
    sub = None if split is None else "gathered" if (split == 1 and scheme == "ckks") else "permuted"
    GS.case_parity(scheme, *MID, env={} if split is None else {"SEALHIP_KS_SPLIT": split}, sub_route=sub)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(gpu, scheme):
    """K = 1"""
    import galois_set_cases as GS
    GS.case_parity(scheme, *MID, ci=0, batches=(3,), sets=("steps", "elts"), sub_route="permuted")


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_worst_case_keys(gpu, scheme):
    import galois_set_cases as GS
    side = GS.case_parity(scheme, *MID, batches=(3,), sets=("elts",), env={"SEALHIP_KS_SPLIT": 1}, key_pattern="mix4")
    GS.case_parity(scheme, *MID, batches=(3,), sets=("steps",), env={"SEALHIP_KS_SPLIT": 3}, side=side)


@pytest.mark.parametrize("lanes", [1, 3])
def test_chunks(gpu, lanes):
    import galois_set_cases as GS
    GS.case_chunks("ckks", *MID, lanes=lanes)


def test_chunks_bfv(gpu):
    import galois_set_cases as GS
    GS.case_chunks("bfv", *MID, lanes=1)


def test_launch_count(gpu):
    import galois_set_cases as GS
    GS.case_launch_count(*MID, small=SMALL)


def test_parity_c5(gpu):
    """B = 1, R = 3"""
    import galois_set_cases as GS
    GS.case_c5(*C5)


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_pending_tail(gpu, scheme):
    import galois_set_cases as GS
    GS.case_pending_tail(scheme, *MID)


def test_pending_operand(gpu):
    import galois_set_cases as GS
    GS.case_pending_operand(*MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_refusals(gpu, scheme):
    import galois_set_cases as GS
    GS.case_refusals(scheme, *MID)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_transparent_check(gpu, scheme):
    import galois_set_cases as GS
    GS.case_transparent_check(scheme, *MID)


def test_capture(gpu):
    import galois_set_cases as GS
    GS.case_capture(*MID)


def test_set_destroyed_after_the_call(gpu):
    import galois_set_cases as GS
    GS.case_destroy_after_call("ckks", *MID)


def test_keys_changed(gpu):
    import galois_set_cases as GS
    GS.case_keys_changed("ckks", *MID)


def test_create_errors(gpu):
    import galois_set_cases as GS
    GS.case_create_errors("ckks", *MID)


@needs_ref
def test_pipeline_diagonals(gpu):
    import galois_set_cases as GS
    GS.case_pipeline_diagonals(*MID)
