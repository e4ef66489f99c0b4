"""GPU: batched encryption in device memory (Encryptor_EncryptSymmetricDevice / Encryptor_EncryptDevice) on the gfx950 kernels:
N = 8192 and 32768, and the C5 chain at N = 65536 - batch 3 in full, batch 256 sampled (the first and last items, both sides of
every chunk edge and random ones).  Against the REAL reference (oracle/_ref) where it is built and against the per-object forms."""
import pytest

import sealref

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
C5 = (65536, [60] + [50] * 14 + [60])
SIZES = [(8192, [60, 40, 40, 60], 5), (32768, [60, 50, 50, 50, 60], 5), (C5[0], C5[1], 3)]


@needs_ref
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits,batch", SIZES)
def test_reference_parity(gpu, scheme, n, bits, batch):
    import encrypt_batch_cases as EB
    EB.case_reference_parity(scheme, n, bits, batch)


@needs_ref
def test_reference_parity_c5_batch256(gpu):
    """CKKS, batch 256: the public-key form runs in chunks of 32 items, the secret-key form in chunks of 34 (first level) / 36"""
    import encrypt_batch_cases as EB
    EB.case_reference_parity("ckks", *C5, batch=256, sample=True)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits,batch", SIZES)
def test_per_item_seeds(gpu, scheme, n, bits, batch):
    import encrypt_batch_cases as EB
    EB.case_per_item_seeds(scheme, n, bits, batch)


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_per_item_seeds_c5_batch256(gpu, scheme):
    import encrypt_batch_cases as EB
    EB.case_per_item_seeds(scheme, *C5, batch=256, sample=True, levels=[len(C5[1]) - 2])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_small_ring_fallbacks(gpu, scheme):
    import encrypt_batch_cases as EB
    EB.case_per_item_seeds(scheme, 8, [30, 30, 30], batch=3)


@needs_ref
@pytest.mark.parametrize("scheme", SCHEMES)
def test_small_ring_fallbacks_against_reference(gpu, scheme):
    import encrypt_batch_cases as EB
    EB.case_reference_parity(scheme, 8, [30, 30, 30], batch=3)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_fresh_entropy(gpu, scheme):
    import encrypt_batch_cases as EB
    EB.case_fresh_entropy(scheme, 8192, [60, 40, 40, 60], batch=5)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_host_sampling_equals_device(gpu, monkeypatch, scheme):
    import encrypt_batch_cases as EB
    EB.case_host_sampling_equals_device(scheme, 8192, [60, 40, 40, 60], 5, monkeypatch)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_errors(gpu, scheme):
    import encrypt_batch_cases as EB
    EB.case_errors(scheme, 8192, [60, 40, 40, 60])


@needs_ref
@pytest.mark.parametrize("n,bits,batch", [(8192, [60, 40, 40, 60], 5), (32768, [60, 50, 50, 50, 60], 17)])
def test_pipeline(gpu, n, bits, batch):
    import encrypt_batch_cases as EB
    EB.case_pipeline(n, bits, batch)
