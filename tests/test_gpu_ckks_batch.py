"""GPU: batched CKKS encoding in device memory (CKKSEncoder_EncodeDevice / _DecodeDevice) on the gfx950 kernels, against the
REAL reference (oracle/_ref): 8192 (two passes, one column stage), 32768 (three), the C5 chain at N = 65536 (four; full parity
at batch 3, sampled items incl. the chunk edges at batch 256) and N = 131072 (five)."""
import pytest

import sealref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")]

C5 = (65536, [60] + [50] * 14 + [60])


@pytest.mark.parametrize("n,bits,batch", [(8192, [60, 40, 40, 60], 5), (32768, [60, 50, 50, 50, 60], 17)])
def test_encode_decode_parity(gpu, n, bits, batch):
    import ckks_batch_cases as CB
    CB.case_encode_decode_parity(n, bits, batch)


def test_encode_decode_parity_c5(gpu):
    """every level of the C5 chain; one batch holds 64-bit, 128-bit and multi-precision coefficients"""
    import ckks_batch_cases as CB
    widths = CB.case_encode_decode_parity(*C5, batch=3)
    assert {64, 128, 0} <= widths, widths


def test_encode_decode_parity_c5_batch256(gpu):
    """batch 256 at the first level: the first and last items, both sides of every chunk edge and random ones"""
    import ckks_batch_cases as CB
    n, bits = C5
    CB.case_encode_decode_parity(n, bits, 256, sample=True, counts=(n // 2, 5), levels=(len(bits) - 2,), scales=(2.0 ** 30, 2.0 ** 150))


def test_encode_decode_parity_n131072(gpu):
    import ckks_batch_cases as CB
    CB.case_encode_decode_parity(131072, [60, 50, 50, 60], batch=2, counts=(65536, 5))


@pytest.mark.parametrize("n,bits,batch", [(8192, [60, 40, 40, 60], 5), (C5[0], C5[1], 3)])
def test_decode_random_words(gpu, n, bits, batch):
    import ckks_batch_cases as CB
    CB.case_decode_random_words(n, bits, batch)


@pytest.mark.parametrize("n,bits", [(8192, [60, 40, 40, 60]), C5])
def test_errors(gpu, n, bits):
    import ckks_batch_cases as CB
    CB.case_errors(n, bits)


@pytest.mark.parametrize("n,bits,batch", [(8192, [60, 40, 40, 60], 5), (32768, [60, 50, 50, 50, 60], 17)])
def test_client_loop(gpu, n, bits, batch):
    import ckks_batch_cases as CB
    CB.case_client_loop(n, bits, batch)


def test_round_trip(gpu):
    import ckks_batch_cases as CB
    CB.case_round_trip(*C5, batch=16)


@pytest.mark.parametrize("n,bits", [(8192, [60, 40, 40, 60]), C5, (131072, [60, 50, 50, 60])])
def test_batch_of_one(gpu, n, bits):
    import ckks_batch_cases as CB
    CB.case_batch_of_one(n, bits)
