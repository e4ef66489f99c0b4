"""MI355X: pass 1 of the rounding tails in both orders (tail_order_cases.py) - every result word for word against the oracle and
the two orders against each other, at every two-pass size, with mixed and all-integer chains, and on either side of the batch
from which the library picks the source-resident order by itself."""
import os

import pytest

import tail_order_cases as T

GPU_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seal_amd", "lib", "libsealhip.so")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["ckks_k2_8192", "ckks_mixed_8192", "ckks_mixed_last60_8192", "ckks_mixed_32768", "ckks_mixed_65536",
                                  "ckks_int_8192", "ckks_int_65536", "bfv_8192", "bfv_32768"])
def test_both_orders_same_words(gpu, name):
    T.both_orders(GPU_LIB, name)


@pytest.mark.parametrize("name", ["ckks_mixed_8192", "ckks_mixed_65536", "ckks_int_8192", "bfv_8192"])
def test_both_orders_eager_key_switch_tail(gpu, name):
    T.both_orders(GPU_LIB, name, extra_env={"SEALHIP_KS_EAGER_TAIL": "1"})


def test_either_side_of_the_threshold(gpu):
    """N = 2^16: 16 tiles x 2 x batch items - batch 15 is below the 512 workgroups from which the source-resident order is taken,
    batch 16 on it; both batches with the order forced either way and left to the library (two distinct items tiled over the batch,
    every item compared)"""
    T.both_orders(GPU_LIB, "ckks_threshold_below_65536", check_items=2)
    T.both_orders(GPU_LIB, "ckks_threshold_at_65536", check_items=2)
