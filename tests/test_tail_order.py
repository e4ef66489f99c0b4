"""CPU (fiber emulator): pass 1 of the rounding tails in both orders - index arithmetic, the hoisted half of the source mapping under
SEALHIP_CHECK_BOUNDS (the emulated library asserts the bounds p1_tile's lean fix() placement relies on), and the one place that
picks the order.  Every setting in a child process of its own (tail_order_cases.py); the device runs the same cases in
test_gpu_tail_order.py."""
import os

import pytest

import tail_order_cases as T

EMU_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu", "libsealhip_emu.so")


@pytest.mark.parametrize("name", ["ckks_k2_8192", "ckks_mixed_8192", "ckks_mixed_last60_8192", "ckks_int_8192", "bfv_8192"])
def test_both_orders_same_words(emu, name):
    T.both_orders(EMU_LIB, name, auto=False)


@pytest.mark.parametrize("name", ["ckks_mixed_8192", "ckks_int_8192", "bfv_8192"])
def test_both_orders_eager_key_switch_tail(emu, name):
    """SEALHIP_KS_EAGER_TAIL=1: the key switch completes its own mod-down (one mapped source, epilogue 2 / 3), the rescale is plain"""
    T.both_orders(EMU_LIB, name, extra_env={"SEALHIP_KS_EAGER_TAIL": "1"}, auto=False)


@pytest.mark.parametrize("name", ["ckks_mixed_32768", "ckks_mixed_65536", "ckks_int_65536", "bfv_32768"])
def test_both_orders_larger_sizes(emu, name):
    """N = 2^15 and 2^16 (at 2^16 the folded tail's double-precision pass uses the lean fix() placement)"""
    T.both_orders(EMU_LIB, name, auto=False)


def test_order_follows_the_grid(emu):
    """left to the library: source-resident from the threshold on (lowered to 8 workgroups here, a development switch) for class runs
    of more than one target, target-resident below it and for a run of one - and the same words on either side"""
    env = {"SEALHIP_TAIL_P1_MIN_WGS": "8", "SEALHIP_TAIL_P1_TRACE": "1"}
    below, err_below = T.run_in_child(EMU_LIB, "ckks_threshold_below_8192", env)
    at, err_at = T.run_in_child(EMU_LIB, "ckks_threshold_at_8192", env)
    assert "[tail] pass 1" in err_below and "source-resident" not in err_below, err_below[-1500:]
    # chain {60, 40, 50, 45 | 60}: after the division the targets are 60 (a run of one: target-resident) and 40, 50 (a run of two)
    assert "pass 1 source-resident (2 tiles x 4 items, 2 targets of class 1)" in err_at, err_at[-1500:]
    assert "pass 1 target-resident (2 tiles x 4 items, 1 targets of class 0)" in err_at, err_at[-1500:]
    forced, _ = T.run_in_child(EMU_LIB, "ckks_threshold_at_8192", {"SEALHIP_TAIL_P1_ORDER": "0"})
    assert at == forced
