"""MI355X: the key switch with structured keys at every digit-group count and on every route (ks_keys_cases.py), word for word
against the oracle.  One child process at a time, each with its own time limit; after a child that was killed (signal, abort,
time limit) or that reported a device fault no further child is started: the remaining parametrisations fail at once without touching the device.  The
product library has no trace: that SEALHIP_KS_SPLIT gives the group count it asks for is asserted on the emulator
(test_ks_keys.py) and trusted here."""
import os

import pytest

import ks_keys_cases as KC
from oracle import kind_available
from parity_cases import KEY_PATTERNS

GPU_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seal_amd", "lib", "libsealhip.so")
pytestmark = pytest.mark.gpu
BOTH = ["mix4", "half1"]
_dead = []  # why no further child may start


def _child(name, mode, patterns, env=None, timeout=180):
    if KC.CASES[name][0] == "bgv" and kind_available() != "reference":
        pytest.skip("BGV parity needs the real reference (oracle/_ref)")
    if _dead:
        pytest.fail("not started: an earlier child of this module died on the device\n" + _dead[0])
    try:
        res, _ = KC.run_in_child(GPU_LIB, name, mode, patterns, env=env, timeout=timeout)
    except KC.ChildDied as ex:
        _dead.append(str(ex))
        pytest.fail(str(ex))
    assert res["cells"] > 0
    return res


@pytest.mark.parametrize("name", list(KC.CASES))
def test_structured_keys_every_group_count(gpu, name):
    """every key pattern x three items x SEALHIP_KS_SPLIT unset, 1, 2, 3, 5, 8 (a count above K once: the K-group run's words),
    relinearize and rotation each followed by the division; fused_8192 and sched_8192 also: two transparent results refused"""
    _child(name, "splits", list(KEY_PATTERNS))


@pytest.mark.parametrize("name", ["fused_8192", "bfv_8192", "bgv_8192"])
def test_structured_keys_eager_tail(gpu, name):
    _child(name, "splits", BOTH, env={"SEALHIP_KS_EAGER_TAIL": "1"})


@pytest.mark.parametrize("name", ["fused_8192", "bfv_8192", "bgv_8192"])
def test_structured_keys_chunked(gpu, name):
    """batch 5, SEALHIP_KS_CHUNK=2, SEALHIP_KS_LANES=2"""
    _child(name, "chunked", BOTH)


def test_structured_keys_deferred_product(gpu):
    """multiply(x, y, w) + relinearize_inplace(w) (CKKS is the one scheme whose products are deferred)"""
    _child("fused_8192", "lazy", BOTH)


@pytest.mark.parametrize("name,parts", [("fused_8192", "2+3+8"), ("sched_65536", "8"), ("bfv_8192", "2+8"), ("bgv_8192", "2+8")])
def test_structured_keys_digit_parallel(gpu, name, parts):
    """K = 4 over 2, 3 and 8 virtual ranks (ragged ranges, ranks without digits, eight partial sums), K = 9 over 8; BFV, BGV: K = 3
    over 2 and 8"""
    res = _child(name, "dp" + parts, BOTH)
    assert res["cells"] == 2 * len(parts.split("+"))
