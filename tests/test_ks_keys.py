"""CPU (fiber emulator, built with SEALHIP_CHECK_BOUNDS and SEALHIP_AB_SWITCHES): the key switch with structured keys at every
digit-group count and on every route (ks_keys_cases.py) - index arithmetic, the asserted bounds of the lazy accumulators, and the
group count the library traces for every forced SEALHIP_KS_SPLIT.  One child process at a time; a bound violation aborts the
child, which fails the test with the child's stderr.  The device runs the same cases in test_gpu_ks_keys.py."""
import os
import subprocess

import pytest

import ks_keys_cases as KC
from oracle import coeff_modulus_create, kind_available
from parity_cases import KEY_PATTERNS

EMU_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu", "libsealhip_emu.so")
BOTH = ["mix4", "half1"]

ALL = tuple(KEY_PATTERNS)
# (case, key patterns of one child).  The device runs every pattern of every case in seconds; here the cases that the emulator needs
# minutes for are cut to half1 and mix4 - the edge of the balanced doubles and of the quotient estimate, and the mix of all edge
# values: lean_65536 (test_lean_65536: relinearize and rotation in a child each) and sched_8192 (K = 17, one child per pattern).
SPLIT_RUNS = [
    ("mac_4096", ALL), ("fused_8192", ALL), ("bfv_8192", ALL), ("bgv_8192", ALL),
    ("fused_16384", ALL[:4]), ("fused_16384", ALL[4:]),
    ("sched_8192", ("half1",)), ("sched_8192", ("mix4",)),
]


def _child(name, mode, patterns, env=None):
    if KC.CASES[name][0] == "bgv" and kind_available() != "reference":
        pytest.skip("BGV parity needs the real reference (oracle/_ref)")
    e = {"SEALHIP_KS_TRACE": "1"}
    e.update(env or {})
    try:
        return KC.run_in_child(EMU_LIB, name, mode, patterns, env=e, timeout=3000)
    except KC.ChildDied as ex:
        pytest.fail(str(ex))


def _check_trace(name, stderr, patterns, both_ops=True):
    """every fused key switch after a note `pattern P split S` ran in the number of groups that S asks for"""
    K = len(KC.CASES[name][2]) - 1
    fused = KC.CASES[name][1] >= 8192
    seen = set()
    for note, counts in KC.traced_splits(stderr):
        words = note.split()
        if len(words) < 4 or words[2] != "split":
            continue
        if not fused:
            assert counts == [], "%s: the unfused path has no digit groups: %r" % (name, (note, counts))
            continue
        want = KC.auto_split(name) if words[3] == "auto" else min(int(words[3]), K)
        # relinearize and the rotation (a zero key has no rotation), each with the division that follows and, at the launcher's own
        # count, once more on its own
        ops = 2 if both_ops and words[1] != "zero" else 1
        assert counts == [want] * (2 * ops if words[3] == "auto" else ops), "%s: after %r the library ran %r groups, expected %d" % (name, note, counts, want)
        seen.add(words[3] + (" clamp" if len(words) > 4 else ""))
    if fused:
        asked = {"auto"} | {str(s) for s in KC.SPLITS if s is not None and s <= K}
        if K < 8 and "mix4" in patterns:
            asked |= {"%d clamp" % [s for s in KC.SPLITS if s is not None and s > K][0], "%d clamp" % K}
        assert seen == asked, "%s: group counts traced %r, asked %r" % (name, sorted(seen), sorted(asked))


@pytest.mark.parametrize("name,patterns", SPLIT_RUNS, ids=["%s-%s" % (n, "all" if p == ALL else "+".join(p)) for n, p in SPLIT_RUNS])
def test_structured_keys_every_group_count(emu, name, patterns):
    """every key pattern x three items x SEALHIP_KS_SPLIT unset, 1, 2, 3, 5, 8 (a count above K once: the K-group run's words),
    relinearize and rotation each followed by the division; fused_8192 and sched_8192 also: two transparent results refused"""
    res, err = _child(name, "splits", list(patterns))
    assert res["cells"] > 0
    _check_trace(name, err, patterns)


@pytest.mark.parametrize("pattern", BOTH)
@pytest.mark.parametrize("op", ["relin", "rot"])
def test_lean_65536(emu, op, pattern):
    """N = 2^16, a 60-bit digit into 49- and 50-bit targets (lean fix placement, kLeanEntry): every group count, K = 5"""
    res, err = _child("lean_65536", "splits:" + op, [pattern])
    assert res["cells"] > 0
    _check_trace("lean_65536", err, [pattern], both_ops=False)


@pytest.mark.parametrize("name", ["fused_8192", "bfv_8192", "bgv_8192"])
def test_structured_keys_eager_tail(emu, name):
    res, err = _child(name, "splits", BOTH, env={"SEALHIP_KS_EAGER_TAIL": "1"})
    assert res["cells"] > 0
    _check_trace(name, err, BOTH)


@pytest.mark.parametrize("name", ["fused_8192", "bfv_8192", "bgv_8192"])
def test_structured_keys_chunked(emu, name):
    """batch 5, SEALHIP_KS_CHUNK=2, SEALHIP_KS_LANES=2"""
    res, err = _child(name, "chunked", BOTH)
    assert res["cells"] > 0 and "in chunks of 2 on 2 lane(s)" in err, err[-1500:]


def test_structured_keys_deferred_product(emu):
    """multiply(x, y, w) + relinearize_inplace(w) (CKKS is the one scheme whose products are deferred)"""
    res, _ = _child("fused_8192", "lazy", BOTH)
    assert res["cells"] > 0


@pytest.mark.parametrize("name,parts", [("fused_8192", "2+3+8"), ("bfv_8192", "2+8"), ("bgv_8192", "2+8")])
def test_structured_keys_digit_parallel(emu, name, parts):
    """K = 4 over 2, 3 and 8 virtual ranks (ragged ranges, ranks without digits, eight partial sums); BFV, BGV: K = 3 over 2 and 8"""
    res, _ = _child(name, "dp" + parts, BOTH)
    assert res["cells"] == 2 * len(parts.split("+"))


def test_key_register_order_word_by_word(emu):
    """key_layout_kernel's stored words themselves (tests/key_layout_check.cpp, a stand-alone program on the emulated library): the
    balanced doubles of the primes below 2^50 and the (word, floor(word 2^64 / q)) pairs of the 51 to 60-bit ones against 128-bit
    integers, for every key pattern and uniform words, and key_unlayout_kernel's way back.  The key switch's results cannot show a
    quotient that is too small (the lazy product absorbs it, only the accumulators' headroom goes); this does."""
    here = os.path.dirname(os.path.abspath(__file__))
    emudir = os.path.join(here, "hipemu")
    exe = os.path.join(emudir, "obj", "key_layout_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-DSEALHIP_CHECK_BOUNDS", "-DSEALHIP_AB_SWITCHES",
                           "-I" + os.path.join(emudir, "include"), "-I" + os.path.join(os.path.dirname(here), "seal_amd", "csrc"),
                           os.path.join(here, "key_layout_check.cpp"), "-o", exe, "-L" + emudir, "-lsealhip_emu", "-Wl,-rpath," + emudir])
    n = 8192
    primes = coeff_modulus_create(n, [50, 59, 57, 51, 60])
    out = subprocess.run([exe, str(n)] + [str(int(q)) for q in primes], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "key_layout_check ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
