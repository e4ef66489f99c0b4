"""CPU: Galois sets (GaloisSet_Create / CreateFromSteps; Evaluator_ApplyGaloisSet) with the kernels emulated.  Each result item against
the per-object call on a batch of one holding the source item and, where oracle/_ref is built, against the REAL reference with the
same keys.  The small rings take the loop over the entries, N = 8192 the one-batch route on each of its sub-routes.  (Capture and
replay, and the C5 chain, are in the GPU suite only.)"""
import ctypes as C
import os
import re

import pytest

import sealref

needs_ref = pytest.mark.skipif(not sealref.available(), reason="oracle/_ref (the real reference) is not built")

SCHEMES = ["ckks", "bfv", "bgv"]
LOOP_RINGS = [(8, [30, 30, 30]), (64, [60, 40, 40, 60]), (1024, [60, 40, 60])]
MID = (8192, [60, 40, 40, 60])   # K = 3: an integer-class and a double-precision prime in one level
SMALL = (1024, [60, 40, 60])


# ---- the extension header include/sealhip_galois_set.h: what test_cabi.py / test_capi_objects.py / test_host_paths.py hold for
#      include/sealhip.h, for the exports that are declared here.  One word per argument; the ones in capitals are the checked handles
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_LIB = os.path.join(ROOT, "seal_amd", "lib", "libsealhip.so")
EXPORTS = {
    "GaloisSet_Create": "CTX GLK u64 elts OUTH", "GaloisSet_CreateFromSteps": "CTX GLK u64 steps OUTH", "GaloisSet_Destroy": "SET",
    "GaloisSet_Info": "SET out out out outbool", "Evaluator_ApplyGaloisSet": "EV CT SET DST", "SealHip_GaloisSetStats": "out out out",
}


def declared_in_extension_header():
    text = open(os.path.join(ROOT, "include", "sealhip_galois_set.h")).read()
    return sorted(set(re.findall(r"SHL_FUNC\s+(\w+)\s*\(", text)))


def test_extension_header_is_bound_and_in_the_table():
    from seal_amd import _native
    assert declared_in_extension_header() == sorted(_native.EXT_SYMBOLS) == sorted(EXPORTS)
    assert not set(_native.EXT_SYMBOLS) & set(_native.SYMBOLS)
    main = open(os.path.join(ROOT, "include", "sealhip.h")).read()
    assert '#include "sealhip_galois_set.h"' in main, "include/sealhip.h brings the extension in"


def test_library_exports_the_extension_header():
    if not os.path.exists(GPU_LIB):
        import subprocess
        subprocess.check_call(["make", "-s", "-j8", "gpu"], cwd=os.path.join(ROOT, "seal_amd", "csrc"))
    lib = C.CDLL(GPU_LIB)
    assert not [s for s in declared_in_extension_header() if not hasattr(lib, s)]


@pytest.mark.parametrize("symbol", sorted(EXPORTS))
def test_null_handle_is_e_pointer(emu, symbol):
    import galois_set_cases as GS
    S = emu
    side = GS.make_side("ckks", *SMALL)
    gs = side.make_set(GS.entries_of(side, "elts"))
    x = side.dev_ct(side.operand(side.first, 1), side.first)
    dest = S.Ciphertext(side.ctx, batch=5)
    out, flag = (C.c_uint64 * 1)(), C.c_bool()
    values = {"CTX": side.ctx._h, "GLK": side.glk._h, "SET": gs._h, "EV": side.ev._h, "CT": x._h, "DST": dest._h,
              "OUTH": C.pointer(C.c_void_p()), "u64": C.c_uint64(1), "elts": (C.c_uint32 * 1)(side.elt(1)), "steps": (C.c_int * 1)(1),
              "out": out, "outbool": C.byref(flag)}
    kinds = EXPORTS[symbol].split()
    fn = getattr(S._native.lib(), symbol)
    for i in [i for i, k in enumerate(kinds) if k.isupper()]:
        args = [None if j == i else values[k] for j, k in enumerate(kinds)]
        assert fn(*args) & 0xFFFFFFFF == S._native.E_POINTER, (symbol, "argument %d (%s)" % (i, kinds[i]))


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n,bits", LOOP_RINGS)
def test_parity_loop_route(emu, scheme, n, bits):
    import galois_set_cases as GS
    GS.case_parity(scheme, n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("split", [None, 1, 3])
def test_parity_one_batch_route(emu, scheme, split):
    """SEALHIP_KS_SPLIT unset (the rule's own choice), 1 (un-split: CKKS reads the operand through the entries' maps) and 3 (digit
    groups: permuted scratch)"""
    import galois_set_cases as GS
    sub = None if split is None else "gathered" if (split == 1 and scheme == "ckks") else "permuted"
    GS.case_parity(scheme, *MID, env={} if split is None else {"SEALHIP_KS_SPLIT": split}, sub_route=sub)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lowest_level(emu, scheme):
    """K = 1 at 8192: nothing defers, nothing folds"""
    import galois_set_cases as GS
    GS.case_parity(scheme, *MID, ci=0, batches=(3,), sets=("steps", "elts"), sub_route="permuted")


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_worst_case_keys(emu, scheme):
    """key words at 0, q - 1, q/2 and q/2 + 1 (parity_cases.extreme_key), both sub-routes"""
    import galois_set_cases as GS
    side = GS.case_parity(scheme, *MID, batches=(3,), sets=("elts",), env={"SEALHIP_KS_SPLIT": 1}, key_pattern="mix4")
    GS.case_parity(scheme, *MID, batches=(3,), sets=("steps",), env={"SEALHIP_KS_SPLIT": 3}, side=side)


@pytest.mark.parametrize("lanes", [1, 3])
def test_chunks(emu, lanes):
    import galois_set_cases as GS
    GS.case_chunks("ckks", *MID, lanes=lanes)


def test_chunks_bfv(emu):
    import galois_set_cases as GS
    GS.case_chunks("bfv", *MID, lanes=1)


def test_launch_count(emu):
    import galois_set_cases as GS
    GS.case_launch_count(*MID, small=SMALL)


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
def test_pending_tail(emu, scheme):
    import galois_set_cases as GS
    GS.case_pending_tail(scheme, *MID)


def test_pending_operand(emu):
    import galois_set_cases as GS
    GS.case_pending_operand(*MID)


# the loop route in every scheme; the one-batch route once (its refusals and its check do not depend on the scheme)
ROUTES = [("ckks", SMALL), ("bfv", SMALL), ("bgv", SMALL), ("ckks", MID)]


@pytest.mark.parametrize("scheme,ring", ROUTES)
def test_refusals(emu, scheme, ring):
    import galois_set_cases as GS
    GS.case_refusals(scheme, *ring)


@pytest.mark.parametrize("scheme,ring", ROUTES + [("bfv", MID)])
def test_transparent_check(emu, scheme, ring):
    import galois_set_cases as GS
    GS.case_transparent_check(scheme, *ring)


@pytest.mark.parametrize("n,bits", [SMALL, MID])
def test_set_destroyed_after_the_call(emu, n, bits):
    import galois_set_cases as GS
    GS.case_destroy_after_call("ckks", n, bits)


@pytest.mark.parametrize("n,bits", [SMALL, MID])
def test_keys_changed(emu, n, bits):
    import galois_set_cases as GS
    GS.case_keys_changed("ckks", n, bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_create_errors(emu, scheme):
    import galois_set_cases as GS
    GS.case_create_errors(scheme, *SMALL)


def test_create_errors_register_order(emu):
    import galois_set_cases as GS
    GS.case_create_errors("ckks", *MID)


@needs_ref
def test_pipeline_diagonals(emu):
    import galois_set_cases as GS
    GS.case_pipeline_diagonals(*MID)
