"""CPU (emulated kernels): what the host code above the kernels promises a caller and a consolidation of it could silently change -
which NULL handles every Evaluator_* export answers with E_POINTER, that sub refuses what add refuses, that the out-of-place
multiply refuses what multiply_inplace refuses, that the in-place and out-of-place rotations and conjugations refuse alike, and
what the *_to walkers do with an unknown, a higher and the current level.  "Words" of a refusal are SealHip_LastError's."""
import ctypes as C

import numpy as np
import pytest

import seal_amd._native as N
from seal_amd.api import Conv2dShape
from harness import DeviceSide
from oracle import Oracle, coeff_modulus_create, plain_modulus_batching, rand_ct

n = 64
E_POINTER, E_INVALIDARG, COR_E_INVALIDOPERATION = N.E_POINTER, N.E_INVALIDARG, N.COR_E_INVALIDOPERATION


def refusal(call):
    """-> (HRESULT, words) of a call that must fail"""
    with pytest.raises(N.SealHipError) as e:
        call()
    return e.value.hresult, e.value.message


class Side:
    """one scheme at N = 64 with a relinearisation key and the Galois key of one step"""

    def __init__(self, S, scheme, seed):
        self.S, self.scheme = S, scheme
        if scheme == "ckks":
            self.primes, self.t = coeff_modulus_create(n, [40, 30, 30, 40]), 0
        else:
            self.primes, self.t = coeff_modulus_create(n, [30, 30, 30, 30]), plain_modulus_batching(n, 12)
        self.K = len(self.primes) - 1
        self.o = Oracle(scheme, n, self.primes, self.t, galois_elts=[3], kind="port")   # element 3 = one step to the left
        self.d = DeviceSide(scheme, n, self.primes, self.t)
        self.d.upload_keys(self.o)
        self.other = DeviceSide(scheme, n, self.primes, self.t)                         # the same parameters, another context
        self.rng = np.random.default_rng(seed)

    def ct(self, K=None, batch=1, side=None, **kw):
        K = self.K if K is None else K
        return (side or self.d).ct([rand_ct(self.rng, self.primes, K, n) for _ in range(batch)], **kw)


@pytest.fixture(scope="module")
def ckks(emu):
    return Side(emu, "ckks", 11)


@pytest.fixture(scope="module")
def bfv(emu):
    return Side(emu, "bfv", 12)


# ---- every Evaluator_* export: a NULL in each handle position that is checked gives E_POINTER.  One word per argument; the ones in
#      capitals are the checked handles, the others are never E_POINTER (the C++ layer refuses a null among them as E_INVALIDARG).
UNARY, UNARY_POOL, BINARY = "EV CT DST", "EV CT DST pool", "EV CT CT2 DST"
PLAIN_DEVICE, TO = "EV CT dev u64 bool dbl DST", "EV CT PID DST pool"
EXPORTS = {
    "Evaluator_Create": "CTX OUTH", "Evaluator_Destroy": "EV", "Evaluator_SetStream": "EV stream", "Evaluator_BeginCapture": "EV",
    "Evaluator_EndCapture": "EV OUTH", "Evaluator_LaunchGraph": "EV GRAPH", "Evaluator_SetTransparentCheck": "EV bool",
    "Evaluator_CopyTo": UNARY, "Evaluator_Synchronize": "EV",
    "Evaluator_Negate": UNARY, "Evaluator_TransformToNTT2": UNARY, "Evaluator_TransformFromNTT": UNARY,
    "Evaluator_Square": UNARY_POOL, "Evaluator_ModSwitchToNext1": UNARY_POOL, "Evaluator_RescaleToNext": UNARY_POOL,
    "Evaluator_ModReduceToNext": UNARY_POOL,
    "Evaluator_AddPlain": "EV CT PT DST", "Evaluator_SubPlain": "EV CT PT DST", "Evaluator_MultiplyPlain": "EV CT PT DST pool",
    "Evaluator_AddPlainDevice": PLAIN_DEVICE, "Evaluator_SubPlainDevice": PLAIN_DEVICE, "Evaluator_MultiplyPlainDevice": PLAIN_DEVICE,
    "Evaluator_TransformPlainToNTTDevice": "EV dev u64 PID dev",
    "Evaluator_SumItems": "EV CT u64 DST", "Evaluator_DotPlainDevice": "EV CT dev u64 u64 dbl DST",
    "Evaluator_DotItems": "EV CT CT2 u64 DST",
    "Evaluator_SumItemsMapped": "EV CT MAP DST", "Evaluator_DotPlainMapped": "EV CT dev u64 MAP dbl DST",
    "Evaluator_DotScalarsMapped": "EV CT dev u64 MAP flags dbl DST", "Evaluator_DotItemsMapped": "EV CT CT2 MAP DST",
    "Evaluator_LiftScalars": "EV u64 host PID dev", "Evaluator_DotScalarsDevice": "EV CT dev u64 u64 dbl DST",
    "Evaluator_MatMulItems": "EV CT CT2 u64 u64 u64 flags DST",
    "Evaluator_MatMulPlainItems": "EV dev CT u64 u64 u64 flags dbl DST",
    "Evaluator_MatMulScalarsItems": "EV dev CT u64 u64 u64 flags dbl DST",
    "Evaluator_Conv2dScalarsItems": "EV dev CT shape flags dbl DST",
    "Evaluator_TransformToNTT1": "EV PT PID PDST pool", "Evaluator_ModSwitchToNext2": "EV PT PDST",
    "Evaluator_ModSwitchTo2": "EV PT PID PDST",
    "Evaluator_AddMany": "EV u64 CTS DST", "Evaluator_MultiplyMany": "EV u64 CTS RLK DST pool",
    "Evaluator_Exponentiate": "EV CT u64 RLK DST pool",
    "Evaluator_Add": BINARY, "Evaluator_Sub": BINARY, "Evaluator_Multiply": BINARY + " pool",
    "Evaluator_Relinearize": "EV CT RLK DST pool",
    "Evaluator_SwitchKeyAccWords": "EV CT OUT64", "Evaluator_RelinearizePartial": "EV CT RLK u64 u64 ACC",
    "Evaluator_RelinearizeFinish": "EV CT ACC u64", "Evaluator_ApplyGaloisPartial": "EV CT u32 GLK u64 u64 ACC",
    "Evaluator_ApplyGaloisFinish": "EV CT ACC u64",
    "Evaluator_RelinearizeDigitParallel": "EV CT RLK COMM int DST",
    "Evaluator_ApplyGaloisDigitParallel": "EV CT u32 GLK COMM int DST",
    "Evaluator_RotateVectorDigitParallel": "EV CT int GLK COMM int DST",
    "Evaluator_BroadcastKeyDigits": "EV RLK u64 ACC COMM int",
    "Evaluator_SwitchKeySlots": "EV CT u64 OUT64", "Evaluator_SwitchKeyPackTargets": "EV CT dev u64 dev dev",
    "Evaluator_SwitchKeyFinishOwned": "EV CT dev dev u64 u64 dev", "Evaluator_SwitchKeyAddGathered": "EV CT dev u64",
    "Evaluator_ModSwitchTo1": TO, "Evaluator_RescaleTo": TO, "Evaluator_ModReduceTo": TO,
    "Evaluator_ApplyGalois": "EV CT u32 GLK DST pool", "Evaluator_RotateRows": "EV CT int GLK DST pool",
    "Evaluator_RotateVector": "EV CT int GLK DST pool", "Evaluator_RotateColumns": "EV CT GLK DST pool",
    "Evaluator_ComplexConjugate": "EV CT GLK DST pool",
    "Evaluator_ContextUsingKeyswitching": "EV OUTBOOL",
}


@pytest.fixture(scope="module")
def arguments(ckks):
    """a valid argument of every kind (live objects of one CKKS context); the objects are kept alive beside the ctypes values"""
    S, d = ckks.S, ckks.d
    x, y, dest = ckks.ct(), ckks.ct(), S.Ciphertext(d.ctx)
    pid = d.parms_id_for_K(ckks.K)
    plain = S.Plaintext.from_numpy(d.ctx, np.zeros((ckks.K, n), dtype=np.uint64), pid, 2.0 ** 20)
    plain2 = S.Plaintext(d.ctx)
    item_map = S.ItemMap(d.ctx, [[0]], 1)
    comm = S.Comm(S.Comm.unique_id(), 1, 0)
    words = S.DeviceBuffer(4 * (ckks.K + 1) * n)
    host = (C.c_uint64 * 4)(1, 2, 3, 4)
    not_a_graph = (C.c_uint64 * 8)()   # (a recording is not made for this: a call with a NULL elsewhere returns before it looks)
    keep = [x, y, dest, plain, plain2, item_map, comm, words, host, not_a_graph]
    values = {
        "EV": d.ev._h, "CTX": d.ctx._h, "CT": x._h, "CT2": y._h, "DST": dest._h, "PT": plain._h, "PDST": plain2._h,
        "RLK": d.rlk._h, "GLK": d.glk._h, "MAP": item_map._h, "COMM": comm._h, "PID": (C.c_uint64 * 4)(*pid),
        "ACC": C.c_void_p(words.ptr), "CTS": (C.c_void_p * 2)(x._h.value, y._h.value), "GRAPH": C.c_void_p(C.addressof(not_a_graph)),
        "OUTH": C.pointer(C.c_void_p()), "OUT64": C.pointer(C.c_uint64()), "OUTBOOL": C.pointer(C.c_bool()),
        "dev": C.c_void_p(words.ptr), "host": host, "u64": C.c_uint64(1), "u32": C.c_uint32(3), "int": C.c_int(1),
        "dbl": C.c_double(2.0 ** 20), "bool": C.c_bool(True), "flags": C.c_uint64(0), "pool": None, "stream": None,
        "shape": C.pointer(Conv2dShape(1, 1, 1, 1, 1, 1, 1, 1, 0, 0)),
    }
    return values, keep


def test_table_names_every_evaluator_export():
    assert sorted(EXPORTS) == sorted(s for s in N.SYMBOLS if s.startswith("Evaluator_"))


@pytest.mark.parametrize("symbol", sorted(EXPORTS))
def test_null_handle_is_e_pointer(arguments, symbol):
    values, _ = arguments
    kinds = EXPORTS[symbol].split()
    checked = [i for i, k in enumerate(kinds) if k.isupper()]
    assert checked and checked[0] == 0
    fn = getattr(N.lib(), symbol)
    for i in checked:
        args = [None if j == i else values[k] for j, k in enumerate(kinds)]
        assert fn(*args) & 0xFFFFFFFF == E_POINTER, (symbol, "argument %d (%s)" % (i, kinds[i]))


def test_null_device_pointers_are_invalid_arguments_not_e_pointer(ckks):
    """the pointers the C++ layer looks at itself: a null among them is std::invalid_argument"""
    S, d = ckks.S, ckks.d
    x, dest = ckks.ct(), S.Ciphertext(d.ctx)
    weights = S.DeviceBuffer(ckks.K)
    shape = Conv2dShape(1, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    conv = N.lib().Evaluator_Conv2dScalarsItems
    assert refusal(lambda: N.check(conv(d.ev._h, None, x._h, C.byref(shape), C.c_uint64(0), C.c_double(1.0), dest._h))) == \
        (E_INVALIDARG, "device_scalars is null")
    assert refusal(lambda: N.check(conv(d.ev._h, C.c_void_p(weights.ptr), x._h, None, C.c_uint64(0), C.c_double(1.0), dest._h))) == \
        (E_INVALIDARG, "shape is null")
    assert refusal(lambda: N.check(conv(d.ev._h, C.c_void_p(weights.ptr), x._h, C.byref(shape), C.c_uint64(8), C.c_double(1.0), dest._h))) == \
        (E_INVALIDARG, "unknown flags")
    add = N.lib().Evaluator_AddPlainDevice
    assert refusal(lambda: N.check(add(d.ev._h, x._h, None, C.c_uint64(1), C.c_bool(True), C.c_double(2.0 ** 20), dest._h))) == \
        (E_INVALIDARG, "device_plain is null")


# ---- sub_inplace refuses what add_inplace refuses
def addsub_refusals(side):
    K = side.K
    return {
        "level": lambda: (side.ct(K), side.ct(K - 1)),
        "ntt form": lambda: (side.ct(K, is_ntt=True), side.ct(K, is_ntt=False)),
        "scale": lambda: (side.ct(K, scale=2.0 ** 20), side.ct(K, scale=2.0 ** 21)),
        "batch": lambda: (side.ct(K, batch=1), side.ct(K, batch=2)),
    }


@pytest.mark.parametrize("what,words", [("level", "encrypted1 and encrypted2 parameter mismatch"), ("ntt form", "NTT form mismatch"),
                                        ("scale", "scale mismatch"), ("batch", "batch mismatch")])
def test_sub_refuses_what_add_refuses(ckks, what, words):
    ev = ckks.d.ev
    x, y = addsub_refusals(ckks)[what]()
    before = x.to_numpy()
    added = refusal(lambda: ev.add_inplace(x, y))
    assert added == (E_INVALIDARG, words)
    assert refusal(lambda: ev.sub_inplace(x, y)) == added
    assert np.array_equal(x.to_numpy(), before)


def test_bgv_add_sub_balance_unequal_correction_factors(emu):
    """balance_correction_factors (evaluator.cpp:50-117, 173-192, 259-278): both operands are scaled to a common factor first"""
    primes, t = coeff_modulus_create(n, [40, 40, 41]), plain_modulus_batching(n, 13)
    o = Oracle("bgv", n, primes, t)
    assert o.kind == "reference", "BGV parity needs oracle/_ref"
    d = DeviceSide("bgv", n, primes, t)
    rng = np.random.default_rng(13)
    for sizes in ((2, 2), (2, 3), (3, 2)):   # the longer operand's tail is copied (add) or negated (sub)
        a, b = rand_ct(rng, primes, 2, n, size=sizes[0]), rand_ct(rng, primes, 2, n, size=sizes[1])
        for op in ("add_inplace", "sub_inplace"):
            x, y = d.ct(a, is_ntt=True), d.ct(b, is_ntt=True)
            x.set_correction_factor(3)
            y.set_correction_factor(5)
            getattr(d.ev, op)(x, y)
            expected, info = o.run(op, [(a, 3), (b, 5)])
            assert np.array_equal(d.out(x)[0], expected), (op, sizes)
            assert x.correction_factor() == info["correction_factor"], (op, sizes)
            assert np.array_equal(d.out(y)[0], b) and y.correction_factor() == 5, (op, sizes)


# ---- multiply into a third object of the same context and batch refuses what multiply_inplace on a copy refuses
def multiply_refusals(side):
    K = side.K
    if side.scheme == "ckks":
        return {
            "level": lambda: (side.ct(K), side.ct(K - 1)),
            "batch": lambda: (side.ct(K, batch=1), side.ct(K, batch=2)),
            "coefficient form": lambda: (side.ct(K, is_ntt=False), side.ct(K)),
            "scale": lambda: (side.ct(K, scale=2.0 ** 60), side.ct(K, scale=2.0 ** 60)),
        }
    return {"ntt form": lambda: (side.ct(K, is_ntt=True), side.ct(K, is_ntt=True))}


def check_multiply_refusal(side, what, words):
    S, ev = side.S, side.d.ev
    x, y = multiply_refusals(side)[what]()
    a, b = x.to_numpy(), y.to_numpy()
    dest, copy = S.Ciphertext(side.d.ctx, batch=x.batch()), x.copy()
    out_of_place = refusal(lambda: ev.multiply(x, y, dest))
    assert out_of_place == (E_INVALIDARG, words)
    assert refusal(lambda: ev.multiply_inplace(copy, y)) == out_of_place
    assert np.array_equal(x.to_numpy(), a) and np.array_equal(y.to_numpy(), b)   # the operands are only read
    return dest, copy


@pytest.mark.parametrize("what,words", [("level", "encrypted1 and encrypted2 parameter mismatch"), ("batch", "batch mismatch"),
                                        ("coefficient form", "encrypted1 or encrypted2 must be in NTT form"),
                                        ("scale", "scale out of bounds")])
def test_ckks_multiply_into_third_object_refuses_like_inplace(ckks, what, words):
    dest, copy = check_multiply_refusal(ckks, what, words)
    if what == "scale":
        # the reference forms the product and sets the scale before it looks at the scale (evaluator.cpp:700-706): so do both paths
        assert dest.size() == copy.size() == 3 and dest.scale() == copy.scale() == 2.0 ** 120
        assert np.array_equal(dest.to_numpy(), copy.to_numpy())
    else:
        assert dest.size() == 0


def test_bfv_multiply_into_third_object_refuses_like_inplace(bfv):
    dest, _ = check_multiply_refusal(bfv, "ntt form", "encrypted1 or encrypted2 cannot be in NTT form")
    assert dest.size() == 0


# ---- rotations and conjugation: in place (destination = operand) and out of place refuse alike
ROTATIONS = {   # form -> (the scheme it serves, the one it refuses, call(ev, a, steps, keys, destination))
    "rotate_rows": ("bfv", "ckks", lambda ev, a, steps, keys, dest: ev.rotate_rows(a, steps, keys, dest)),
    "rotate_columns": ("bfv", "ckks", lambda ev, a, steps, keys, dest: ev.rotate_columns(a, keys, dest)),
    "rotate_vector": ("ckks", "bfv", lambda ev, a, steps, keys, dest: ev.rotate_vector(a, steps, keys, dest)),
    "complex_conjugate": ("ckks", "bfv", lambda ev, a, steps, keys, dest: ev.complex_conjugate(a, keys, dest)),
}


@pytest.mark.parametrize("form", sorted(ROTATIONS))
def test_rotation_refusals_in_place_and_out_of_place(ckks, bfv, form):
    sides = {"ckks": ckks, "bfv": bfv}
    serves, refuses, call = ROTATIONS[form]

    def both(side, operand, steps, keys):
        S, ev = side.S, side.d.ev
        x = operand()
        before = x.to_numpy()
        in_place = refusal(lambda: call(ev, x, steps, keys, x))
        assert np.array_equal(x.to_numpy(), before)
        dest = S.Ciphertext(side.d.ctx)
        assert refusal(lambda: call(ev, x, steps, keys, dest)) == in_place
        assert np.array_equal(x.to_numpy(), before)
        return in_place

    wrong, right = sides[refuses], sides[serves]
    assert both(wrong, wrong.ct, 1, wrong.d.glk) == (COR_E_INVALIDOPERATION, "unsupported scheme")
    assert both(right, lambda: right.ct(side=right.other), 1, right.d.glk) == \
        (E_INVALIDARG, "encrypted is not valid for encryption parameters")
    # the key of one step is there (element 3); four steps is one NAF term without a key, the column swap / conjugation has none
    assert both(right, right.ct, 4, right.d.glk) == (E_INVALIDARG, "Galois key not present")
    # ... and with the key both forms give the same ciphertext
    S, ev = right.S, right.d.ev
    if form in ("rotate_rows", "rotate_vector"):
        x = right.ct()
        dest = S.Ciphertext(right.d.ctx)
        call(ev, x, 1, right.d.glk, dest)
        call(ev, x, 1, right.d.glk, x)
        assert np.array_equal(x.to_numpy(), dest.to_numpy())


# ---- the *_to walkers: an unknown parms_id, a higher level, the level the object is at
UNKNOWN = (1, 2, 3, 4)
WALKERS = {
    "mod_switch_to": lambda ev, c, pid: ev.mod_switch_to_inplace(c, pid),
    "rescale_to": lambda ev, c, pid: ev.rescale_to_inplace(c, pid),
    "mod_reduce_to": lambda ev, c, pid: ev.mod_reduce_to_inplace(c, pid),
}


@pytest.mark.parametrize("walker", sorted(WALKERS))
def test_ciphertext_walkers(ckks, walker):
    d, ev, walk = ckks.d, ckks.d.ev, WALKERS[walker]
    x = ckks.ct(ckks.K - 1)
    before, level = x.to_numpy(), x.parms_id()
    assert refusal(lambda: walk(ev, x, UNKNOWN)) == (E_INVALIDARG, "parms_id is not valid for encryption parameters")
    assert refusal(lambda: walk(ev, x, d.parms_id_for_K(ckks.K))) == (E_INVALIDARG, "cannot switch to higher level modulus")
    foreign = ckks.ct(side=ckks.other)
    assert refusal(lambda: walk(ev, foreign, UNKNOWN)) == (E_INVALIDARG, "encrypted is not valid for encryption parameters")
    walk(ev, x, level)   # already there: nothing happens
    assert x.parms_id() == level and x.scale() == 2.0 ** 20 and np.array_equal(x.to_numpy(), before)
    walk(ev, x, d.parms_id_for_K(1))   # ... and it does walk
    assert x.parms_id() == d.parms_id_for_K(1) and x.coeff_modulus_size() == 1


def test_rescale_to_is_ckks_only_after_the_level_checks(bfv):
    d, ev = bfv.d, bfv.d.ev
    x = bfv.ct(bfv.K - 1)
    assert refusal(lambda: ev.rescale_to_inplace(x, UNKNOWN)) == (E_INVALIDARG, "parms_id is not valid for encryption parameters")
    assert refusal(lambda: ev.rescale_to_inplace(x, x.parms_id())) == (E_INVALIDARG, "unsupported operation for scheme type")


def test_plaintext_walker(ckks):
    S, d, ev = ckks.S, ckks.d, ckks.d.ev
    K = ckks.K - 1
    words = np.stack([ckks.rng.integers(0, ckks.primes[i], n, dtype=np.uint64) for i in range(K)])
    p = S.Plaintext.from_numpy(d.ctx, words, d.parms_id_for_K(K), 2.0 ** 20)
    assert refusal(lambda: ev.mod_switch_plain_to_inplace(p, UNKNOWN)) == (E_INVALIDARG, "parms_id is not valid for encryption parameters")
    assert refusal(lambda: ev.mod_switch_plain_to_inplace(p, d.parms_id_for_K(ckks.K))) == \
        (E_INVALIDARG, "cannot switch to higher level modulus")
    coefficients = S.Plaintext.from_numpy(d.ctx, np.arange(8, dtype=np.uint64))
    assert refusal(lambda: ev.mod_switch_plain_to_inplace(coefficients, UNKNOWN)) == (E_INVALIDARG, "plain is not in NTT form")
    ev.mod_switch_plain_to_inplace(p, d.parms_id_for_K(K))   # already there: nothing happens
    assert p.parms_id() == d.parms_id_for_K(K) and np.array_equal(p.to_numpy(), words.reshape(-1))
    ev.mod_switch_plain_to_inplace(p, d.parms_id_for_K(1))
    assert p.parms_id() == d.parms_id_for_K(1) and np.array_equal(p.to_numpy(), words[0])
