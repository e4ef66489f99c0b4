"""What the C layer outside Evaluator_* promises about its serialisable objects (Ciphertext, Plaintext, KSwitchKeys, SecretKey,
PublicKey, EncryptionParameters): which HRESULT and which SealHip_LastError words every *_Save gives for every capacity and
compression mode, the order in which the context-taking loads refuse, and what the key-object copies do.  The functions return what
they observe; tests/test_capi_objects.py (emulated build, N = 64) and tests/test_gpu_serialization.py (device, N = 4096) compare it
with the tables here, which were recorded before the entries were folded onto shared helpers."""
import ctypes as C

import numpy as np

import seal_amd._native as N
from harness import DeviceSide
from oracle import coeff_modulus_create, rand_ct

E_POINTER, E_INVALIDARG, COR_E_IO = N.E_POINTER, N.E_INVALIDARG, N.COR_E_IO
COR_E_INVALIDOPERATION, E_INVALID_INDEX = N.COR_E_INVALIDOPERATION, N.E_INVALID_INDEX
OK = (0, "")
KINDS = ("Ciphertext", "Plaintext", "KSwitchKeys", "SecretKey", "PublicKey", "EncParams")
MODES = (0, 1, 2, 9)   # none, zlib, zstd (looked up at run time), unknown


def outcome(hr):
    """-> (HRESULT, SealHip_LastError words) of a call; (0, "") for S_OK"""
    try:
        N.check(hr)
    except N.SealHipError as e:
        return e.hresult, e.message
    return OK


class Objects:
    """one object of every kind on a CKKS context, a second context with the same parameters, and what makes empty ones"""

    def __init__(self, S, n, bits, seed):
        self.S, self.n, self.primes = S, n, coeff_modulus_create(n, list(bits))
        self.K = K = len(self.primes) - 1
        self.d = DeviceSide("ckks", n, self.primes, 0)
        self.other = DeviceSide("ckks", n, self.primes, 0)
        self.rng = rng = np.random.default_rng(seed)
        ctx = self.d.ctx
        self.pid = self.d.parms_id_for_K(K)
        self.ct = self.d.ct([rand_ct(rng, self.primes, K, n)])
        self.ct2 = self.d.ct([rand_ct(rng, self.primes, K, n) for _ in range(2)])
        words = np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in self.primes[:K]])
        self.pt = S.Plaintext.from_numpy(ctx, words, self.pid, 2.0 ** 20)
        self.kg = S.KeyGenerator(ctx, seed=list(range(1, 9)))
        self.sk, self.pk, self.ksk = self.kg.secret_key(), self.kg.create_public_key(), self.kg.create_relin_keys()
        self.full = {"Ciphertext": self.ct, "Plaintext": self.pt, "KSwitchKeys": self.ksk, "SecretKey": self.sk,
                     "PublicKey": self.pk, "EncParams": self.d.parms}

    def empty(self, kind, side=None):
        S, ctx = self.S, (side or self.d).ctx
        return {"Ciphertext": lambda: S.Ciphertext(ctx), "Plaintext": lambda: S.Plaintext(ctx), "KSwitchKeys": lambda: S.RelinKeys(ctx),
                "SecretKey": lambda: S.SecretKey(ctx), "PublicKey": lambda: S.PublicKey(ctx),
                "EncParams": lambda: S.EncryptionParameters("ckks")}[kind]()


def save_size(kind, obj, mode):
    """-> ((HRESULT, words), size)"""
    v = C.c_int64(-1)
    return outcome(getattr(N.lib(), kind + "_SaveSize")(obj._h, C.c_uint8(mode), C.byref(v))), v.value


def save(kind, obj, capacity, mode):
    """*_Save into a buffer of exactly `capacity` bytes -> ((HRESULT, words), the bytes written)"""
    buf, nb = (C.c_uint8 * capacity)(), C.c_int64(-1)
    got = outcome(getattr(N.lib(), kind + "_Save")(obj._h, buf, C.c_uint64(capacity), C.c_uint8(mode), C.byref(nb)))
    return got, (C.string_at(buf, nb.value) if got == OK else None)


def load(kind, obj, context, data, unsafe=False, size=None):
    """*_Load / *_UnsafeLoad of data[:size] -> ((HRESULT, words), bytes read)"""
    data = bytes(data)
    size = len(data) if size is None else size
    nb, ptr = C.c_int64(-1), C.cast(C.c_char_p(data), C.c_void_p)
    fn = getattr(N.lib(), kind + ("_UnsafeLoad" if unsafe and kind != "EncParams" else "_Load"))
    args = (obj._h, ptr, C.c_uint64(size), C.byref(nb)) if kind == "EncParams" else (obj._h, context._h, ptr, C.c_uint64(size), C.byref(nb))
    return outcome(fn(*args)), nb.value


def stream(kind, obj, mode=0):
    """the object's whole stream, through a buffer of the size *_SaveSize names"""
    got, cap = save_size(kind, obj, mode)
    assert got == OK, got
    got, data = save(kind, obj, cap, mode)
    assert got == OK, got
    return data


# ---- the save matrix.  `raw` = *_SaveSize(mode 0), `packed` = the length of the whole stream in this mode.
def expected_save(kind, capacity, mode, raw, packed):
    """what *_Save answers, as the reference's Serialization::Save does (serialization.cpp:36-54, 193, 548): an unknown mode and a
    buffer below a header are invalid arguments, a buffer the stream does not fit is an I/O failure - with the one cell that differs:
    KSwitchKeys_Save calls every short uncompressed buffer an invalid argument (serial_cases.py:228 pins it)."""
    if mode == 9:
        return E_INVALIDARG, "unsupported compression mode"
    if kind == "KSwitchKeys" and mode == 0 and capacity < raw:
        return E_INVALIDARG, "capacity"
    if capacity < 16:
        return E_INVALIDARG, "insufficient size"
    if capacity < (raw if mode == 0 else packed):
        return COR_E_IO, "I/O error"
    return OK


def save_matrix(objects, kinds=KINDS):
    """-> [(kind, capacity name, mode, observed, expected)] over capacities 8, 16, 64, cap - 1, cap and every mode; at capacity
    cap the bytes written are loaded into an empty object, whose own stream has to equal the original's"""
    rows = []
    for kind in kinds:
        obj = objects.full[kind]
        got, raw = save_size(kind, obj, 0)
        assert got == OK and raw > 64, (kind, got, raw)
        plain = stream(kind, obj)
        assert len(plain) == raw
        for mode in MODES:
            got, _ = save_size(kind, obj, mode)
            if mode == 9:
                rows.append((kind, "size", mode, got, (E_INVALIDARG, "unsupported compression mode")))
                packed = raw
            elif got != OK:
                assert mode == 2, (kind, mode, got)   # zstd is looked up at run time: without it the mode is refused everywhere
                continue
            else:
                packed = len(stream(kind, obj, mode))
            for name, capacity in (("8", 8), ("16", 16), ("64", 64), ("cap-1", raw - 1), ("cap", raw)):
                got, data = save(kind, obj, capacity, mode)
                rows.append((kind, name, mode, got, expected_save(kind, capacity, mode, raw, packed)))
                if got == OK:
                    assert len(data) <= capacity and len(data) == (raw if mode == 0 else packed), (kind, name, mode, len(data))
                if got == OK and name == "cap":
                    back = objects.empty(kind)
                    assert load(kind, back, objects.d.ctx, data) == (OK, len(data)), (kind, mode)
                    assert stream(kind, back) == plain, (kind, mode, "the stream written at full capacity loads back into an equal object")
    return rows


def save_special_cases(objects):
    """-> {case: observed}: Ciphertext_Save on a batch of two, an item out of range, a digit-parallel slice of a key"""
    L, S = N.lib(), objects.S
    buf, nb = (C.c_uint8 * 64)(), C.c_int64()
    got = {}
    got["batch of two, no outptr"] = outcome(L.Ciphertext_Save(objects.ct2._h, None, C.c_uint64(64), C.c_uint8(0), C.byref(nb)))
    got["batch of two"] = outcome(L.Ciphertext_Save(objects.ct2._h, buf, C.c_uint64(64), C.c_uint8(0), C.byref(nb)))
    got["batch of two, unknown mode"] = outcome(L.Ciphertext_Save(objects.ct2._h, buf, C.c_uint64(64), C.c_uint8(9), C.byref(nb)))
    for mode in (0, 1, 9):
        got["item out of range, mode %d" % mode] = outcome(
            L.Ciphertext_SaveItem(objects.ct2._h, C.c_uint64(2), buf, C.c_uint64(64), C.c_uint8(mode), C.byref(nb)))
    got["item 1 of two"] = save_item_round_trip(objects)
    part = S.RelinKeys(objects.d.ctx)
    part.set_key_digits(0, 1, np.zeros((1, 2, len(objects.primes), objects.n), dtype=np.uint64))   # digit 1 only
    big = (C.c_uint8 * (1 << 16))()
    for mode in (0, 1, 9):
        got["slice, size, mode %d" % mode] = save_size("KSwitchKeys", part, mode)[0]
        got["slice, save, mode %d" % mode] = outcome(L.KSwitchKeys_Save(part._h, big, C.c_uint64(len(big)), C.c_uint8(mode), C.byref(nb)))
    got["slice, save, 8 bytes"] = outcome(L.KSwitchKeys_Save(part._h, big, C.c_uint64(8), C.c_uint8(0), C.byref(nb)))
    return got


def save_item_round_trip(objects):
    """slot 1 of a batch of two saved (zlib) and loaded into slot 0 of an empty batch of two: the words arrive"""
    S, ct2 = objects.S, objects.ct2
    data = ct2.save_bytes(item=1, compr_mode=1)
    back = S.Ciphertext(objects.d.ctx, batch=2)
    assert back.load_bytes(data, item=0) == len(data)
    assert back.save_bytes(item=0) == ct2.save_bytes(item=1)
    return OK


SAVE_SPECIAL = {
    "batch of two, no outptr": (E_INVALIDARG, "Ciphertext_Save needs a batch of one: use Ciphertext_SaveItem for a slot of a batch"),
    "batch of two": (E_INVALIDARG, "Ciphertext_Save needs a batch of one: use Ciphertext_SaveItem for a slot of a batch"),
    "batch of two, unknown mode": (E_INVALIDARG, "Ciphertext_Save needs a batch of one: use Ciphertext_SaveItem for a slot of a batch"),
    "item out of range, mode 0": (E_INVALID_INDEX, "batch item"),
    "item out of range, mode 1": (E_INVALID_INDEX, "batch item"),
    "item out of range, mode 9": (E_INVALIDARG, "unsupported compression mode"),
    "item 1 of two": OK,
    "slice, size, mode 0": (COR_E_INVALIDOPERATION, "a digit-parallel slice of a key cannot be saved"),
    "slice, size, mode 1": (COR_E_INVALIDOPERATION, "a digit-parallel slice of a key cannot be saved"),
    "slice, size, mode 9": (E_INVALIDARG, "unsupported compression mode"),
    "slice, save, mode 0": (COR_E_INVALIDOPERATION, "a digit-parallel slice of a key cannot be saved"),
    "slice, save, mode 1": (COR_E_INVALIDOPERATION, "a digit-parallel slice of a key cannot be saved"),
    "slice, save, mode 9": (E_INVALIDARG, "unsupported compression mode"),
    "slice, save, 8 bytes": (COR_E_INVALIDOPERATION, "a digit-parallel slice of a key cannot be saved"),
}


# ---- the order of refusals of the loads that take a context
LOADERS = ("Ciphertext", "Plaintext", "KSwitchKeys", "SecretKey", "PublicKey")


def load_order(objects):
    """-> {case: (observed, object left as it was)}.  "Another context" is a second context of the same parameters given in the
    context argument; "cut short" is the stream without its last 8 bytes."""
    d, other, L = objects.d, objects.other, N.lib()
    got = {}
    for kind in LOADERS:
        data = stream(kind, objects.full[kind])
        for unsafe in (False, True):
            for cut in (False, True):
                target = objects.empty(kind)
                assert load(kind, target, d.ctx, data) == (OK, len(data))
                before = stream(kind, target)
                seen, _ = load(kind, target, other.ctx, data, unsafe, len(data) - 8 if cut else None)
                case = "%s%s, another context%s" % (kind, " unsafe" if unsafe else "", ", cut short" if cut else "")
                got[case] = (seen, stream(kind, target) == before)
    data = stream("Ciphertext", objects.ct)

    def item_case(case, target, context, item, payload, size=None):
        before = [target.save_bytes(item=i) for i in range(2)]
        nb, ptr = C.c_int64(-1), C.cast(C.c_char_p(payload), C.c_void_p)
        size = len(payload) if size is None else size
        if item is None:
            seen = outcome(L.Ciphertext_Load(target._h, context._h, ptr, C.c_uint64(size), C.byref(nb)))
        else:
            seen = outcome(L.Ciphertext_LoadItem(target._h, context._h, C.c_uint64(item), ptr, C.c_uint64(size), C.byref(nb)))
        got[case] = (seen, [target.save_bytes(item=i) for i in range(2)] == before)

    item_case("Load into a batch of two", objects.ct2, d.ctx, None, data)
    item_case("Load into a batch of two, cut short", objects.ct2, d.ctx, None, data, len(data) - 8)
    item_case("Load into a batch of two, another context", objects.ct2, other.ctx, None, data)
    item_case("LoadItem, item out of range", objects.ct2, d.ctx, 2, data)
    item_case("LoadItem, item out of range, cut short", objects.ct2, d.ctx, 2, data, len(data) - 8)
    item_case("LoadItem, item out of range, another context", objects.ct2, other.ctx, 2, data)
    rescaled = objects.S.Ciphertext(d.ctx)
    assert rescaled.load_bytes(data) == len(data)
    rescaled.set_scale(2.0 ** 21)
    item_case("LoadItem, metadata disagrees", objects.ct2, d.ctx, 1, rescaled.save_bytes())
    item_case("LoadItem, metadata disagrees, another context", objects.ct2, other.ctx, 1, rescaled.save_bytes())
    return got


_CUT = (E_INVALIDARG, "SEALHeader.size exceeds available input")
_BATCH = (E_INVALIDARG, "Ciphertext_Load needs a batch of one: use Ciphertext_LoadItem for a slot of a batch")
LOAD_ORDER = {
    # the stream is parsed (against the context given) before the object's own context is compared
    "Ciphertext, another context": ((E_INVALIDARG, "ciphertext belongs to another context"), True),
    "Ciphertext, another context, cut short": (_CUT, True),
    "Ciphertext unsafe, another context": ((E_INVALIDARG, "ciphertext belongs to another context"), True),
    "Ciphertext unsafe, another context, cut short": (_CUT, True),
    # these three compare the context first
    "Plaintext, another context": ((E_INVALIDARG, "plaintext belongs to another context"), True),
    "Plaintext, another context, cut short": ((E_INVALIDARG, "plaintext belongs to another context"), True),
    "Plaintext unsafe, another context": ((E_INVALIDARG, "plaintext belongs to another context"), True),
    "Plaintext unsafe, another context, cut short": ((E_INVALIDARG, "plaintext belongs to another context"), True),
    "SecretKey, another context": ((E_INVALIDARG, "secret key belongs to another context"), True),
    "SecretKey, another context, cut short": ((E_INVALIDARG, "secret key belongs to another context"), True),
    "SecretKey unsafe, another context": ((E_INVALIDARG, "secret key belongs to another context"), True),
    "SecretKey unsafe, another context, cut short": ((E_INVALIDARG, "secret key belongs to another context"), True),
    "PublicKey, another context": ((E_INVALIDARG, "public key belongs to another context"), True),
    "PublicKey, another context, cut short": ((E_INVALIDARG, "public key belongs to another context"), True),
    "PublicKey unsafe, another context": ((E_INVALIDARG, "public key belongs to another context"), True),
    "PublicKey unsafe, another context, cut short": ((E_INVALIDARG, "public key belongs to another context"), True),
    # KSwitchKeys_Load compares no context itself: the object does when the first key is set, after the previous keys were dropped
    "KSwitchKeys, another context": ((E_INVALIDARG, "kswitch_keys belongs to another context"), False),
    "KSwitchKeys, another context, cut short": (_CUT, True),
    "KSwitchKeys unsafe, another context": ((E_INVALIDARG, "kswitch_keys belongs to another context"), False),
    "KSwitchKeys unsafe, another context, cut short": (_CUT, True),
    "Load into a batch of two": (_BATCH, True),
    "Load into a batch of two, cut short": (_BATCH, True),
    "Load into a batch of two, another context": (_BATCH, True),
    "LoadItem, item out of range": ((E_INVALID_INDEX, "batch item"), True),
    "LoadItem, item out of range, cut short": (_CUT, True),
    "LoadItem, item out of range, another context": ((E_INVALIDARG, "ciphertext belongs to another context"), True),
    "LoadItem, metadata disagrees": ((E_INVALIDARG, "serialized ciphertext does not match the metadata of the batch"), True),
    "LoadItem, metadata disagrees, another context": ((E_INVALIDARG, "ciphertext belongs to another context"), True),
}


class _Handle:
    def __init__(self, handle):
        self._h = handle


# ---- SecretKey / PublicKey: Create2, Assign, ParmsId on a set key and on an empty one
def key_copies(objects):
    L, got = N.lib(), {}
    zero, key_pid = (0, 0, 0, 0), objects.d.ctx.key_parms_id()

    def parms_id(kind, handle):
        out = (C.c_uint64 * 4)()
        assert outcome(getattr(L, kind + "_ParmsId")(handle, out)) == OK
        return tuple(out)

    for kind in ("SecretKey", "PublicKey"):
        full, empty, foreign = objects.full[kind], objects.empty(kind), objects.empty(kind, objects.other)
        words = stream(kind, full)
        assert parms_id(kind, full._h) == key_pid and parms_id(kind, empty._h) == zero
        for name, source in (("set", full), ("empty", empty)):
            h = C.c_void_p()
            got["%s Create2 of the %s key" % (kind, name)] = outcome(getattr(L, kind + "_Create2")(source._h, C.byref(h)))
            assert parms_id(kind, h) == (key_pid if source is full else zero)
            assert stream(kind, _Handle(h)) == stream(kind, source)
            assert outcome(getattr(L, kind + "_Destroy")(h)) == OK
        target = objects.empty(kind)
        got["%s Assign from an empty key" % kind] = outcome(getattr(L, kind + "_Assign")(target._h, empty._h))
        assert parms_id(kind, target._h) == zero
        got["%s Assign across contexts" % kind] = outcome(getattr(L, kind + "_Assign")(foreign._h, full._h))
        assert parms_id(kind, foreign._h) == zero
        got["%s Assign" % kind] = outcome(getattr(L, kind + "_Assign")(target._h, full._h))
        assert parms_id(kind, target._h) == key_pid and stream(kind, target) == words
    return got


KEY_COPIES = {
    "SecretKey Create2 of the set key": OK, "SecretKey Create2 of the empty key": OK, "SecretKey Assign": OK,
    "SecretKey Assign from an empty key": (E_INVALIDARG, "secret key is not set"),
    "SecretKey Assign across contexts": (E_INVALIDARG, "secret keys belong to different contexts"),
    "PublicKey Create2 of the set key": OK, "PublicKey Create2 of the empty key": OK, "PublicKey Assign": OK,
    "PublicKey Assign from an empty key": (E_INVALIDARG, "public key is not set"),
    "PublicKey Assign across contexts": (E_INVALIDARG, "public keys belong to different contexts"),
}


def mismatches(observed, expected):
    """the cases whose observation differs from the table (both directions), for an assertion message that names them"""
    keys = sorted(set(observed) | set(expected))
    return [(k, observed.get(k), expected.get(k)) for k in keys if observed.get(k) != expected.get(k)]
