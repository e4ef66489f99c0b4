"""One plaintext per item of a device-resident batch (Evaluator_AddPlainDevice / SubPlainDevice / MultiplyPlainDevice /
TransformPlainToNTTDevice), shared by the CPU (emulated kernels) and `-m gpu` suites.  Byte equality, per item, against two
yardsticks: the REAL reference (oracle/_ref) where it is built - add_plain_inplace / sub_plain_inplace / multiply_plain_inplace /
transform_to_ntt_inplace on its own objects - and the library's per-object forms on batches of one.  The per-object and the
per-item forms share their kernels and their host path (a shared plaintext is a per-item one with item stride 0), so agreement
between the two proves little by itself: the independent yardsticks are the reference here and parity_cases.case_plain_ops.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import sealref
from harness import DeviceSide
from oracle import coeff_modulus_create, plain_modulus_batching

SCRATCH_BYTES = 256 << 20   # include/sealhip.h: the cap of a chunk's lifted plaintexts
OPS = ("add", "sub", "multiply")
REF_OP = {"add": "add_plain_inplace", "sub": "sub_plain_inplace", "multiply": "multiply_plain_inplace"}


def chunk_items(n, K, budget=SCRATCH_BYTES):
    """items per chunk, as include/sealhip.h states it"""
    return max(1, budget // (8 * K * n))


def combos(scheme):
    """(operation, ciphertext in NTT form, plaintexts in NTT form): what the per-object forms accept for the scheme"""
    if scheme == "ckks":
        return [(op, True, True) for op in OPS]
    if scheme == "bfv":
        return [("add", False, False), ("sub", False, False)] + [("multiply", c, p) for c in (False, True) for p in (False, True)]
    return [("add", True, False), ("sub", True, False), ("multiply", True, False), ("multiply", True, True)]


class Side:
    def __init__(self, scheme, n, bits, tbits=20):
        self.scheme, self.n, self.bits = scheme, n, bits
        self.primes = coeff_modulus_create(n, bits)
        self.t = plain_modulus_batching(n, tbits) if scheme != "ckks" else 0
        self.d = DeviceSide(scheme, n, self.primes, self.t)
        self.ctx, self.ev = self.d.ctx, self.d.ev
        self.ref = sealref.RefContext(scheme, n, self.primes, self.t) if sealref.available() else None
        self.first = self.ctx.chain_index(self.ctx.first_parms_id())
        self.cf = 3 if scheme == "bgv" else 1
        self.scale = 2.0 ** 10 if scheme == "ckks" else 1.0

    def q(self, ci):
        return np.array(self.ctx.coeff_modulus_at(ci), dtype=np.uint64)

    def rand_ct(self, rng, ci, batch, size):
        """[size][batch][K][N] words below their primes"""
        q = self.q(ci)
        return (rng.integers(0, 2 ** 63, (size, batch, q.size, self.n), dtype=np.uint64) % q[None, None, :, None]).astype(np.uint64)

    def rand_plain(self, rng, ci, batch, ntt):
        if ntt:
            q = self.q(ci)
            w = (rng.integers(0, 2 ** 63, (batch, q.size, self.n), dtype=np.uint64) % q[None, :, None]).astype(np.uint64)
            w[:, :, 0] = 0
            w[:, :, 1] = q - 1
            return w
        w = rng.integers(0, self.t, (batch, self.n), dtype=np.uint64)   # both sides of (t + 1) / 2
        w[:, 0] = self.t - 1
        w[:, 1] = (self.t + 1) // 2
        w[:, 2] = (self.t + 1) // 2 - 1
        return w

    def dev_ct(self, words, ci, ntt):
        return S.Ciphertext.from_numpy(self.ctx, words, self.ctx.parms_id_at(ci), ntt, self.scale, self.cf)

    def plaintext(self, words_b, ci, ntt):
        if ntt:
            return S.Plaintext.from_numpy(self.ctx, words_b, self.ctx.parms_id_at(ci), self.scale)
        return S.Plaintext.from_numpy(self.ctx, words_b)

    def call(self, op, ct, buf, plain_ntt, destination=None, scale=None):
        fn = getattr(self.ev, "%s_plain_device" % op)
        return fn(ct, buf, plain_ntt, self.scale if scale is None else scale, destination=destination)

    def expect_item(self, op, ct_words_b, plain_b, ci, ct_ntt, plain_ntt):
        """item b through the per-object form on a batch of one -> (words [size][K][N], metadata); the reference, where it is
        built, must say the same"""
        c = self.dev_ct(ct_words_b[:, None], ci, ct_ntt)
        getattr(self.ev, "%s_plain_inplace" % op)(c, self.plaintext(plain_b, ci, plain_ntt))
        words, meta = c.to_numpy()[:, 0], (c.is_ntt_form(), c.scale(), c.correction_factor())
        if self.ref is not None:
            r = self.ref.ct(ci, ct_words_b, ct_ntt, self.scale, self.cf)
            rp = self.ref.pt(plain_b, ci, self.scale) if plain_ntt else self.ref.pt(plain_b)
            try:
                getattr(self.ref, REF_OP[op])(r, rp)
            except sealref.RefError:
                # the reference is built with SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT: a product with the zero plaintext is refused
                # there (logic_error).  With the check off, as here, the per-object form gives the zero ciphertext
                assert op == "multiply" and not np.any(plain_b) and not np.any(words), ("reference refused", op, ct_ntt, plain_ntt)
                return words, meta
            i = r.info()
            assert np.array_equal(words, r.data()), ("per-object form and reference disagree", op, ct_ntt, plain_ntt)
            assert meta == (i["is_ntt_form"], i["scale"], i["correction_factor"])
        return words, meta

    def check(self, what, got_ct, op, ct_words, plain, ci, ct_ntt, plain_ntt, items=None):
        got = got_ct.to_numpy()
        batch = ct_words.shape[1]
        assert got.shape == ct_words.shape, (what, got.shape)
        for b in (range(batch) if items is None else items):
            words, meta = self.expect_item(op, ct_words[:, b], plain[b], ci, ct_ntt, plain_ntt)
            assert np.array_equal(got[:, b], words), (what, "item", b)
            assert (got_ct.is_ntt_form(), got_ct.scale(), got_ct.correction_factor()) == meta, (what, "metadata")


def case_parity(scheme, n, bits, batch, sizes=(2, 3), ci=None, seed=5, side=None, items=None, only=None):
    """every accepted combination of forms, all three operations, in place: item b equals the per-object form and the reference"""
    side = side or Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    for size in sizes:
        for op, ct_ntt, plain_ntt in combos(scheme):
            if only is not None and (op, ct_ntt, plain_ntt) not in only:
                continue
            x = side.rand_ct(rng, ci, batch, size)
            pl = side.rand_plain(rng, ci, batch, plain_ntt)
            c = side.dev_ct(x, ci, ct_ntt)
            out = side.call(op, c, S.DeviceBuffer.from_numpy(pl), plain_ntt)
            assert out is c
            side.check((scheme, n, op, ct_ntt, plain_ntt, size), c, op, x, pl, ci, ct_ntt, plain_ntt, items)


def branch_plaintexts(side, rng):
    """coefficient-form plaintexts that steer the branches, in one batch: monomials next to other items"""
    n, t = side.n, side.t
    w = np.zeros((8, n), dtype=np.uint64)
    w[0] = rng.integers(0, t, n, dtype=np.uint64)           # both sides of (t + 1) / 2
    w[0, :2] = ((t + 1) // 2, (t + 1) // 2 - 1)
    w[1, 4] = t - 2                                         # a monomial with an upper-half coefficient (parity_cases.py)
    w[2] = 0                                                # zero
    w[3, : n // 4] = rng.integers(1, t, n // 4, dtype=np.uint64)   # non-zero only in the first N / 4 coefficients
    w[4, 0] = t - 3                                         # a monomial at exponent 0
    w[5, n - 1] = 5                                         # a monomial at exponent N - 1, lower half
    w[6] = rng.integers(0, t, n, dtype=np.uint64)
    w[7, n - 1] = (t + 1) // 2                              # odd exponent, the threshold itself
    return w


def case_branches(scheme, n, bits, tbits=20, size=2, seed=9):
    """plaintext values that steer branches: the centred lift's two sides, zero, a short plaintext, monomials (raw coefficient
    under the fast plain lift; increment per prime otherwise) at exponents 0, 4, N - 1 next to other items.  Coefficient-form
    ciphertexts take the monomial branch per item (BFV; BGV accepts the combination too, as the reference does)."""
    side = Side(scheme, n, bits, tbits)
    rng = np.random.default_rng(seed)
    pl = branch_plaintexts(side, rng)
    batch, ci = pl.shape[0], side.first
    fast = all(side.t < q for q in side.ctx.coeff_modulus_at(ci))
    buf = S.DeviceBuffer.from_numpy(pl)
    todo = [c for c in combos(scheme) if not c[2]] + [("multiply", False, False)]
    for op, ct_ntt, plain_ntt in dict.fromkeys(todo):
        x = side.rand_ct(rng, ci, batch, size)
        c = side.dev_ct(x, ci, ct_ntt)
        side.call(op, c, buf, False)
        side.check((scheme, "branches", op, ct_ntt, "fast lift" if fast else "general lift"), c, op, x, pl, ci, ct_ntt, False)
    return fast


C_ABI = {"add": "Evaluator_AddPlain", "sub": "Evaluator_SubPlain", "multiply": "Evaluator_MultiplyPlain"}


def case_shared_plaintext(scheme, n, bits, tbits, batch=3, size=2, seed=19):
    """ONE Plaintext handle of coeff_count 1, 5, N - 1 and N words applied to a batch (item stride 0): every item, in place and
    out of place through the C ABI, carries the words of the REFERENCE's own add / sub / multiply_plain_inplace on that item.
    Coefficients beyond coeff_count act as zero and are never read.  Among the plaintexts the 5-coefficient monomial with an
    upper-half coefficient: the raw coefficient under the fast plain lift, the increment per prime otherwise.  -> fast lift?"""
    side = Side(scheme, n, bits, tbits)
    ref, t, ci = side.ref, side.t, side.first
    assert ref is not None, "this case compares with the reference alone"
    rng = np.random.default_rng(seed)
    fast = all(t < q for q in side.ctx.coeff_modulus_at(ci))
    plains = []
    for cc in (1, 5, n - 1, n):
        w = rng.integers(1, t, cc, dtype=np.uint64)
        w[-1] = t - 1 - cc            # upper half, and the last word the plaintext holds
        w[0] = (t + 1) // 2 - (cc & 1)   # the threshold itself / the value below it
        plains.append(w)
    mono = np.zeros(5, dtype=np.uint64)
    mono[4] = t - 2
    plains.append(mono)
    todo = [c for c in combos(scheme) if not c[2]] + [("multiply", False, False)]
    for op, ct_ntt, _ in dict.fromkeys(todo):
        for w in plains:
            x = side.rand_ct(rng, ci, batch, size)
            want = []
            for b in range(batch):
                r = ref.ct(ci, x[:, b], ct_ntt, side.scale, side.cf)
                getattr(ref, REF_OP[op])(r, ref.pt(w))
                want.append((r.data(), r.info()))
            pt = S.Plaintext.from_numpy(side.ctx, w)
            assert pt.coeff_count() == w.size
            c = side.dev_ct(x, ci, ct_ntt)
            src = side.dev_ct(x, ci, ct_ntt)
            dest = S.Ciphertext(side.ctx, batch=batch)
            getattr(side.ev, "%s_plain_inplace" % op)(c, pt)
            side.ev._pl(C_ABI[op], src, pt, dest, pool=op == "multiply")
            assert np.array_equal(src.to_numpy(), x), ("encrypted changed", scheme, op, ct_ntt, w.size)
            for what, got_ct in (("in place", c), ("out of place", dest)):
                got = got_ct.to_numpy()
                assert got.shape == x.shape, (what, got.shape)
                for b in range(batch):
                    words, i = want[b]
                    assert np.array_equal(got[:, b], words), (what, scheme, op, ct_ntt, "coeff_count", w.size, "item", b, "fast" if fast else "general")
                    assert (got_ct.is_ntt_form(), got_ct.scale(), got_ct.correction_factor()) == \
                        (i["is_ntt_form"], i["scale"], i["correction_factor"]), (what, "metadata")
    return fast


def case_transform(scheme, n, bits, batch, seed=13):
    """TransformPlainToNTTDevice: item for item the per-object and the reference transform, at the first and at a lower level; its
    output with plain_is_ntt=True gives the words of the coefficient-form call"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    pl = side.rand_plain(rng, side.first, batch, False)
    pl[0, n // 2:] = 0
    buf = S.DeviceBuffer.from_numpy(pl)
    for ci in [c for c in (side.first, side.first - 1) if c >= 0]:
        pid, K = side.ctx.parms_id_at(ci), len(side.ctx.coeff_modulus_at(ci))
        out = side.ev.transform_plain_to_ntt_device(buf, batch, pid)
        got = out.to_numpy((batch, K, n))
        for b in range(batch):
            p = S.Plaintext.from_numpy(side.ctx, pl[b])
            side.ev.transform_plain_to_ntt_inplace(p, pid)
            assert np.array_equal(got[b].reshape(-1), p.to_numpy()), ("transform", scheme, ci, b)
            if side.ref is not None:
                rp = side.ref.pt_transform_to_ntt_inplace(side.ref.pt(pl[b]), ci)
                assert np.array_equal(got[b].reshape(-1), rp.data()), ("transform vs reference", scheme, ci, b)
        x = side.rand_ct(rng, ci, batch, 2)
        a = side.call("multiply", side.dev_ct(x, ci, True), out, True).to_numpy()
        b_ = side.call("multiply", side.dev_ct(x, ci, True), buf, False).to_numpy()
        assert np.array_equal(a, b_), ("pre-transformed plaintexts", scheme, ci)


def case_out_of_place(scheme, n, bits, batch=4, seed=17):
    """in place and out of place give the same words and metadata; out of place leaves `encrypted` bit-identical; the destination
    may have had another shape and batch"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    for op, ct_ntt, plain_ntt in combos(scheme):
        x = side.rand_ct(rng, ci, batch, 3 if op == "multiply" else 2)
        pl = side.rand_plain(rng, ci, batch, plain_ntt)
        if not plain_ntt:
            pl[1] = 0
            pl[1, 6] = side.t - 2   # a monomial: in place, the coefficient x coefficient product goes through a fresh slab
        buf = S.DeviceBuffer.from_numpy(pl)
        inplace = side.dev_ct(x, ci, ct_ntt)
        side.call(op, inplace, buf, plain_ntt)
        for dest in (S.Ciphertext(side.ctx, batch=batch), S.Ciphertext(side.ctx, batch=batch + 1), side.dev_ct(side.rand_ct(rng, 0, batch, 2), 0, ct_ntt)):
            src = side.dev_ct(x, ci, ct_ntt)
            out = side.call(op, src, buf, plain_ntt, destination=dest)
            assert out is dest and np.array_equal(src.to_numpy(), x), ("encrypted changed", op, ct_ntt, plain_ntt)
            assert np.array_equal(dest.to_numpy(), inplace.to_numpy()), ("out of place", op, ct_ntt, plain_ntt)
            assert (dest.parms_id(), dest.size(), dest.batch(), dest.is_ntt_form(), dest.scale(), dest.correction_factor()) == \
                (inplace.parms_id(), inplace.size(), batch, inplace.is_ntt_form(), inplace.scale(), inplace.correction_factor())
            assert (src.scale(), src.is_ntt_form(), src.correction_factor()) == (side.scale, ct_ntt, side.cf)


def case_chunks(scheme, n, bits, batch, per_chunk, monkeypatch):
    """a scratch cap that makes chunks of `per_chunk` lifted plaintexts (development builds: SEALHIP_PLAIN_SCRATCH_BYTES): every
    item, on both sides of every chunk edge, equals the per-object form"""
    side = Side(scheme, n, bits)
    K = len(side.ctx.coeff_modulus_at(side.first))
    monkeypatch.setenv("SEALHIP_PLAIN_SCRATCH_BYTES", str(per_chunk * 8 * K * n))
    assert chunk_items(n, K, per_chunk * 8 * K * n) == per_chunk and (batch - 1) // per_chunk >= 2, "at least two chunk edges"
    case_parity(scheme, n, bits, batch, sizes=(2,), side=side, only=[c for c in combos(scheme) if not c[2]])


def case_natural_chunks(scheme, n, bits, batch, seed=21):
    """no switch: the 256 MiB rule itself splits the batch (checked from the rule, not assumed); the first and last items and
    both sides of the chunk edge equal the per-object form"""
    side = Side(scheme, n, bits)
    K = len(side.ctx.coeff_modulus_at(side.first))
    per_chunk = chunk_items(n, K)
    assert per_chunk < batch, ("the rule does not split this batch", per_chunk, batch)
    only = [("multiply", True, False)] + ([("add", True, False)] if scheme == "bgv" else [])
    case_parity(scheme, n, bits, batch, sizes=(2,), side=side, only=only, items=[0, per_chunk - 1, per_chunk, batch - 1], seed=seed)


def _expect(exc, call, what):
    try:
        call()
    except exc:
        return
    raise AssertionError("expected %s: %s" % (exc.__name__, what))


def case_errors(scheme, n, bits, batch=3):
    """every check returns its HRESULT and leaves a separate destination untouched; a valid call afterwards works"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, lib = side.first, S._native.lib()
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    op, ct_ntt, plain_ntt = combos(scheme)[0]
    x = side.rand_ct(rng, ci, batch, 2)
    pl = side.rand_plain(rng, ci, batch, plain_ntt)
    buf = S.DeviceBuffer.from_numpy(pl)
    ct = side.dev_ct(x, ci, ct_ntt)
    dest = side.dev_ct(side.rand_ct(rng, ci, batch, 3), ci, ct_ntt)
    snapshot, meta = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.scale(), dest.is_ntt_form(), dest.correction_factor())
    other = Side(scheme, n, bits)
    foreign = other.dev_ct(x, ci, ct_ntt)

    def raw(fn, ct_h, ptr, b, ntt, scale, dest_h):
        return getattr(lib, fn)(side.ev._h, ct_h, C.c_void_p(ptr), C.c_uint64(b), C.c_bool(ntt), C.c_double(scale), dest_h) & 0xFFFFFFFF

    for name in ("Evaluator_AddPlainDevice", "Evaluator_SubPlainDevice", "Evaluator_MultiplyPlainDevice"):
        o = name[len("Evaluator_"):-len("PlainDevice")].lower()
        ok_ct_ntt, ok_pl_ntt = next((c, p) for k, c, p in combos(scheme) if k == o)
        assert (ok_ct_ntt, ok_pl_ntt) == (ct_ntt, plain_ntt)
        good = (ct._h, buf.ptr, batch, plain_ntt, side.scale, dest._h)
        assert raw(name, *good[:2], batch + 1, *good[3:]) == INVALID, "batch mismatch"
        assert raw(name, *good[:2], 0, *good[3:]) == INVALID, "batch 0"
        assert raw(name, ct._h, buf.ptr + 8, *good[2:]) == INVALID, "misaligned pointer"
        assert raw(name, ct._h, None, *good[2:]) == INVALID, "NULL device_plain"
        assert raw(name, None, *good[1:]) == POINTER and raw(name, *good[:5], None) == POINTER, "NULL handles"
        ptr, total = ct.device_ptr()
        assert raw(name, ct._h, ptr + 16, *good[2:]) == INVALID, "device_plain inside encrypted"
        ptr, total = dest.device_ptr()
        assert raw(name, ct._h, ptr + 16, *good[2:]) == INVALID, "device_plain inside destination"
        assert raw(name, foreign._h, *good[1:]) == INVALID, "a ciphertext of another context"
        # wrong form for the scheme
        wrong_ct = side.dev_ct(x, ci, not ct_ntt)
        if scheme == "ckks":
            assert raw(name, ct._h, buf.ptr, batch, False, side.scale, dest._h) == INVALID, "CKKS plain must be in NTT form"
            assert raw(name, *good[:4], 0.0, dest._h) == INVALID, "CKKS plaintext scale"
            if o != "multiply":
                assert raw(name, wrong_ct._h, *good[1:]) == INVALID, "CKKS ciphertext in coefficient form"
                assert raw(name, *good[:4], side.scale * 2, dest._h) == INVALID, "scale mismatch"
            else:
                assert raw(name, *good[:4], 2.0 ** 400, dest._h) == INVALID, "scale out of bounds"
        elif o != "multiply":
            assert raw(name, wrong_ct._h, *good[1:]) == INVALID, "ciphertext in the wrong form"
            big = S.DeviceBuffer(batch * len(side.ctx.coeff_modulus_at(ci)) * n)
            assert raw(name, ct._h, big.ptr, batch, True, side.scale, dest._h) == INVALID, "plaintext in NTT form"
        # a level expressed through the word count it implies: too few words for [batch][K][N] / [batch][N]
        small = S.DeviceBuffer(max(pl.size - n, 1))
        _expect(ValueError, lambda: side.call(o, ct, small, plain_ntt, destination=dest), "too few plaintext words for the level")
        assert np.array_equal(dest.to_numpy(), snapshot), (name, "a failed check must leave the destination untouched")
        assert (dest.parms_id(), dest.size(), dest.scale(), dest.is_ntt_form(), dest.correction_factor()) == meta, name
        assert np.array_equal(ct.to_numpy(), x)
    # the transform
    if scheme != "ckks":
        coeffs = S.DeviceBuffer.from_numpy(side.rand_plain(rng, ci, batch, False))
        K = len(side.ctx.coeff_modulus_at(ci))
        out = S.DeviceBuffer(batch * K * n)
        pid = (C.c_uint64 * 4)(*side.ctx.parms_id_at(ci))

        def tr(src, b, p, dst):
            return lib.Evaluator_TransformPlainToNTTDevice(side.ev._h, C.c_void_p(src), C.c_uint64(b), p, C.c_void_p(dst)) & 0xFFFFFFFF
        assert tr(coeffs.ptr, batch, (C.c_uint64 * 4)(1, 2, 3, 4), out.ptr) == INVALID, "unknown parms_id"
        assert tr(coeffs.ptr, 0, pid, out.ptr) == INVALID and tr(None, batch, pid, out.ptr) == INVALID
        assert tr(coeffs.ptr + 8, batch, pid, out.ptr) == INVALID and tr(coeffs.ptr, batch, pid, out.ptr + 8) == INVALID
        assert tr(out.ptr + 16 * n, batch, pid, out.ptr) == INVALID, "input overlapping output"
        assert tr(coeffs.ptr, batch, None, out.ptr) == POINTER
        assert tr(coeffs.ptr, batch, pid, out.ptr) == 0
    else:
        coeffs, out = S.DeviceBuffer(batch * n), S.DeviceBuffer(batch * len(side.ctx.coeff_modulus_at(ci)) * n)
        _expect(S.InvalidArgument, lambda: side.ev.transform_plain_to_ntt_device(coeffs, batch, side.ctx.parms_id_at(ci), out), "CKKS")
    # a valid call afterwards
    side.call(op, ct, buf, plain_ntt, destination=dest)
    side.check("after the failures", dest, op, x, pl, ci, ct_ntt, plain_ntt)


def case_transparent_check(scheme, n, bits, batch=2):
    """the transparent-ciphertext check, switched on, is the existing one over the batch"""
    side = Side(scheme, n, bits)
    op, ct_ntt, plain_ntt = [c for c in combos(scheme) if c[0] == "multiply"][-1]
    x = side.rand_ct(np.random.default_rng(3), side.first, batch, 2)
    x[1] = 0
    pl = side.rand_plain(np.random.default_rng(4), side.first, batch, plain_ntt)
    side.ev.set_transparent_check(True)
    try:
        _expect(S.LogicError, lambda: side.call("multiply", side.dev_ct(x, side.first, ct_ntt), S.DeviceBuffer.from_numpy(pl), plain_ntt), "transparent")
    finally:
        side.ev.set_transparent_check(False)


def _client(scheme, n, bits, tbits=20):
    """contexts and keys from the reference's seeded KeyGenerator"""
    import encrypt_batch_cases as EB
    return EB.Side(scheme, n, bits, ref_seed=0x5EA1, tbits=tbits)


def case_pipeline_ckks(n, bits, batch, seed=41):
    """encode_device -> encrypt_symmetric_device -> multiply_plain_device with a second encode_device output -> rescale_to_next ->
    decrypt_batch -> decode_device: the words after every evaluator stage and the decoded values equal the reference's, per item"""
    side = _client("ckks", n, bits)
    ref, ev = side.ref, side.d.ev
    enc = S.CKKSEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    pid, ci, slots = side.ctx.first_parms_id(), side.first, n // 2
    scale = 2.0 ** (bits[-2] if len(bits) > 2 else 12)
    a, w = rng.standard_normal((batch, slots)), rng.standard_normal((batch, slots))
    wa = enc.encode_device(S.DeviceBuffer.from_array(a), batch, pid, scale)
    ww = enc.encode_device(S.DeviceBuffer.from_array(w), batch, pid, scale)
    K = side.K(ci)
    ww_host = ww.to_numpy((batch, K, n))
    for b in range(batch):   # stage 1: the encoder's words are the reference's
        assert np.array_equal(ww_host[b].reshape(-1), ref.ckks_encode(w[b], ci, scale).data()), ("encode", b)
    side.enc.set_seed(None)
    A = side.enc.encrypt_symmetric_device(wa, batch, pid, scale)
    fresh = [A.save_bytes(item=b) for b in range(batch)]
    ev.multiply_plain_device(A, ww, True, scale)
    product = A.to_numpy()
    ev.rescale_to_next_inplace(A)
    rescaled = A.to_numpy()
    coeffs, _ = side.dec.decrypt_batch(A)
    got = enc.decode_device(coeffs, batch, A.parms_id(), A.scale()).to_array((batch, slots))
    for b in range(batch):
        r, _ = ref.ct_load(fresh[b])
        ref.multiply_plain_inplace(r, ref.pt(ww_host[b], ci, scale))
        assert np.array_equal(product[:, b], r.data()), ("multiply_plain_device", b)
        ref.rescale_to_next_inplace(r)
        assert np.array_equal(rescaled[:, b], r.data()) and A.scale() == r.info()["scale"], ("rescale", b)
        want = ref.ckks_decode(ref.decrypt(r), False)
        assert got[b].tobytes() == want.tobytes(), ("decode", b)
        assert np.max(np.abs(got[b] - a[b] * w[b])) < 1e-2, ("a * w", b)


def case_pipeline_bfv(n, bits, batch, seed=43):
    """BatchEncoder.encode_device -> encrypt_device -> add_plain_device + multiply_plain_device -> decrypt_batch -> decode_device:
    the ciphertext words after each stage equal the reference's per item, and the slots hold (a + u) * v modulo t"""
    side = _client("bfv", n, bits)
    ref, ev, t = side.ref, side.d.ev, side.t
    be = S.BatchEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    vals = [rng.integers(0, 50, (batch, n), dtype=np.uint64) for _ in range(3)]
    a, u, v = [be.encode_device(S.DeviceBuffer.from_numpy(x), batch) for x in vals]
    u_host, v_host = u.to_numpy((batch, n)), v.to_numpy((batch, n))
    side.enc.set_seed(None)
    A = side.enc.encrypt_device(a, batch)
    fresh = [A.save_bytes(item=b) for b in range(batch)]
    ev.add_plain_device(A, u, False)
    added = A.to_numpy()
    ev.multiply_plain_device(A, v, False)
    product = A.to_numpy()
    coeffs, _ = side.dec.decrypt_batch(A)
    got = be.decode_device(coeffs, batch).to_numpy((batch, n))
    plain_coeffs = coeffs.to_numpy((batch, n))
    for b in range(batch):
        r, _ = ref.ct_load(fresh[b])
        ref.add_plain_inplace(r, ref.pt(u_host[b]))
        assert np.array_equal(added[:, b], r.data()), ("add_plain_device", b)
        ref.multiply_plain_inplace(r, ref.pt(v_host[b]))
        assert np.array_equal(product[:, b], r.data()), ("multiply_plain_device", b)
        want = np.zeros(n, dtype=np.uint64)
        rd = ref.decrypt(r).data()
        want[: rd.size] = rd
        assert np.array_equal(plain_coeffs[b], want), ("decrypt", b)
        assert np.array_equal(got[b], (vals[0][b] + vals[1][b]) * vals[2][b] % t), ("(a + u) * v", b)


def case_capture(n, bits, batch, seed=47):
    """CKKS: multiply_plain_device + rescale recorded in a graph; the plaintext words are refreshed in place before each replay
    and the replay equals the eager result"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    x = side.rand_ct(rng, ci, batch, 2)
    cx = side.dev_ct(x, ci, True)
    buf = S.DeviceBuffer(batch * K * n)
    prod, res = S.Ciphertext(side.ctx, batch=batch), S.Ciphertext(side.ctx, batch=batch)
    # the eager yardstick writes objects of its own: a graph replays on the addresses its destinations had when it was recorded,
    # and an eager rescale of the same objects would give them new slabs
    prod_e, res_e = S.Ciphertext(side.ctx, batch=batch), S.Ciphertext(side.ctx, batch=batch)

    def refresh():
        pl = np.ascontiguousarray(side.rand_plain(rng, ci, batch, True))
        S._native.check(S._native.lib().shl_memcpy_h2d(C.c_void_p(buf.ptr), pl.ctypes.data_as(C.c_void_p), C.c_uint64(pl.nbytes)))

    def step(p=prod, r=res):
        side.ev.multiply_plain_device(cx, buf, True, side.scale, destination=p)
        side.ev.rescale_to_next(p, r)

    refresh()
    step()   # eager once
    graph = side.ev.capture(step)
    for trial in range(3):
        refresh()
        graph.launch()
        replay = res.to_numpy()
        step(prod_e, res_e)
        assert np.array_equal(replay, res_e.to_numpy()), ("graph replay", trial)
        assert np.array_equal(cx.to_numpy(), x), "the operand is only read"
        assert (res.scale(), res.is_ntt_form()) == (res_e.scale(), res_e.is_ntt_form())
        assert res.coeff_modulus_size() == K - 1 and res.size() == 2
