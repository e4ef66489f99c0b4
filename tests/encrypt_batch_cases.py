"""Batched encryption in device memory (Encryptor_EncryptSymmetricDevice / Encryptor_EncryptDevice), shared by the CPU
(emulated kernels) and `-m gpu` suites.  Two yardsticks: the REAL reference (oracle/_ref) where it is built - every item equals
the bytes of seal::Encryptor under the same seeded factory - and the per-object Encryptor_EncryptSymmetric / Encryptor_Encrypt:
item b equals them under set_seed(seeds[b]).  The per-object forms are the batch path at batch one, so that comparison pins
seeds and metadata; the arithmetic is checked by the reference, here and in decrypt_cases.py.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import sealref
from harness import DeviceSide
from oracle import coeff_modulus_create, plain_modulus_batching

SCRATCH_BYTES = 256 << 20   # include/sealhip.h: the chunks' scratch cap


def chunk_items(n, K_at, budget=SCRATCH_BYTES):
    """items per chunk, as include/sealhip.h states it; K_at = primes at the level the item is encrypted at"""
    return max(1, min(budget // (8 * K_at * n), 65535))


class Side:
    """contexts and keys: from the reference's seeded KeyGenerator (ref_seed given) or from the device's own"""

    def __init__(self, scheme, n, bits, ref_seed=None, tbits=20):
        self.scheme, self.n, self.bits = scheme, n, bits
        self.primes = coeff_modulus_create(n, bits)
        self.t = plain_modulus_batching(n, tbits) if scheme != "ckks" else 0
        self.d = DeviceSide(scheme, n, self.primes, self.t)
        self.ctx = self.d.ctx
        self.ref = None
        if ref_seed is not None:
            self.ref = sealref.RefContext(scheme, n, self.primes, self.t, seed=ref_seed)
            self.sk = S.SecretKey(self.ctx, self.ref.secret_key())
            self.pk = S.PublicKey(self.ctx, self.ref.public_key())
        else:
            self.kg = S.KeyGenerator(self.ctx, seed=np.array([0xC0FFEE, 1, 2, 3, 4, 5, 6, 7], dtype=np.uint64))
            self.sk, self.pk = self.kg.secret_key(), self.kg.create_public_key()
        self.first = self.ctx.chain_index(self.ctx.first_parms_id())
        self.key_ci = self.ctx.chain_index(self.ctx.key_parms_id())
        self.enc = S.Encryptor(self.ctx, self.sk, public_key=self.pk)
        self.dec = S.Decryptor(self.ctx, self.sk)

    def K(self, ci):
        return len(self.ctx.coeff_modulus_at(ci))

    def K_at(self, ci, public):
        """primes at the level an item is encrypted at: the level above for the public-key form where there is one"""
        return self.K(ci + 1) if public and ci + 1 <= self.key_ci else self.K(ci)

    def plain_words(self, rng, batch, ci):
        """one plaintext per item: CKKS [batch][K][N] residues (NTT form at ci), BFV / BGV [batch][N] coefficients modulo t"""
        if self.scheme == "ckks":
            q = np.array(self.primes[: self.K(ci)], dtype=np.uint64)
            w = rng.integers(0, 2 ** 63, (batch, q.size, self.n), dtype=np.uint64) % q[None, :, None]
            w[:, :, 0] = 0
            w[:, :, 1] = q - 1
            return w.astype(np.uint64)
        w = rng.integers(0, self.t, (batch, self.n), dtype=np.uint64)
        w[:, 0] = self.t - 1
        w[:, 1] = 0
        w[0, self.n // 2:] = 0     # a plaintext whose upper half is zero
        return w

    def plaintext(self, words_b, ci, scale):
        """the per-object Plaintext of one item"""
        if self.scheme == "ckks":
            return S.Plaintext.from_numpy(self.ctx, words_b, parms_id=self.ctx.parms_id_at(ci), scale=scale)
        return S.Plaintext.from_numpy(self.ctx, words_b)

    def ref_plaintext(self, words_b, ci, scale):
        return self.ref.pt(words_b, ci, scale) if self.scheme == "ckks" else self.ref.pt(words_b)


def _levels(side):
    """the first data level and one lower level"""
    return [ci for ci in (side.first, side.first - 1) if ci >= 0]


def _plain_levels(side):
    return _levels(side) if side.scheme == "ckks" else [side.first]


def _sample(batch, chunks, rng, extra=6):
    picks = {0, batch - 1}
    for c in chunks:
        for e in range(c, batch, c):
            picks |= {e - 1, e}
    picks |= set(int(x) for x in rng.integers(0, batch, extra))
    return sorted(p for p in picks if 0 <= p < batch)


def _call(side, public, words, batch, ci, scale, seeds=None, destination=None):
    fn = side.enc.encrypt_device if public else side.enc.encrypt_symmetric_device
    buf = S.DeviceBuffer.from_numpy(words) if words is not None else None
    return fn(buf, batch, side.ctx.parms_id_at(ci), scale, seeds=seeds, destination=destination)


def case_reference_parity(scheme, n, bits, batch, seed=0x5EA1, sample=False, rng_seed=3):
    """symmetric and public-key, plaintext and zero, under the installed seed: every item (each with its own plaintext) carries
    the reference's bytes - words and metadata - for the same plaintext under Blake2xbPRNGFactory(seed)"""
    side = Side(scheme, n, bits, ref_seed=seed)
    ref = side.ref
    side.enc.set_seed(seed)
    rng = np.random.default_rng(rng_seed)
    scale = 2.0 ** 25
    for public in (False, True):
        for ci in _levels(side):
            items = _sample(batch, {chunk_items(n, side.K_at(ci, public))}, rng) if sample else range(batch)
            # zero: all items are the one ciphertext the reference produces
            ct = _call(side, public, None, batch, ci, scale)
            want = ref.encrypt_asymmetric_save(None, ci) if public else ref.encrypt_zero_symmetric_save(ci, False)
            for b in items:
                assert ct.save_bytes(item=b) == want, ("zero", scheme, n, public, ci, b)
            if ci not in _plain_levels(side):
                continue
            words = side.plain_words(rng, batch, ci)
            ct = _call(side, public, words, batch, ci, scale)
            for b in items:
                rpt = side.ref_plaintext(words[b], ci, scale)
                want = ref.encrypt_asymmetric_save(rpt) if public else ref.encrypt_symmetric_save(rpt, False)
                assert ct.save_bytes(item=b) == want, ("plain", scheme, n, public, ci, b)
    # the form without a parms_id works at the first data level
    ct = side.enc.encrypt_symmetric_device(None, batch, None)
    assert ct.save_bytes(item=batch - 1) == ref.encrypt_zero_symmetric_save(side.first, False)


def _per_object(side, public, words_b, ci, scale, seed_b):
    side.enc.set_seed(seed_b)
    pid = side.ctx.parms_id_at(ci)
    if words_b is None:
        ct = side.enc.encrypt_zero(pid) if public else side.enc.encrypt_zero_symmetric(pid)
    else:
        pt = side.plaintext(words_b, ci, scale)
        ct = side.enc.encrypt(pt) if public else side.enc.encrypt_symmetric(pt)
    return ct.save_bytes()


def _seeds(rng, batch):
    return rng.integers(0, 2 ** 63, (batch, 8), dtype=np.uint64)


def case_per_item_seeds(scheme, n, bits, batch, sample=False, rng_seed=7, side=None, levels=None):
    """distinct seeds[b]: item b equals the per-object call after set_seed(seeds[b]), byte for byte through save_bytes(item=b);
    an installed seed is ignored when seeds are given and is still installed afterwards"""
    side = side or Side(scheme, n, bits)
    rng = np.random.default_rng(rng_seed)
    scale = 2.0 ** 25
    for public in (False, True):
        for ci in (levels if levels is not None else _levels(side)):
            items = _sample(batch, {chunk_items(n, side.K_at(ci, public))}, rng) if sample else range(batch)
            for with_plain in (False, True):
                if with_plain and ci not in _plain_levels(side):
                    continue
                words = side.plain_words(rng, batch, ci) if with_plain else None
                seeds = _seeds(rng, batch)
                side.enc.set_seed(12345)
                ct = _call(side, public, words, batch, ci, scale, seeds=seeds)
                for b in items:
                    want = _per_object(side, public, words[b] if with_plain else None, ci, scale, seeds[b])
                    assert ct.save_bytes(item=b) == want, ("per-item seed", scheme, n, public, ci, with_plain, b)
    # `batch` ints = the first words of the seeds
    ct = side.enc.encrypt_symmetric_device(None, batch, None, seeds=list(range(100, 100 + batch)))
    assert ct.save_bytes(item=batch - 1) == _per_object(side, False, None, side.first, scale, 100 + batch - 1)


def case_fresh_entropy(scheme, n, bits, batch, rng_seed=19):
    """seeds=None and no installed seed: the c1 planes of all items differ pairwise and every item decrypts correctly - BFV / BGV
    exactly, CKKS within the tolerance of ckks_batch_cases.case_round_trip"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(rng_seed)
    side.enc.set_seed(None)
    ci, pid = side.first, side.ctx.first_parms_id()
    K, slots = side.K(ci), n // 2
    for public in (False, True):
        if scheme == "ckks":
            ce = S.CKKSEncoder(side.ctx)
            scale = 2.0 ** min(40, sum(bits[: ci + 1]) - 20)
            x = rng.standard_normal((batch, slots)) * 4
            buf = ce.encode_device(S.DeviceBuffer.from_array(x), batch, pid, scale)
            fn = side.enc.encrypt_device if public else side.enc.encrypt_symmetric_device
            ct = fn(buf, batch, pid, scale)
            assert ct.scale() == scale and ct.is_ntt_form() and ct.parms_id() == pid
            coeffs, _ = side.dec.decrypt_batch(ct)
            got = ce.decode_device(coeffs, batch, pid, scale).to_array((batch, slots))
            tol = 2.0 ** 12 / scale * np.sqrt(n)
            assert np.max(np.abs(got - x)) < tol, (public, np.max(np.abs(got - x)), tol)
        else:
            words = side.plain_words(rng, batch, ci)
            ct = _call(side, public, words, batch, ci, 1.0)
            coeffs, count = side.dec.decrypt_batch(ct)
            assert np.array_equal(coeffs.to_numpy((batch, n)), words), ("decrypt_batch", scheme, public)
        c1 = ct.to_numpy()[1].reshape(batch, -1)
        for a in range(batch):
            for b in range(a + 1, batch):
                assert not np.array_equal(c1[a], c1[b]), ("c1 of two items is the same", a, b)


def case_host_sampling_equals_device(scheme, n, bits, batch, monkeypatch):
    """SEALHIP_ENCRYPT_HOST_SAMPLING=1 (the samplers' host branch, per item) gives the words of the device samplers.  The chain has
    60-bit primes, yet rejected uniform words stay rare: the generated primes lie just below 2^60, so 2^64 mod q is tiny and a
    word is rejected with probability about 2^-40, not 2^-5.  The replacement walk (xof.cpp, shared with the per-object forms and
    unchanged) is therefore not asserted to run here: the comparisons with the reference and the per-object forms stand alone."""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(23)
    scale = 2.0 ** 25
    ci = side.first
    seeds = _seeds(rng, batch)
    words = side.plain_words(rng, batch, ci)
    for public in (False, True):
        before = S.xof_stats()
        dev = _call(side, public, words, batch, ci, scale, seeds=seeds).to_numpy()
        after = S.xof_stats()
        if not public:
            assert after[0] - before[0] == batch, "one uniform polynomial per item"
            assert after[1] >= before[1]
        monkeypatch.setenv("SEALHIP_ENCRYPT_HOST_SAMPLING", "1")
        host = _call(side, public, words, batch, ci, scale, seeds=seeds).to_numpy()
        monkeypatch.delenv("SEALHIP_ENCRYPT_HOST_SAMPLING")
        assert np.array_equal(dev, host), (scheme, n, public)


def case_chunks(scheme, n, bits, batch, per_chunk, monkeypatch, with_ref=False):
    """a scratch cap that makes chunks of `per_chunk` items (development builds: SEALHIP_ENCRYPT_SCRATCH_BYTES for the Encryptor's
    own chunks, SEALHIP_PLAIN_SCRATCH_BYTES for the Evaluator's plaintext addition after a public-key encryption, at the first
    level): every item on both sides of every chunk edge equals the per-object form - or, with_ref, carries the reference's bytes
    (the per-object forms are the same code at batch one: only the reference checks the arithmetic)"""
    side = Side(scheme, n, bits)
    K_top = side.K_at(side.first, True)
    monkeypatch.setenv("SEALHIP_ENCRYPT_SCRATCH_BYTES", str(per_chunk * 8 * K_top * n))
    monkeypatch.setenv("SEALHIP_PLAIN_SCRATCH_BYTES", str(per_chunk * 8 * side.K(side.first) * n))
    assert (batch - 1) // per_chunk >= 2, "at least two chunk edges"
    if with_ref:
        case_reference_parity(scheme, n, bits, batch)
    else:
        case_per_item_seeds(scheme, n, bits, batch, side=side, levels=[side.first])


def _expect(exc, call, what):
    try:
        call()
    except exc:
        return
    raise AssertionError("expected %s: %s" % (exc.__name__, what))


def case_errors(scheme, n, bits, batch=3):
    """the per-object forms' HRESULTs; a failed argument check leaves the destination untouched; a valid call afterwards works"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, pid = side.first, side.ctx.first_parms_id()
    scale = 2.0 ** 25
    words = side.plain_words(rng, batch, ci)
    buf = S.DeviceBuffer.from_numpy(words)
    seeds = _seeds(rng, batch)
    good = side.enc.encrypt_symmetric_device(buf, batch, pid, scale, seeds=seeds)
    snapshot, meta = good.to_numpy(), (good.parms_id(), good.scale(), good.is_ntt_form())
    only_sk = S.Encryptor(side.ctx, side.sk)
    only_pk = S.Encryptor(side.ctx, public_key=side.pk)
    other = Side(scheme, n, bits)
    for fn, keyless in ((side.enc.encrypt_symmetric_device, only_pk.encrypt_symmetric_device), (side.enc.encrypt_device, only_sk.encrypt_device)):
        _expect(S.InvalidArgument, lambda: fn(buf, batch, pid, scale, destination=S.Ciphertext(side.ctx, batch=batch + 1)), "wrong destination batch")
        _expect(S.InvalidArgument, lambda: fn(buf, batch - 1, pid, scale, destination=good), "wrong destination batch")
        _expect(S.LogicError, lambda: keyless(buf, batch, pid, scale, destination=good), "missing key")
        _expect(S.InvalidArgument, lambda: fn(buf, batch, (1, 2, 3, 4), scale, destination=good), "unknown parms_id")
        _expect(S.InvalidArgument, lambda: fn(None, batch, (1, 2, 3, 4), scale, destination=good), "unknown parms_id (zero)")
        _expect(S.InvalidArgument, lambda: fn(buf, batch, pid, scale, destination=S.Ciphertext(other.ctx, batch=batch)), "foreign destination")
        if scheme == "ckks":
            _expect(S.InvalidArgument, lambda: fn(buf, batch, side.ctx.key_parms_id(), scale, destination=good), "CKKS level above first")
            _expect(S.InvalidArgument, lambda: fn(buf, batch, pid, 0.0, destination=good), "scale")
        elif ci > 0:
            _expect(S.InvalidArgument, lambda: fn(buf, batch, side.ctx.parms_id_at(ci - 1), scale, destination=good), "BFV / BGV below the first level")
        # device_plain inside the destination's slab
        ptr, total = good.device_ptr()
        lib = S._native.lib()
        cfn = lib.Encryptor_EncryptDevice if fn == side.enc.encrypt_device else lib.Encryptor_EncryptSymmetricDevice
        p = (C.c_uint64 * 4)(*pid)
        hr = cfn(side.enc._h, C.c_void_p(ptr + 16), C.c_uint64(batch), p, C.c_double(scale), None, good._h)
        assert hr & 0xFFFFFFFF == S._native.E_INVALIDARG, "overlapping buffers"
        assert cfn(None, C.c_void_p(buf.ptr), C.c_uint64(batch), p, C.c_double(scale), None, good._h) & 0xFFFFFFFF == S._native.E_POINTER
        assert cfn(side.enc._h, C.c_void_p(buf.ptr), C.c_uint64(batch), p, C.c_double(scale), None, None) & 0xFFFFFFFF == S._native.E_POINTER
        # batch 0 does nothing
        fn(buf, 0, pid, scale, destination=good)
        assert np.array_equal(good.to_numpy(), snapshot) and (good.parms_id(), good.scale(), good.is_ntt_form()) == meta, \
            "a failed argument check must leave the destination untouched"
    again = side.enc.encrypt_symmetric_device(buf, batch, pid, scale, seeds=seeds, destination=good)
    assert again is good and np.array_equal(good.to_numpy(), snapshot), "a valid call after the failures"


def case_pipeline(n, bits, batch, seed=11):
    """ckks_batch_cases.case_client_loop without the per-item loop: encode_device -> encrypt_symmetric_device -> multiply /
    relinearize / rescale -> decrypt_batch -> decode_device: every item equals the reference's decrypt + decode of the same saved
    item bit for bit, and a*b approximately"""
    side = Side("ckks", n, bits, ref_seed=0x5EA1)
    ref, d = side.ref, side.d
    enc = S.CKKSEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    ref.keygen_relin()
    rlk = S.RelinKeys(side.ctx)
    rlk.load_bytes(ref.keys_save("relin", True))
    pid, slots = side.ctx.first_parms_id(), n // 2
    scale = 2.0 ** (bits[-2] if len(bits) > 2 else 12)
    a, b = rng.standard_normal((batch, slots)), rng.standard_normal((batch, slots))
    wa = enc.encode_device(S.DeviceBuffer.from_array(a), batch, pid, scale)
    wb = enc.encode_device(S.DeviceBuffer.from_array(b), batch, pid, scale)
    side.enc.set_seed(None)
    A = side.enc.encrypt_symmetric_device(wa, batch, pid, scale)
    B = side.enc.encrypt_symmetric_device(wb, batch, pid, scale)
    d.ev.multiply_inplace(A, B)
    d.ev.relinearize_inplace(A, rlk)
    if len(side.primes) > 2:
        d.ev.rescale_to_next_inplace(A)
    coeffs, _ = side.dec.decrypt_batch(A)
    pid2, scale2 = A.parms_id(), A.scale()
    for want_c in (False, True):
        got = enc.decode_device(coeffs, batch, pid2, scale2, complex_values=want_c)
        got = got.to_array((batch, slots), np.complex128 if want_c else np.float64)
        for k in range(batch):
            rct, _ = ref.ct_load(A.save_bytes(item=k))
            want = ref.ckks_decode(ref.decrypt(rct), want_c)
            assert got[k].tobytes() == want.tobytes(), ("pipeline", k, want_c)
            err = np.max(np.abs(got[k].real - a[k] * b[k]))
            assert err < 1e-2, ("a*b", k, err)
