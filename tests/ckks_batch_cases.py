"""Batched CKKS encoding in device memory (CKKSEncoder_EncodeDevice / CKKSEncoder_DecodeDevice), shared by the CPU (emulated
kernels) and `-m gpu` suites.  Every item of a batch is checked against the REAL reference (oracle/_ref): encode gives the
words of seal::CKKSEncoder::encode word for word, decode the doubles of seal::CKKSEncoder::decode bit for bit.
TEST INFRASTRUCTURE: the reference is the checker."""
import numpy as np

import seal_amd as S
import sealref
from decrypt_cases import _setup

SCRATCH_BYTES = 256 << 20   # include/sealhip.h: the chunks' scratch cap
LDS_LOG = 12                # one LDS block of 2^12 complex values: larger N take two passes


def chunk_items(n, K, decode):
    """items per chunk, as include/sealhip.h states it: scratch of a two-pass transform = N complex values per item, plus the
    copy of the K*N words for decode"""
    two_pass = n > (1 << LDS_LOG)
    per = (2 * n if two_pass else 0) + (K * n if decode else 0)
    return max(1, SCRATCH_BYTES // (8 * per)) if per else None


def _scales(bits, ci):
    total = sum(bits[: ci + 1])
    scales = [2.0 ** 30, 2.0 ** 20]
    if sum(bits[:-1]) > 100:
        scales.append(2.0 ** 80)
    if sum(bits[:-1]) > 180:
        scales += [2.0 ** 150, 2.0 ** 131.5]
    return [s for s in scales if np.log2(s) + 8 < total]


def _items(rng, ref, batch, count, cplx, ci, scale, total_bits):
    """`batch` vectors whose coefficients land in very different widths (below 64 bits, 64-128, above 128 where the level
    allows it), each shrunk until the reference accepts it -> (values [batch][count](complex), reference plaintexts)"""
    targets = [30, 96, 160, 45, 100, 20, 150]    # bits of the largest coefficient, roughly
    vals, rpts = [], []
    for b in range(batch):
        t = min(targets[b % len(targets)], total_bits - 6)
        mag = 2.0 ** t / _gain(ref.n, count, scale)
        v = rng.standard_normal(count) * mag
        if cplx:
            v = v + 1j * rng.standard_normal(count) * mag
        for _ in range(40):
            try:
                rpt = ref.ckks_encode_complex(v, ci, scale) if cplx else ref.ckks_encode(v, ci, scale)
                break
            except sealref.RefError:
                v = v / 2.0 ** 8
        else:
            raise AssertionError("no accepted magnitude for item %d" % b)
        vals.append(v)
        rpts.append(rpt)
    dtype = np.complex128 if cplx else np.float64
    return np.array(vals, dtype=dtype).reshape(batch, count), rpts


def _sample(batch, chunks, rng, extra=8):
    """first, last, the items on both sides of every chunk edge and about `extra` random ones"""
    picks = {0, batch - 1}
    for c in chunks:
        if c:
            for e in range(c, batch, c):
                picks |= {e - 1, e}
    picks |= set(int(x) for x in rng.integers(0, batch, extra))
    return sorted(p for p in picks if 0 <= p < batch)


def case_encode_decode_parity(n, bits, batch, sample=False, counts=None, levels=None, scales=None, seed=5):
    """encode parity at every level, with 64-bit / 128-bit / multi-precision coefficients mixed in one batch, real and complex,
    full, short and empty vectors; decode parity on those words, real and complex output"""
    primes, t, ref, d, dec, _ = _setup("ckks", n, bits)
    enc = S.CKKSEncoder(d.ctx)
    rng = np.random.default_rng(seed)
    slots = n // 2
    counts = counts if counts is not None else (slots, min(5, slots), 0)
    levels = levels if levels is not None else range(ref.first_chain_index, -1, -1)
    widths = set()
    for ci in levels:
        pid, K, total = d.ctx.parms_id_at(ci), ci + 1, sum(bits[: ci + 1])
        items = _sample(batch, (chunk_items(n, K, False), chunk_items(n, K, True)), rng) if sample else range(batch)
        for scale in _scales(bits, ci):
            if scales is not None and scale not in scales:
                continue
            for cplx in (False, True):
                for count in counts:
                    vals, rpts = _items(rng, ref, batch, count, cplx, ci, scale, total)
                    out = enc.encode_device(S.DeviceBuffer.from_array(vals), batch, pid, scale, complex_values=cplx, count=count)
                    words = out.to_numpy((batch, K, n))
                    for b in items:
                        assert np.array_equal(words[b].reshape(-1), rpts[b].data()), ("encode", n, ci, scale, cplx, count, b)
                        widths.add(_width(n, vals[b], scale))
                    for want_c in (False, True):
                        got = enc.decode_device(out, batch, pid, scale, complex_values=want_c)
                        got = got.to_array((batch, slots), np.complex128 if want_c else np.float64)
                        for b in items:
                            want = ref.ckks_decode(rpts[b], want_c)
                            assert got[b].tobytes() == want.tobytes(), ("decode", n, ci, scale, cplx, count, b, want_c)
    return widths


def _gain(n, count, scale):
    """about the largest |coefficient| per unit of slot magnitude: scale / N times a random walk over the 2 count placed values"""
    return scale * 4.0 * np.sqrt(2.0 * max(count, 1)) / n


def _width(n, vals, scale):
    """the decomposition width an item's largest coefficient needs, estimated with a wide margin: 64, 128, 0 (multi-precision),
    or None near a boundary"""
    if not vals.size:
        return 64
    est = np.log2(np.max(np.abs(vals)) * _gain(n, vals.size, scale))
    return 64 if est < 52 else 128 if 76 < est < 116 else 0 if est > 140 else None


def case_decode_random_words(n, bits, batch, seed=9):
    """decode of arbitrary residues (0 and q - 1 included) at every level equals the reference's decode of the same plaintext"""
    primes, t, ref, d, dec, _ = _setup("ckks", n, bits)
    enc = S.CKKSEncoder(d.ctx)
    rng = np.random.default_rng(seed)
    for ci in range(ref.first_chain_index, -1, -1):
        pid, K = d.ctx.parms_id_at(ci), ci + 1
        scale = 2.0 ** 20
        q = np.array(primes[:K], dtype=np.uint64)
        words = (rng.integers(0, 2 ** 63, (batch, K, n), dtype=np.uint64) % q[None, :, None]).astype(np.uint64)
        words[:, :, 0] = 0
        words[:, :, 1] = q - 1
        words[0, :, 2:7] = 0
        words[-1, :, 2:7] = (q - 1)[:, None]
        buf = S.DeviceBuffer.from_numpy(words)
        for want_c in (False, True):
            got = enc.decode_device(buf, batch, pid, scale, complex_values=want_c)
            got = got.to_array((batch, n // 2), np.complex128 if want_c else np.float64)
            for b in range(batch):
                want = ref.ckks_decode(ref.pt(words[b], ci, scale), want_c)
                assert got[b].tobytes() == want.tobytes(), ("decode random", ci, b, want_c)
        assert np.array_equal(buf.to_numpy((batch, K, n)), words), "decode_device must not modify its input"


def case_errors(n, bits, batch=5):
    """argument checks and per-item value checks; a valid call after a failed one still gives the reference's words"""
    primes, t, ref, d, dec, _ = _setup("ckks", n, bits)
    enc = S.CKKSEncoder(d.ctx)
    rng = np.random.default_rng(3)
    ci = ref.first_chain_index
    pid, K, slots = d.ctx.parms_id_at(ci), ci + 1, n // 2
    scale = 2.0 ** 20
    vals = rng.standard_normal((batch, slots))
    mid = batch // 2
    bad = vals.copy()
    bad[mid, 3] = np.nan
    out = S.DeviceBuffer(batch * K * n)
    try:
        enc.encode_device(S.DeviceBuffer.from_array(bad), batch, pid, scale, out=out)
        raise AssertionError("a NaN item was accepted")
    except S.InvalidArgument as e:
        assert "item %d" % mid in str(e), str(e)
    inf = vals.copy()
    inf[batch - 1, 0] = np.inf
    for arr in (inf, vals * 1e300):
        try:
            enc.encode_device(S.DeviceBuffer.from_array(arr), batch, pid, 2.0 ** 40, out=out)
            raise AssertionError("expected InvalidArgument")
        except S.InvalidArgument:
            pass
    # a coefficient too large for the level, in one item only (the reference's "encoded values are too large")
    big = vals.copy()
    big[1] *= 2.0 ** sum(bits[: ci + 1])
    try:
        ref.ckks_encode(big[1], ci, scale)
        raise AssertionError("the reference accepted the oversized item")
    except sealref.RefError:
        pass
    try:
        enc.encode_device(S.DeviceBuffer.from_array(big), batch, pid, scale, out=out)
        raise AssertionError("an oversized item was accepted")
    except S.InvalidArgument as e:
        assert "item 1" in str(e), str(e)
    good = S.DeviceBuffer.from_array(vals)
    words = S.DeviceBuffer(batch * K * n)
    dvals = S.DeviceBuffer(batch * slots * 2)
    for bad_call in (lambda: enc.encode_device(good, 1, pid, scale, count=slots + 1, out=words),
                     lambda: enc.encode_device(good, batch, (1, 2, 3, 4), scale, out=words),
                     lambda: enc.encode_device(good, batch, pid, 0.0, out=words),
                     lambda: enc.encode_device(good, batch, pid, float("inf"), out=words),
                     lambda: enc.encode_device(good, batch, pid, scale, out=good),                  # input and output overlap
                     lambda: enc.decode_device(words, batch, (1, 2, 3, 4), scale, out=dvals),
                     lambda: enc.decode_device(words, batch, d.ctx.key_parms_id(), scale, out=dvals),   # above the data levels
                     lambda: enc.decode_device(words, batch, pid, 0.0, out=dvals),
                     lambda: enc.decode_device(words, batch, pid, float("inf"), out=dvals),
                     lambda: enc.decode_device(words, batch, pid, scale, out=words)):               # input and output overlap
        try:
            bad_call()
            raise AssertionError("expected InvalidArgument")
        except S.InvalidArgument:
            pass
    lib = S._native.lib()
    import ctypes as C
    p = (C.c_uint64 * 4)(*pid)
    assert lib.CKKSEncoder_EncodeDevice(enc._h, None, C.c_uint64(slots), C.c_uint64(batch), C.c_bool(False), p, C.c_double(scale),
                                        C.c_void_p(words.ptr)) & 0xFFFFFFFF == S._native.E_INVALIDARG
    assert lib.CKKSEncoder_EncodeDevice(enc._h, C.c_void_p(good.ptr), C.c_uint64(slots), C.c_uint64(batch), C.c_bool(False), p,
                                        C.c_double(scale), None) & 0xFFFFFFFF == S._native.E_INVALIDARG
    assert lib.CKKSEncoder_DecodeDevice(enc._h, None, C.c_uint64(batch), p, C.c_double(scale), C.c_bool(False),
                                        C.c_void_p(dvals.ptr)) & 0xFFFFFFFF == S._native.E_INVALIDARG
    assert lib.CKKSEncoder_DecodeDevice(enc._h, C.c_void_p(words.ptr), C.c_uint64(batch), p, C.c_double(scale), C.c_bool(False),
                                        None) & 0xFFFFFFFF == S._native.E_INVALIDARG
    # batch 0 does nothing
    enc.encode_device(good, 0, pid, scale, count=slots, out=words)
    enc.decode_device(words, 0, pid, scale, out=dvals)
    # a valid call after the failures
    enc.encode_device(good, batch, pid, scale, out=words)
    got = words.to_numpy((batch, K * n))
    for b in range(batch):
        assert np.array_equal(got[b], ref.ckks_encode(vals[b], ci, scale).data()), ("after a failure", b)


def case_client_loop(n, bits, batch, seed=11):
    """encode_device -> per item Plaintext.set_from_device + secret-key encryption -> one ciphertext batch -> multiply /
    relinearize / rescale -> decrypt_batch -> decode_device: every item equals the reference's decrypt + decode of the same
    saved item bit for bit, and a*b approximately"""
    primes, t, ref, d, dec, _ = _setup("ckks", n, bits)
    enc = S.CKKSEncoder(d.ctx)
    rng = np.random.default_rng(seed)
    ref.keygen_relin()
    e = S.Encryptor(d.ctx, S.SecretKey(d.ctx, ref.secret_key()))
    rlk = S.RelinKeys(d.ctx)
    rlk.load_bytes(ref.keys_save("relin", True))
    ci = ref.first_chain_index
    pid, K, slots = d.ctx.parms_id_at(ci), ci + 1, n // 2
    scale = 2.0 ** (bits[-2] if len(bits) > 2 else 12)
    a, b = rng.standard_normal((batch, slots)), rng.standard_normal((batch, slots))
    wa = enc.encode_device(S.DeviceBuffer.from_array(a), batch, pid, scale)
    wb = enc.encode_device(S.DeviceBuffer.from_array(b), batch, pid, scale)
    A, B = S.Ciphertext(d.ctx, batch=batch), S.Ciphertext(d.ctx, batch=batch)
    for k in range(batch):
        for words, ct in ((wa, A), (wb, B)):
            pt = S.Plaintext(d.ctx).set_from_device(words, K * n, offset=k * K * n, parms_id=pid, scale=scale)
            assert pt.is_ntt_form() and pt.parms_id() == pid and pt.scale() == scale
            ct.load_bytes(e.encrypt_symmetric(pt).save_bytes(), item=k)
    d.ev.multiply_inplace(A, B)
    d.ev.relinearize_inplace(A, rlk)
    if len(primes) > 2:
        d.ev.rescale_to_next_inplace(A)
    coeffs, _ = dec.decrypt_batch(A)
    pid2, scale2 = A.parms_id(), A.scale()
    for want_c in (False, True):
        got = enc.decode_device(coeffs, batch, pid2, scale2, complex_values=want_c)
        got = got.to_array((batch, slots), np.complex128 if want_c else np.float64)
        for k in range(batch):
            rct, _ = ref.ct_load(A.save_bytes(item=k))
            want = ref.ckks_decode(ref.decrypt(rct), want_c)
            assert got[k].tobytes() == want.tobytes(), ("client loop", k, want_c)
            err = np.max(np.abs(got[k].real - a[k] * b[k]))
            assert err < 1e-2, ("a*b", k, err)


def case_round_trip(n, bits, batch, seed=13):
    """decode_device(encode_device(x)) = x within CKKS precision, real and complex"""
    primes, t, ref, d, dec, _ = _setup("ckks", n, bits)
    enc = S.CKKSEncoder(d.ctx)
    rng = np.random.default_rng(seed)
    ci = ref.first_chain_index
    pid, slots, scale = d.ctx.parms_id_at(ci), n // 2, 2.0 ** min(40, sum(bits[: ci + 1]) - 20)
    x = rng.standard_normal((batch, slots)) * 4
    got = enc.decode_device(enc.encode_device(S.DeviceBuffer.from_array(x), batch, pid, scale), batch, pid, scale).to_array((batch, slots))
    tol = 2.0 ** 12 / scale * np.sqrt(n)
    assert np.max(np.abs(got - x)) < tol, np.max(np.abs(got - x))
    z = x + 1j * rng.standard_normal((batch, slots))
    w = enc.encode_device(S.DeviceBuffer.from_array(z), batch, pid, scale, complex_values=True)
    got = enc.decode_device(w, batch, pid, scale, complex_values=True).to_array((batch, slots), np.complex128)
    assert np.max(np.abs(got - z)) < tol, np.max(np.abs(got - z))


def case_batch_of_one(n, bits, seed=17):
    """batch = 1 gives the words of the per-object encode and the doubles of the per-object decode"""
    primes, t, ref, d, dec, _ = _setup("ckks", n, bits)
    enc = S.CKKSEncoder(d.ctx)
    rng = np.random.default_rng(seed)
    ci = ref.first_chain_index
    pid, K, slots, scale = d.ctx.parms_id_at(ci), ci + 1, n // 2, 2.0 ** min(30, sum(bits[: ci + 1]) - 10)
    short = min(7, slots - 1)
    for v in (rng.standard_normal(slots), rng.standard_normal(short) + 1j * rng.standard_normal(short)):
        cplx = np.iscomplexobj(v)
        pt = enc.encode(v, pid, scale)
        w = enc.encode_device(S.DeviceBuffer.from_array(v), 1, pid, scale, complex_values=cplx)
        assert np.array_equal(w.to_numpy(K * n), pt.to_numpy())
        for want_c in (False, True):
            got = enc.decode_device(w, 1, pid, scale, complex_values=want_c).to_array(slots, np.complex128 if want_c else np.float64)
            assert got.tobytes() == enc.decode(pt, want_c).tobytes()
