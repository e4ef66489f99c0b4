"""A dense matrix of scalar plaintexts times a batch (CKKSEncoder_EncodeScalars / _EncodeIntegerScalars, Evaluator_LiftScalars,
Evaluator_DotScalarsDevice; shl_dot_scalars), shared by the CPU (emulated kernels) and `-m gpu` suites.  Exact word equality
everywhere.  Three yardsticks for the product: Evaluator_DotPlainMapped over the dense map with every scalar expanded to a full
[K][N] plaintext; the library's unchanged per-object forms on batches of one (Encode3 / the transformed constant plaintext,
multiply_plain_inplace, add_many); and, where oracle/_ref is built, the REAL reference doing the same on its own objects.  The
flush-boundary and cut cases compare with Python-integer arithmetic, which depends on neither library.  Row counts are written in
terms of the row tile R the library reports, so that they follow a change of R.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import sealref
import batch_reduce_cases as BR
from harness import two_pass_ring
from batch_reduce_cases import meta, _columns, DOT_FLUSH
from plain_batch_cases import Side, _expect

BATCH = 7
FLUSH_BATCHES = [1, DOT_FLUSH - 1, DOT_FLUSH, DOT_FLUSH + 1, 2 * DOT_FLUSH + 3]


def info():
    """(row tile R, items between two reductions) as the library reports them"""
    r, f = C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_dot_scalars_info(C.byref(r), C.byref(f)))
    return r.value, f.value


def row_counts():
    """a lone row, a short tile, a full tile, a full tile and a lone row, two full tiles and a lone row"""
    R, _ = info()
    return sorted({1, R - 1, R, R + 1, 2 * R + 1} - {0})


def threads(size, rows, K, n):
    """include/sealhip.h: one thread per coefficient pair of a plane, a prime and a TILE of R rows"""
    R, _ = info()
    return size * -(-rows // R) * K * n // 2


# ---- scalars
def scalar_values(side, rng, rows, batch):
    """[rows][batch] host values among random ones: a zero, and (CKKS) a negative one and one that rounds to zero, (BFV / BGV) t - 1
    and the upper-half threshold.  No row is all zeros: add_many of nothing throws in the reference"""
    assert batch >= 2
    if side.scheme == "ckks":
        v = rng.standard_normal((rows, batch)) * 8
        v[0, 0], v[-1, 0], v[-1, -1] = 0.0, 1e-9, -3.0
        return v
    v = rng.integers(1, side.t, (rows, batch), dtype=np.uint64)
    v[0, 0], v[-1, 0], v[-1, -1] = 0, (side.t + 1) // 2, side.t - 1
    return v


def make_scalars(side, values, ci):
    """the public producers -> (DeviceBuffer [rows][batch][K], the same words on the host)"""
    pid, K = side.ctx.parms_id_at(ci), len(side.ctx.coeff_modulus_at(ci))
    if side.scheme == "ckks":
        buf = S.CKKSEncoder(side.ctx).encode_scalars(values, pid, side.scale)
    else:
        buf = side.ev.lift_scalars(values, pid)
    return buf, buf.to_numpy(values.shape + (K,))


def constant_plaintext(side, value, ci):
    """the per-object form of one scalar: Encode3, or the constant polynomial lifted and transformed at the level"""
    pid = side.ctx.parms_id_at(ci)
    if side.scheme == "ckks":
        return S.CKKSEncoder(side.ctx).encode(float(value), pid, side.scale)
    p = S.Plaintext.from_numpy(side.ctx, np.array([value], dtype=np.uint64))
    return side.ev.transform_plain_to_ntt_inplace(p, pid)


def ref_constant_plaintext(side, value, ci):
    if side.scheme == "ckks":
        return side.ref.ckks_encode_value(float(value), ci, side.scale)
    return side.ref.pt_transform_to_ntt_inplace(side.ref.pt(np.array([value], dtype=np.uint64)), ci)


def expect_row(side, x, values_o, ci):
    """x [size][B][K][N], values_o [B]: multiply_plain_inplace with the constant plaintext per item on batches of one, then add_many
    -> (words [size][K][N], metadata); the reference, where it is built, must say the same"""
    cts = [side.dev_ct(x[:, b:b + 1], ci, True) for b in range(x.shape[1])]
    for b, c in enumerate(cts):
        side.ev.multiply_plain_inplace(c, constant_plaintext(side, values_o[b], ci))
    out = side.ev.add_many(cts, S.Ciphertext(side.ctx))
    words, m = out.to_numpy()[:, 0], meta(out)
    if side.ref is not None:
        rs = []
        for b in range(x.shape[1]):
            r = side.ref.ct(ci, x[:, b], True, side.scale, side.cf)
            try:
                rs.append(side.ref.multiply_plain_inplace(r, ref_constant_plaintext(side, values_o[b], ci)))
            except sealref.RefError:
                # the reference is built with SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT: the product with a scalar that encodes to zero
                # is refused there; it is the zero ciphertext and adds nothing
                assert side.scheme != "ckks" and values_o[b] == 0 or side.scheme == "ckks" and round(values_o[b] * side.scale) == 0
        r = side.ref.add_many(rs)
        i = r.info()
        assert np.array_equal(words, r.data()), "per-object forms and reference disagree"
        assert m == (i["is_ntt_form"], i["scale"], i["correction_factor"])
    return words, m


def dense_map(side, rows, batch):
    return S.ItemMap(side.ctx, [list(range(batch))] * rows, batch, second=[list(range(o * batch, (o + 1) * batch)) for o in range(rows)],
                     second_batch=rows * batch)


def expand(words, n):
    """[rows][B][K] scalars -> [rows * B][K][N] plaintexts, each filled with its scalar's K words"""
    rows, batch, K = words.shape
    return np.ascontiguousarray(np.broadcast_to(words.reshape(rows * batch, K, 1), (rows * batch, K, n)))


def via_dense_map(side, c, words, rows, scale=None):
    pl = S.DeviceBuffer.from_numpy(expand(words[:rows], side.n))
    return side.ev.dot_plain_mapped(c, pl, rows * words.shape[1], dense_map(side, rows, words.shape[1]), side.scale if scale is None else scale)


# ---- parity
def case_parity(scheme, n, bits, sizes=(2, 3), ci=None, batch=BATCH, rows_list=None, seed=5):
    """every row count: the words and metadata of DotPlainMapped over the dense map with expanded plaintexts, of the per-object
    composition and of the reference.  The yardsticks are formed once, for the largest row count: fewer rows are a prefix of
    [rows][B][K]"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    rows_list = row_counts() if rows_list is None else rows_list
    most = max(rows_list)
    for size in sizes:
        x = side.rand_ct(rng, ci, batch, size)
        values = scalar_values(side, rng, most, batch)
        buf, words = make_scalars(side, values, ci)
        want = [expect_row(side, x, values[o], ci) for o in range(most)]
        c = side.dev_ct(x, ci, True)
        for rows in rows_list:
            out = side.ev.dot_scalars_device(c, buf, rows, side.scale)
            got = out.to_numpy()
            assert got.shape == (size, rows) + x.shape[2:], (scheme, n, size, rows, got.shape)
            assert (out.batch(), out.size(), out.parms_id()) == (rows, size, side.ctx.parms_id_at(ci))
            mapped = via_dense_map(side, c, words, rows)
            assert np.array_equal(got, mapped.to_numpy()) and meta(out) == meta(mapped), ("dense map", scheme, n, size, rows)
            for o in range(rows):
                assert np.array_equal(got[:, o], want[o][0]), ("per-object forms", scheme, n, size, rows, "output item", o)
                assert meta(out) == want[o][1], ("metadata", scheme, n, size, rows)
        assert np.array_equal(c.to_numpy(), x), "the operand is only read"


# ---- encoders
def _prefilled(words):
    return S.DeviceBuffer.from_numpy(np.full(words, 0xA5A5A5A5, dtype=np.uint64))


def case_encode_scalars(n=1024, bits=(60, 60, 60, 60)):
    """encode_scalars against Encode3 at coefficients 0 and N - 1 of every prime, one value per branch of the reference: at most 64
    bits, 65 .. 128 bits, more than 128 bits (the first level has 180), negative, zero, below one after scaling; the refusals carry
    the per-object form's message and the index and leave the buffer unchanged"""
    side = Side("ckks", n, list(bits))
    enc = S.CKKSEncoder(side.ctx)
    scale = 2.0 ** 30
    values = [3.5, 1.7 * 2.0 ** 40, 1.3 * 2.0 ** 110, -2.25 * 2.0 ** 50, -1.1 * 2.0 ** 120, 0.0, 1e-12, -1e-12, -7.0, 2.0 ** 34 - 2.0 ** -30]
    bit_counts = [2 if abs(v * scale) < 1 else int(np.log2(abs(v * scale))) + 2 for v in values]
    assert bit_counts[0] <= 64 and 64 < bit_counts[1] <= 128 and bit_counts[2] > 128 and bit_counts[4] > 128
    for ci in (side.first, 0):
        pid, q = side.ctx.parms_id_at(ci), side.ctx.coeff_modulus_at(ci)
        K = len(q)
        ok = [v for v, b in zip(values, bit_counts) if b < sum(int(p).bit_length() for p in q)]
        assert ci != side.first or len(ok) == len(values), "the first level admits every branch"
        got = enc.encode_scalars(ok, pid, scale).to_numpy((len(ok), K))
        for i, v in enumerate(ok):
            p = enc.encode(float(v), pid, scale).to_numpy().reshape(K, n)
            assert np.array_equal(p[:, 0], got[i]) and np.array_equal(p[:, n - 1], got[i]), ("encode_scalars", ci, v)
            if side.ref is not None:
                assert np.array_equal(side.ref.ckks_encode_value(float(v), ci, scale).data().reshape(K, n)[:, 0], got[i]), ("reference", ci, v)
        assert not np.any(got[ok.index(0.0)]) and not np.any(got[ok.index(1e-12)])
        # refusals: the per-object message, the first failing index, nothing written
        for bad, where in ((float("nan"), 2), (float("inf"), 0), (2.0 ** 1000, 1), (2.0 ** 200, 3)):
            try:
                enc.encode(bad, pid, scale)
                raise AssertionError("the per-object form accepted %r" % bad)
            except S.InvalidArgument as e:
                message = e.message
            vals = [1.0, 2.0, 3.0, 4.0]
            vals[where] = bad
            vals[3] = bad if where < 3 else vals[3]   # a second failing value further on: the FIRST index is named
            out = _prefilled(4 * K)
            try:
                enc.encode_scalars(vals, pid, scale, out=out)
                raise AssertionError("encode_scalars accepted %r" % bad)
            except S.InvalidArgument as e:
                assert message in e.message and "values[%d]" % where in e.message, (e.message, message, where)
            assert np.all(out.to_numpy((4 * K,)) == 0xA5A5A5A5), "a failed call writes nothing"
        _expect(S.InvalidArgument, lambda: enc.encode_scalars([1.0], pid, 2.0 ** 400), "scale out of bounds")
        _expect(S.InvalidArgument, lambda: enc.encode_scalars([1.0], pid, 0.0), "scale 0")


def case_encode_integer_scalars(n=1024, bits=(60, 60, 60, 60)):
    """encode_integer_scalars against Encode5, negative values and INT64_MIN included; at K = 1 (60 bits) a 64-bit value is refused"""
    side = Side("ckks", n, list(bits))
    enc = S.CKKSEncoder(side.ctx)
    lo, hi = -2 ** 63, 2 ** 63 - 1
    values = [0, 1, -1, 12345, -(2 ** 40) - 3, 2 ** 62 + 1, lo, hi, -(2 ** 56)]
    for ci in (side.first, 0):
        pid = side.ctx.parms_id_at(ci)
        K = len(side.ctx.coeff_modulus_at(ci))
        total = sum(int(p).bit_length() for p in side.ctx.coeff_modulus_at(ci))
        ok = [v for v in values if abs(v).bit_length() + 2 < total]
        assert (lo in ok) == (ci == side.first) and -1 in ok and -(2 ** 56) in ok
        got = enc.encode_integer_scalars(ok, pid).to_numpy((len(ok), K))
        for i, v in enumerate(ok):
            p = enc.encode(int(v), pid, None).to_numpy().reshape(K, n)
            assert np.array_equal(p[:, 0], got[i]) and np.array_equal(p[:, n - 1], got[i]), ("encode_integer_scalars", ci, v)
            if side.ref is not None:
                assert np.array_equal(side.ref.ckks_encode_value(int(v), ci).data().reshape(K, n)[:, 0], got[i]), ("reference", ci, v)
        if len(ok) < len(values):
            out = _prefilled(3 * K)
            try:
                enc.encode_integer_scalars([5, lo, hi], pid, out=out)
                raise AssertionError("a 64-bit value at a 60-bit level")
            except S.InvalidArgument as e:
                assert "encoded value is too large" in e.message and "values[1]" in e.message, e.message
            assert np.all(out.to_numpy((3 * K,)) == 0xA5A5A5A5), "a failed call writes nothing"


def case_lift_scalars(scheme, n, bits, tbits, fast):
    """lift_scalars against TransformPlainToNTTDevice on the constant polynomials, below and from the upper-half threshold on, at
    the first level and the lowest: every coefficient of every prime holds the scalar's word (and the reference's transform agrees)"""
    side = Side(scheme, n, bits, tbits)
    t = side.t
    assert all(t < q for q in side.ctx.coeff_modulus_at(side.first)) == fast, "the lift branch this case is for"
    rng = np.random.default_rng(23)
    values = np.array([0, 1, (t + 1) // 2 - 1, (t + 1) // 2, t - 1, t - 2] + [int(v) for v in rng.integers(0, t, 6)], dtype=np.uint64)
    coeffs = np.zeros((values.size, n), dtype=np.uint64)
    coeffs[:, 0] = values
    for ci in (side.first, 0):
        pid, K = side.ctx.parms_id_at(ci), len(side.ctx.coeff_modulus_at(ci))
        got = side.ev.lift_scalars(values, pid).to_numpy((values.size, K))
        want = side.ev.transform_plain_to_ntt_device(S.DeviceBuffer.from_numpy(coeffs), values.size, pid).to_numpy((values.size, K, n))
        assert np.array_equal(want, np.broadcast_to(got[:, :, None], want.shape)), ("lift_scalars", scheme, ci, fast)
        if side.ref is not None:
            for i in (2, 3, 4, 7):
                rp = side.ref.pt_transform_to_ntt_inplace(side.ref.pt(coeffs[i, :1]), ci)
                assert np.array_equal(rp.data().reshape(K, n)[:, n - 1], got[i]), ("reference", scheme, ci, i)
    out = _prefilled(3 * K)
    try:
        side.ev.lift_scalars([1, t, 2], pid, out=out)
        raise AssertionError("a value >= t")
    except S.InvalidArgument as e:
        assert "values[1]" in e.message, e.message
    assert np.all(out.to_numpy((3 * K,)) == 0xA5A5A5A5), "a failed call writes nothing"


# ---- the raw seam
def raw(side, ci, x, s, slices=0):
    """shl_dot_scalars on raw words: x [size][B][K][N], s [rows][B][K] -> (words [size][rows][K][N], slices run)"""
    size, batch, K, n = x.shape
    rows = s.shape[0]
    a, w = S.DeviceBuffer.from_numpy(x), S.DeviceBuffer.from_numpy(s)
    r = S.DeviceBuffer(size * rows * K * n)
    used = C.c_uint64()
    S._native.check(S._native.lib().shl_dot_scalars(side.ctx._h, C.c_uint64(ci), C.c_void_p(a.ptr), C.c_void_p(w.ptr), C.c_void_p(r.ptr),
                                                    C.c_uint64(size), C.c_uint64(rows), C.c_uint64(batch), C.c_uint64(slices), C.byref(used)))
    if slices:
        per = -(-batch // slices)
        assert used.value == -(-batch // per), ("slices run", used.value, slices)
    return r.to_numpy((size, rows, K, n)), used.value


def raw_tile(side, ci, x, s, row_tile, slices=0):
    """shl_dot_scalars_tile: the same with a row tile of 2, 4 or 8 rows per thread (0: the library's), on the NULL stream"""
    size, batch, K, n = x.shape
    rows = s.shape[0]
    a, w = S.DeviceBuffer.from_numpy(x), S.DeviceBuffer.from_numpy(s)
    r = S.DeviceBuffer(size * rows * K * n)
    used = C.c_uint64()
    S._native.check(S._native.lib().shl_dot_scalars_tile(side.ctx._h, C.c_uint64(ci), C.c_void_p(a.ptr), C.c_void_p(w.ptr), C.c_void_p(r.ptr),
                                                         C.c_uint64(size), C.c_uint64(rows), C.c_uint64(batch), C.c_uint64(slices), C.byref(used),
                                                         C.c_uint64(row_tile), None))
    return r.to_numpy((size, rows, K, n)), used.value   # (the copy back waits for the device)


def case_tiles(n, bits, batch=23, size=2, seed=83):
    """every row tile the library is built with - the rate tool sweeps them - gives the Python integers' words: two full tiles and a
    lone row, and a short tile alone, in one launch and cut in three; a tile that is not built is refused"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    for R in (2, 4, 8):
        for rows in (2 * R + 1, R - 1):
            for pattern in ("max", "random"):
                xc = _columns(side, ci, pattern, rng, (size, batch))
                s = scalar_pattern(side, ci, pattern, rng, rows, batch)
                x = np.ascontiguousarray(np.tile(xc, n // 2))
                want = np.tile(integers(xc, s, q), n // 2)
                for slices in (1, 3):
                    got, used = raw_tile(side, ci, x, s, R, slices)
                    assert used == slices and np.array_equal(got, want), ("tile", n, R, rows, pattern, slices)
    _expect(S.InvalidArgument, lambda: raw_tile(side, ci, x, s, 3), "a row tile that is not built")


def scalar_pattern(side, ci, pattern, rng, rows, batch):
    """[rows][batch][K] words by pattern"""
    q = side.q(ci)
    qk = np.broadcast_to(q, (rows, batch, q.size))
    if pattern == "max":
        return (qk - 1).astype(np.uint64)
    if pattern == "half":
        return (qk // 2 + (np.indices(qk.shape)[1] % 2).astype(np.uint64)).astype(np.uint64)
    if pattern == "alternating":   # q - 1 and 0 in turn along the rows and along the items
        idx = np.indices(qk.shape)
        return np.where((idx[0] + idx[1]) % 2 == 0, qk - 1, 0).astype(np.uint64)
    return (rng.integers(0, 2 ** 63, qk.shape, dtype=np.uint64) % qk).astype(np.uint64)


def integers(xc, s, q):
    """Python integers: xc [size][B][K][2] columns, s [rows][B][K] -> [size][rows][K][2]"""
    xo, so = xc.astype(object), s.astype(object)
    out = np.zeros((xc.shape[0], s.shape[0], len(q), 2), dtype=np.uint64)
    for o in range(s.shape[0]):
        for k in range(len(q)):
            out[:, o, k] = ((xo[:, :, k] * so[o, :, k][None, :, None]).sum(axis=1) % q[k]).astype(np.uint64)
    return out


def case_flush(n, bits, batches=None, patterns=("max", "alternating", "half", "random"), size=2, seed=61, row_tile=None):
    """B around the flush interval, R + 1 rows (a full tile and a short one), one launch: every word equals the sum formed with
    Python integers.  With "max" every ciphertext word and every scalar is q - 1: the largest run the accumulators must hold.
    row_tile: that built tile through shl_dot_scalars_tile instead of the library's"""
    R, flush = info()
    R = R if row_tile is None else row_tile
    assert flush == DOT_FLUSH == 256 and FLUSH_BATCHES == [1, 255, 256, 257, 515]
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    for batch in (FLUSH_BATCHES if batches is None else batches):
        for pattern in patterns:
            xc = _columns(side, ci, pattern if pattern != "alternating" else "max", rng, (size, batch))
            s = scalar_pattern(side, ci, pattern, rng, R + 1, batch)
            x = np.ascontiguousarray(np.tile(xc, n // 2))
            got, used = raw(side, ci, x, s, 1) if row_tile is None else raw_tile(side, ci, x, s, row_tile, 1)
            assert used == 1 and np.array_equal(got, np.tile(integers(xc, s, q), n // 2)), ("flush", n, batch, pattern, row_tile)


def case_cuts(n, bits, slice_counts=(1, 2, 3, 5, 23), sizes=(1, 2, 4), patterns=("max", "random"), batch=23, seed=67):
    """forced cuts of a batch of 23 - slice counts that do not divide it among them - for a lone row and for R + 1 rows: the words of
    the uncut call, which are the Python integers'"""
    R, _ = info()
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    assert batch in slice_counts and any(batch % s for s in slice_counts)
    for pattern in patterns:
        for size in sizes:
            for rows in (1, R + 1):
                xc = _columns(side, ci, pattern, rng, (size, batch))
                s = scalar_pattern(side, ci, pattern, rng, rows, batch)
                x = np.ascontiguousarray(np.tile(xc, n // 2))
                one, _ = raw(side, ci, x, s, 1)
                assert np.array_equal(one, np.tile(integers(xc, s, q), n // 2)), ("uncut", n, pattern, size, rows)
                for k in slice_counts:
                    assert np.array_equal(raw(side, ci, x, s, k)[0], one), ("cut", n, pattern, size, rows, k)


def case_natural_slices(scheme, n, bits, size=2, seed=71):
    """no forcing: by the documented rule, asked with the tiled thread count, a batch of 23 is cut and a batch of 7 is not (asserted
    from the rule, not assumed); slices_used is the rule's for both, and the evaluator's words are the one-launch words and the
    per-object forms'"""
    R, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, rows = side.first, R + 1
    K = len(side.ctx.coeff_modulus_at(ci))
    t = threads(size, rows, K, n)
    assert BR.rule_slices(t, 23) > 1 and BR.rule_slices(t, 7) == 1, ("the rule does not separate these shapes", t)
    for batch in (23, 7):
        x = side.rand_ct(rng, ci, batch, size)
        values = scalar_values(side, rng, rows, batch)
        buf, words = make_scalars(side, values, ci)
        got, used = raw(side, ci, x, words, 0)
        assert used == BR.rule_slices(t, batch), ("the library's rule is the documented one", batch, used)
        assert np.array_equal(got, raw(side, ci, x, words, 1)[0]), ("rule and one launch", batch)
        out = side.ev.dot_scalars_device(side.dev_ct(x, ci, True), buf, rows, side.scale)
        assert np.array_equal(out.to_numpy(), got), ("the evaluator's choice", batch)
        words_0, m = expect_row(side, x, values[rows - 1], ci)
        assert np.array_equal(got[:, rows - 1], words_0) and meta(out) == m, ("per-object forms", batch)


# ---- life cycle
def case_out_of_place(scheme, n, bits, seed=17):
    """the operand is unchanged; a destination of another level, size, form or context's worth of words is reshaped"""
    R, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, rows = side.first, R + 1
    x = side.rand_ct(rng, ci, BATCH, 2)
    values = scalar_values(side, rng, rows, BATCH)
    buf, words = make_scalars(side, values, ci)
    foreign = Side(scheme, n, bits)
    want = None
    for dest in (S.Ciphertext(side.ctx, batch=rows), side.dev_ct(side.rand_ct(rng, 0, rows, 2), 0, True),
                 side.dev_ct(side.rand_ct(rng, ci, rows, 4), ci, False), foreign.dev_ct(x[:, :rows], ci, True)):
        src = side.dev_ct(x, ci, True)
        got = side.ev.dot_scalars_device(src, buf, rows, side.scale, dest)
        assert got is dest and np.array_equal(src.to_numpy(), x) and meta(src) == (True, side.scale, side.cf), "encrypted changed"
        assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), 2, rows)
        if want is None:
            for o in (0, rows - 1):
                w, m = expect_row(side, x, values[o], ci)
                assert np.array_equal(dest.to_numpy()[:, o], w) and meta(dest) == m, ("per-object forms", o)
            want = dest.to_numpy(), meta(dest)
        assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], "reshaped destination"


def case_transparent_check(scheme, n, bits):
    """an all-zero result plane is refused when the check is on and computed when it is off; a zero SCALAR is an ordinary word"""
    R, _ = info()
    side = Side(scheme, n, bits)
    ci, rows = side.first, R + 1
    x = side.rand_ct(np.random.default_rng(3), ci, BATCH, 2)
    x0 = x.copy()
    x0[1] = 0
    values = scalar_values(side, np.random.default_rng(4), rows, BATCH)
    buf, words = make_scalars(side, values, ci)
    assert not np.any(words[0, 0]) and rows > 1, "a zero scalar among the weights"
    zeros = S.DeviceBuffer.from_numpy(np.zeros_like(words))
    assert not np.any(side.ev.dot_scalars_device(side.dev_ct(x0, ci, True), buf, rows, side.scale).to_numpy()[1])
    assert not np.any(side.ev.dot_scalars_device(side.dev_ct(x, ci, True), zeros, rows, side.scale).to_numpy())
    side.ev.set_transparent_check(True)
    try:
        _expect(S.LogicError, lambda: side.ev.dot_scalars_device(side.dev_ct(x0, ci, True), buf, rows, side.scale), "transparent result")
        _expect(S.LogicError, lambda: side.ev.dot_scalars_device(side.dev_ct(x, ci, True), zeros, rows, side.scale), "all-zero weights")
        out = side.ev.dot_scalars_device(side.dev_ct(x, ci, True), buf, rows, side.scale)
    finally:
        side.ev.set_transparent_check(False)
    assert np.array_equal(out.to_numpy(), via_dense_map(side, side.dev_ct(x, ci, True), words, rows).to_numpy())


def case_pending(n, bits, seed=73):
    """operands with a pending tensor product and with a deferred key-switch tail are settled before the call reads them, and a
    destination's own pending product is discarded: the words of the eager sequence (SEALHIP_LAZY_PRODUCT=0
    SEALHIP_KS_EAGER_TAIL=1), which are the dense-map words on the settled operands"""
    from parity_cases import _Env
    R, _ = info()
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, batch, rows = side.first, 3, R + 1
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    x, y = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)
    z = side.rand_ct(rng, ci, rows, 2), side.rand_ct(rng, ci, rows, 2)   # the destination's own pending product
    values = scalar_values(side, rng, rows, batch)
    buf, words = make_scalars(side, values, ci)

    def run():
        a, b = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
        prod = side.ev.multiply(a, b, S.Ciphertext(side.ctx, batch=batch))
        of_product = side.ev.dot_scalars_device(prod, buf, rows, side.scale)      # a pending product is formed first
        relin = side.ev.relinearize_inplace(side.ev.multiply(a, b, S.Ciphertext(side.ctx, batch=batch)), rlk)
        of_tail = side.ev.dot_scalars_device(relin, buf, rows, side.scale)        # a deferred tail is completed first
        a1, b1 = side.dev_ct(z[0], ci, True), side.dev_ct(z[1], ci, True)   # (alive: a product is formed when an operand goes away)
        dest = side.ev.multiply(a1, b1, S.Ciphertext(side.ctx, batch=rows))
        side.ev.dot_scalars_device(relin, buf, rows, side.scale, dest)            # pending state of the destination is discarded
        return [c.to_numpy() for c in (of_product, of_tail, dest, prod, relin)], (of_product.scale(), of_tail.scale())

    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT_MIN_WGS=0, SEALHIP_LAZY_PRODUCT=None, SEALHIP_KS_EAGER_TAIL=None):
        tails0, products0 = S.tail_stats(), S.product_stats()
        lazy, scales = run()
        tails1, products1 = S.tail_stats(), S.product_stats()
    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT=0, SEALHIP_KS_EAGER_TAIL=1):
        eager, _ = run()
    if two_pass_ring(n):   # the sizes at which the library defers
        assert tails1[1] - tails0[1] >= 1, "the call completed a deferred tail"
        assert products1[1] - products0[1] >= 1, "the call formed a pending product"
        assert products1[2] - products0[2] >= 1, "the destination's pending product was discarded"
    for got, want, what in zip(lazy, eager, ("of a product", "after relinearize", "into a pending destination", "product", "relinearized")):
        assert np.array_equal(got, want), what
    assert np.array_equal(lazy[1], lazy[2])
    assert scales == (side.scale ** 3, side.scale ** 3)
    # the dense map on the settled words
    saved, side.scale = side.scale, side.scale ** 2   # the operands carry the product's scale
    try:
        for src, got in ((lazy[3], lazy[0]), (lazy[4], lazy[1])):
            assert np.array_equal(via_dense_map(side, side.dev_ct(src, ci, True), words, rows, scale=saved).to_numpy(), got)
    finally:
        side.scale = saved


def case_capture(n, bits, batch=16, seed=47):
    """CKKS: the call recorded in a graph at a shape the documented rule cuts (pool scratch inside the recording), replayed twice
    with ciphertext words AND scalars refreshed in place: each replay equals the eager result and the dense-map words"""
    R, _ = info()
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, rows = side.first, R + 1
    K = len(side.ctx.coeff_modulus_at(ci))
    assert BR.rule_slices(threads(2, rows, K, n), batch) > 1, "the recorded call is cut"
    cx = side.dev_ct(side.rand_ct(rng, ci, batch, 2), ci, True)
    buf = S.DeviceBuffer(rows * batch * K)
    outs = [S.Ciphertext(side.ctx, batch=rows) for _ in range(2)]
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        s = np.ascontiguousarray(scalar_pattern(side, ci, "random", rng, rows, batch))
        S._native.check(h2d(C.c_void_p(buf.ptr), s.ctypes.data_as(C.c_void_p), C.c_uint64(s.nbytes)))
        w = np.ascontiguousarray(side.rand_ct(rng, ci, batch, 2))
        S._native.check(h2d(C.c_void_p(cx.device_ptr()[0]), w.ctypes.data_as(C.c_void_p), C.c_uint64(w.nbytes)))
        state["s"], state["x"] = s, w

    def step(o=outs[0]):
        side.ev.dot_scalars_device(cx, buf, rows, side.scale, o)

    refresh()
    step()   # eager once
    graph = side.ev.capture(step)
    seen = []
    for trial in range(2):
        refresh()
        graph.launch()
        replay = outs[0].to_numpy()
        step(outs[1])
        assert np.array_equal(replay, outs[1].to_numpy()) and meta(outs[0]) == meta(outs[1]), ("graph replay", trial)
        assert np.array_equal(replay, via_dense_map(side, cx, state["s"], rows).to_numpy()), ("replay and dense map", trial)
        assert np.array_equal(cx.to_numpy(), state["x"]), "the operand is only read"
        seen.append(replay)
    assert not np.array_equal(seen[0], seen[1]), "the replays saw different operand words"


# ---- errors
def case_errors(scheme, n, bits):
    """every check of Evaluator_DotScalarsDevice returns its HRESULT and leaves the destination untouched; a valid call afterwards
    works"""
    R, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, lib, ev = side.first, S._native.lib(), side.ev._h
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    rows = R + 1
    x = side.rand_ct(rng, ci, BATCH, 2)
    values = scalar_values(side, rng, rows, BATCH)
    buf, words = make_scalars(side, values, ci)
    cx = side.dev_ct(x, ci, True)
    dest = side.dev_ct(side.rand_ct(rng, ci, rows, 3), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)
    wrong_batch = S.Ciphertext(side.ctx, batch=rows + 1)
    foreign = Side(scheme, n, bits).dev_ct(x, ci, True)
    invalid = side.dev_ct(x, ci, True)
    invalid.set_scale(0.0 if scheme == "ckks" else 2.0)   # is_metadata_valid_for fails

    def call(ev_h, ct_h, ptr, r, b, scale, dest_h):
        return lib.Evaluator_DotScalarsDevice(ev_h, ct_h, C.c_void_p(ptr), C.c_uint64(r), C.c_uint64(b), C.c_double(scale), dest_h) & 0xFFFFFFFF

    good = (ev, cx._h, buf.ptr, rows, BATCH, side.scale, dest._h)
    for k in (0, 1, 6):
        args = list(good)
        args[k] = None
        assert call(*args) == POINTER, ("NULL handle", k)
    assert call(ev, invalid._h, *good[2:]) == INVALID, "an invalid ciphertext"
    assert call(ev, foreign._h, *good[2:]) == INVALID, "a ciphertext of another context"
    assert call(*good[:3], 0, *good[4:]) == INVALID, "rows == 0"
    assert call(*good[:3], -(-(1 << 32) // BATCH), *good[4:]) == INVALID, "rows * B >= 2^32"
    assert call(*good[:3], 1 << 32, *good[4:]) == INVALID and call(*good[:3], 1 << 63, *good[4:]) == INVALID, "rows beyond 32 bits"
    assert call(*good[:4], BATCH + 1, *good[5:]) == INVALID and call(*good[:4], BATCH - 1, *good[5:]) == INVALID, "batch != B"
    assert call(*good[:4], 0, *good[5:]) == INVALID, "batch 0"
    assert call(*good[:6], wrong_batch._h) == INVALID, "destination's batch != rows"
    assert call(ev, cx._h, buf.ptr, BATCH, BATCH, side.scale, cx._h) == INVALID, "destination == encrypted"
    assert call(ev, cx._h, None, *good[3:]) == INVALID, "NULL device_scalars"
    assert call(ev, cx._h, buf.ptr + 8, *good[3:]) == INVALID, "misaligned device_scalars"
    ptr, _ = cx.device_ptr()
    assert call(ev, cx._h, ptr + 16, *good[3:]) == INVALID, "device_scalars inside encrypted"
    ptr, _ = dest.device_ptr()
    assert call(ev, cx._h, ptr + 16, *good[3:]) == INVALID, "device_scalars inside destination"
    assert call(ev, side.dev_ct(x, ci, False)._h, *good[2:]) == INVALID, "a coefficient-form ciphertext"
    if scheme == "ckks":
        assert call(*good[:5], 0.0, dest._h) == INVALID, "CKKS plaintext scale"
        assert call(*good[:5], 2.0 ** 400, dest._h) == INVALID, "scale out of bounds"
    _expect(ValueError, lambda: side.ev.dot_scalars_device(cx, S.DeviceBuffer(words.size - 1), rows, side.scale, dest), "too few scalar words")
    assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
    assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
    assert np.array_equal(cx.to_numpy(), x)
    # a valid call afterwards
    side.ev.dot_scalars_device(cx, buf, rows, side.scale, dest)
    assert np.array_equal(dest.to_numpy(), via_dense_map(side, cx, words, rows).to_numpy())


def case_producer_errors(scheme, n, bits):
    """the common checks of the three producers: unknown parms_id, count == 0, NULL and misaligned pointers, the wrong scheme"""
    side = Side(scheme, n, bits)
    lib, ci = S._native.lib(), side.first
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    K = len(side.ctx.coeff_modulus_at(ci))
    pid, bad_pid = (C.c_uint64 * 4)(*side.ctx.parms_id_at(ci)), (C.c_uint64 * 4)(1, 2, 3, 4)
    out = _prefilled(4 * K + 2)
    if scheme == "ckks":
        enc = S.CKKSEncoder(side.ctx)
        dv, iv = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0), (C.c_int64 * 4)(1, -2, 3, -4)

        def fd(h, count, vals, p, dst):
            return lib.CKKSEncoder_EncodeScalars(h, C.c_uint64(count), vals, p, C.c_double(side.scale), C.c_void_p(dst)) & 0xFFFFFFFF

        def fi(h, count, vals, p, dst):
            return lib.CKKSEncoder_EncodeIntegerScalars(h, C.c_uint64(count), vals, p, C.c_void_p(dst)) & 0xFFFFFFFF
        for f, vals in ((fd, dv), (fi, iv)):
            assert f(None, 4, vals, pid, out.ptr) == POINTER, "NULL encoder"
            assert f(enc._h, 4, vals, bad_pid, out.ptr) == INVALID and f(enc._h, 4, vals, None, out.ptr) == INVALID, "unknown / NULL parms_id"
            assert f(enc._h, 0, vals, pid, out.ptr) == INVALID, "count == 0"
            assert f(enc._h, 4, None, pid, out.ptr) == INVALID and f(enc._h, 4, vals, pid, None) == INVALID, "NULL pointers"
            assert f(enc._h, 4, vals, pid, out.ptr + 8) == INVALID, "misaligned device_words"
        _expect(S.InvalidArgument, lambda: side.ev.lift_scalars([1, 2], side.ctx.parms_id_at(ci)), "CKKS is refused")
    else:
        uv = (C.c_uint64 * 4)(1, 2, 3, 4)

        def fl(h, count, vals, p, dst):
            return lib.Evaluator_LiftScalars(h, C.c_uint64(count), vals, p, C.c_void_p(dst)) & 0xFFFFFFFF
        assert fl(None, 4, uv, pid, out.ptr) == POINTER and fl(side.ev._h, 4, uv, None, out.ptr) == POINTER, "NULL handles"
        assert fl(side.ev._h, 4, uv, bad_pid, out.ptr) == INVALID, "unknown parms_id"
        assert fl(side.ev._h, 0, uv, pid, out.ptr) == INVALID, "count == 0"
        assert fl(side.ev._h, 4, None, pid, out.ptr) == INVALID and fl(side.ev._h, 4, uv, pid, None) == INVALID, "NULL pointers"
        assert fl(side.ev._h, 4, uv, pid, out.ptr + 8) == INVALID, "misaligned device_words"
        assert fl(side.ev._h, 4, (C.c_uint64 * 4)(1, 2, side.t, 4), pid, out.ptr) == INVALID, "a value >= t"
    assert np.all(out.to_numpy((4 * K + 2,)) == 0xA5A5A5A5), "failed calls write nothing"
