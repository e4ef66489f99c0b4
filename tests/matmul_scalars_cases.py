"""A matrix of scalar weights times a matrix of ciphertexts over the items of a batch (Evaluator_MatMulScalarsItems;
shl_matmul_scalars), shared by the CPU (emulated kernels) and `-m gpu` suites.  Exact word equality and the metadata triple
everywhere, no tolerances.  The weights have two forms: WIDE, [rows * inner][K] words (the producers' of Evaluator_DotScalarsDevice),
and NARROW, [rows * inner] signed 32-bit integers.  The yardsticks: Evaluator_MatMulPlainItems with the same flags on plaintexts each
filled with its weight's K words; Evaluator_DotScalarsDevice at cols = 1; the library's unchanged per-object forms on batches of one
(the constant plaintext, multiply_plain_inplace, add_many) and, where oracle/_ref is built, the REAL reference doing the same on its
own objects; and, around the two flush intervals, across the cuts and for every built row tile, Python-integer arithmetic, which
depends on neither library.  Row counts are written in terms of the row tile R the library reports for the form.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import batch_reduce_cases as BR
import dot_scalars_cases as DS
from harness import two_pass_ring
from batch_reduce_cases import meta, _columns
from matmul_plain_items_cases import transposed, result_transposed, laid_out
from plain_batch_cases import Side, _expect

INNER = 3
COLS = (1, 2, 3)
TILES = (4, 8)                      # include/sealhip.h (shl_matmul_scalars_tile): the built row tiles
FLAGS = (0, 1, 2, 3)                # bit 0: the ciphertexts are stored [cols][inner]; bit 1: the result is stored [cols][rows]
NARROW = 4                          # bit 2 of the C call's flags
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def info():
    """(R of the wide form, R of the narrow form, values of the inner index between two reductions: wide, narrow)"""
    v = [C.c_uint64() for _ in range(4)]
    S._native.check(S._native.lib().shl_matmul_scalars_info(*[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def row_tile(narrow):
    return info()[1 if narrow else 0]


def flush_interval(narrow):
    return info()[3 if narrow else 2]


def row_counts(R):
    """a lone row, a short tile, a full tile, a full tile and a lone row, two full tiles and a lone row"""
    return sorted({1, R - 1, R, R + 1, 2 * R + 1} - {0})


def shapes(R):
    """every row count with the column counts in turn; the largest row count last, with three columns and with one"""
    rows = row_counts(R)
    out = [(r, COLS[(i + 1) % 3]) for i, r in enumerate(rows[:-1])]
    return out + [(rows[-1], 1), (rows[-1], 3)]


def threads(size, rows, cols, K, n, R):
    """include/sealhip.h: one thread per coefficient pair of a plane, a TILE of R rows, a column and a prime"""
    return size * -(-rows // R) * cols * K * n // 2


# ---- weights
def int_weights(side, rng, rows, inner):
    """[rows][inner] Python integers a narrow weight may hold: for CKKS any signed 32-bit value, for BFV / BGV the centred range of
    the lift; 0, 1, -1 and both ends of the range among random ones.  No row is all zeros: add_many of nothing throws in the
    reference"""
    assert inner >= 2
    if side.scheme == "ckks":
        lo, hi = INT_MIN, INT_MAX
    else:
        half = (side.t + 1) // 2
        lo, hi = -(side.t - half), half - 1
    w = [[int(v) for v in row] for row in rng.integers(lo, hi + 1, (rows, inner))]
    special = [0, 1, -1, hi, lo]
    for i, v in enumerate(special):
        w[(i // inner) % rows][i % inner] = v
    for row in w:
        if not any(row):
            row[-1] = 7
    return w


def words_of(side, ci, ints):
    """[rows][inner] integers -> [rows * inner][K] canonical words w mod q_k, formed here with Python integers"""
    q = [int(v) for v in side.q(ci)]
    return np.array([[w % qk for qk in q] for row in ints for w in row], dtype=np.uint64)


def produced_words(side, ci, ints):
    """the same words from the library's public producers: EncodeIntegerScalars, or LiftScalars of w mod t -> DeviceBuffer"""
    pid = side.ctx.parms_id_at(ci)
    flat = [w for row in ints for w in row]
    if side.scheme == "ckks":
        return S.CKKSEncoder(side.ctx).encode_integer_scalars(flat, pid)
    return side.ev.lift_scalars([w % side.t for w in flat], pid)


def expanded(words, n):
    """[count][K] words -> [count][K][N] plaintexts, each filled with its weight's K words"""
    return np.ascontiguousarray(np.broadcast_to(words[:, :, None], words.shape + (n,)))


class Weights:
    """a rows x inner matrix of weights in one form: .buf for the call, .words [rows * inner][K] it stands for"""

    def __init__(self, side, rng, ci, rows, inner, narrow):
        self.narrow, self.rows, self.inner = narrow, rows, inner
        if narrow:
            self.values = int_weights(side, rng, rows, inner)
            self.host = np.array(self.values, dtype=np.int32)
            self.buf = S.DeviceBuffer.from_int32(self.host)
            self.words = words_of(side, ci, self.values)
        else:   # what the float and modulo-t producers write
            self.values = DS.scalar_values(side, rng, rows, inner)
            self.buf, w = DS.make_scalars(side, self.values, ci)
            self.words = self.host = w.reshape(rows * inner, -1)
        self.plain = S.DeviceBuffer.from_numpy(expanded(self.words, side.n))

    def unchanged(self):
        if self.narrow:
            return np.array_equal(self.buf.to_array(self.host.shape, np.int32), self.host)
        return np.array_equal(self.buf.to_numpy(self.host.shape), self.host)


def call(side, w, c, rows, inner, cols, flags=0, destination=None, scale=None):
    return side.ev.matmul_scalars_items(w.buf, c, rows, inner, cols, flags, side.scale if scale is None else scale, w.narrow, destination)


def yardstick(side, w, c, rows, inner, cols, flags=0, scale=None):
    """Evaluator_MatMulPlainItems with the same flags on the expanded plaintexts"""
    return side.ev.matmul_plain_items(w.plain, c, rows, inner, cols, side.scale if scale is None else scale, bool(flags & 1), bool(flags & 2))


def case_parity(scheme, n, bits, sizes=(2, 3), ci=None, inner=INNER, shape_list=None, per_object=True, seed=5):
    """every shape, all four combinations of flag bits 0 and 1, both forms: the words and metadata of MatMulPlainItems on the
    expanded plaintexts; with one column and no flag DotScalarsDevice's; at the largest shape also the per-object forms and the
    reference"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    for narrow in (False, True):
        for size in sizes:
            for rows, cols in (shapes(row_tile(narrow)) if shape_list is None else shape_list):
                what = (scheme, n, "narrow" if narrow else "wide", size, rows, cols)
                x = side.rand_ct(rng, ci, inner * cols, size)
                w = Weights(side, rng, ci, rows, inner, narrow)
                c, ct = side.dev_ct(x, ci, True), side.dev_ct(transposed(x, inner, cols), ci, True)
                for flags in FLAGS:
                    src = ct if flags & 1 else c
                    out, want = call(side, w, src, rows, inner, cols, flags), yardstick(side, w, src, rows, inner, cols, flags)
                    got = out.to_numpy()
                    assert got.shape == (size, rows * cols) + x.shape[2:], (what, got.shape)
                    assert (out.batch(), out.size(), out.parms_id()) == (rows * cols, size, side.ctx.parms_id_at(ci))
                    assert np.array_equal(got, want.to_numpy()) and meta(out) == meta(want), ("MatMulPlainItems", what, flags)
                    if flags == 0:
                        plain = got
                    else:   # the flags permute items and nothing else
                        assert np.array_equal(got, laid_out(x, plain, rows, inner, cols, (flags & 1, flags & 2))[1]), ("layout", what, flags)
                assert np.array_equal(c.to_numpy(), x) and w.unchanged(), "the operands are only read"
                if cols == 1 and not narrow:
                    dot = side.ev.dot_scalars_device(c, w.buf, rows, side.scale)
                    assert np.array_equal(plain, dot.to_numpy()) and meta(dot) == meta(want), ("DotScalarsDevice", what)
                if per_object and not narrow and (rows, cols) == shapes(row_tile(narrow))[-1]:
                    for i in range(rows):
                        for j in range(cols):
                            words, m = DS.expect_row(side, x[:, j::cols], w.values[i], ci)
                            assert np.array_equal(plain[:, i * cols + j], words) and meta(want) == m, ("per-object forms", what, i, j)


def case_narrow_equals_wide(scheme, n, bits, size=2, inner=5, seed=9):
    """integer weights - 0, 1, -1, 2^31 - 1 and -2^31 for CKKS, the ends of the centred range for BFV / BGV, random ones - given
    narrow and given wide as the words the public producers write for them (EncodeIntegerScalars; LiftScalars of w mod t): the same
    words and metadata, in every layout; and the producers' words are w mod q_k"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    for narrow_r in sorted({row_tile(True), row_tile(False)}):
        rows, cols = narrow_r + 1, 2
        ints = int_weights(side, rng, rows, inner)
        flat = [v for row in ints for v in row]
        assert {0, 1, -1} <= set(flat)
        if scheme == "ckks":   # (below 2^31 a prime meets the reference's wrap of q + w for w < -q: include/sealhip.h)
            assert INT_MAX in flat and INT_MIN in flat and all(int(q) > 2 ** 31 for q in side.q(ci)), "the premise"
        wide = produced_words(side, ci, ints)
        assert np.array_equal(wide.to_numpy((rows * inner, K)), words_of(side, ci, ints)), "the producers' words are w mod q"
        narrow = S.DeviceBuffer.from_int32(np.array(ints, dtype=np.int32))
        x = side.rand_ct(rng, ci, inner * cols, size)
        c, ct = side.dev_ct(x, ci, True), side.dev_ct(transposed(x, inner, cols), ci, True)
        for flags in FLAGS:
            src = ct if flags & 1 else c
            a = side.ev.matmul_scalars_items(wide, src, rows, inner, cols, flags, side.scale)
            b = side.ev.matmul_scalars_items(narrow, src, rows, inner, cols, flags, side.scale, narrow=True)
            assert np.array_equal(a.to_numpy(), b.to_numpy()) and meta(a) == meta(b), ("narrow and wide", scheme, n, rows, flags)
        if scheme == "ckks":   # the result's scale is ct.scale * scale, whatever the form
            assert meta(b)[1] == side.scale * side.scale
            one = side.ev.matmul_scalars_items(narrow, c, rows, inner, cols, 0, 1.0, narrow=True)
            assert meta(one)[1] == side.scale and np.array_equal(one.to_numpy(), side.ev.matmul_scalars_items(wide, c, rows, inner, cols, 0, 1.0).to_numpy())


# ---- the raw seam
def raw(side, ci, w, x, rows, inner, cols, flags=0, slices=0, tile=None):
    """shl_matmul_scalars (tile None) / shl_matmul_scalars_tile on raw words: w [rows * inner][K] uint64 or [rows * inner] int32 (which
    selects the narrow form), x [size][inner * cols][K][N] in the layout flags bit 0 says -> (words [size][rows * cols][K][N] in the
    layout bit 1 says, slices run)"""
    size, _, K, n = x.shape
    narrow = w.dtype == np.int32
    wb = S.DeviceBuffer.from_int32(w) if narrow else S.DeviceBuffer.from_numpy(w)
    a = S.DeviceBuffer.from_numpy(x)
    r = S.DeviceBuffer(size * rows * cols * K * n)
    used = C.c_uint64()
    lib = S._native.lib()
    args = (side.ctx._h, C.c_uint64(ci), C.c_void_p(wb.ptr), C.c_void_p(a.ptr), C.c_void_p(r.ptr), C.c_uint64(size), C.c_uint64(rows),
            C.c_uint64(inner), C.c_uint64(cols), C.c_uint64(flags | (NARROW if narrow else 0)), C.c_uint64(slices), C.byref(used))
    if tile is None:
        S._native.check(lib.shl_matmul_scalars(*args))
    else:
        S._native.check(lib.shl_matmul_scalars_tile(*args, C.c_uint64(tile), None))
    if slices:   # include/sealhip.h: the slices that ceil(inner / slices) values of the inner index each leave non-empty
        per = -(-inner // slices)
        assert used.value == -(-inner // per), ("slices run", used.value, slices)
    return r.to_numpy((size, rows * cols, K, n)), used.value   # (the copy back waits for the device)


def query(side, ci, size, rows, inner, cols, narrow=False, tile=0):
    """the seam's answer without a result: -> (HRESULT, slices the library would run)"""
    used = C.c_uint64()
    hr = S._native.lib().shl_matmul_scalars_tile(side.ctx._h, C.c_uint64(ci), None, None, None, C.c_uint64(size), C.c_uint64(rows),
                                                 C.c_uint64(inner), C.c_uint64(cols), C.c_uint64(NARROW if narrow else 0), C.c_uint64(0),
                                                 C.byref(used), C.c_uint64(tile), None) & 0xFFFFFFFF
    return hr, used.value


def integers(w, xc, q, rows, inner, cols):
    """Python integers: w [rows * inner][K] words or [rows * inner] signed integers, xc [size][inner * cols][K][2] (item (k, j) at
    k * cols + j) -> [size][rows * cols][K][2]"""
    xo = xc.astype(object)
    wo = np.array([[int(v)] * len(q) for v in w], dtype=object) if w.ndim == 1 else w.astype(object)
    want = np.zeros((xc.shape[0], rows * cols, len(q), 2), dtype=np.uint64)
    for i in range(rows):
        for j in range(cols):
            for k in range(len(q)):
                prods = wo[i * inner:(i + 1) * inner, k][None, :, None] * xo[:, j::cols, k]   # [size][inner][2]
                want[:, i * cols + j, k] = (prods.sum(axis=1) % q[k]).astype(np.uint64)
    return want


def weight_pattern(side, ci, pattern, rng, rows, inner, narrow):
    """"max": the largest magnitude every weight can have (q - 1; -2^31); "top": 2^31 - 1 (narrow); "alternating": the two extremes
    in turn along the rows and the inner index (q - 1 and 0; -2^31 and 2^31 - 1); "random\""""
    idx = np.indices((rows, inner))
    even = ((idx[0] + idx[1]) % 2 == 0).reshape(-1)
    if narrow:
        if pattern == "max":
            return np.full(rows * inner, INT_MIN, dtype=np.int32)
        if pattern == "top":
            return np.full(rows * inner, INT_MAX, dtype=np.int32)
        if pattern == "alternating":
            return np.where(even, INT_MIN, INT_MAX).astype(np.int32)
        return rng.integers(INT_MIN, INT_MAX + 1, rows * inner).astype(np.int32)
    q = side.q(ci)
    qk = np.broadcast_to(q, (rows * inner, q.size))
    if pattern in ("max", "top"):
        return (qk - 1).astype(np.uint64)
    if pattern == "alternating":
        return np.where(even[:, None], qk - 1, 0).astype(np.uint64)
    return (rng.integers(0, 2 ** 63, qk.shape, dtype=np.uint64) % qk).astype(np.uint64)


def pattern_operands(side, ci, pattern, rng, size, rows, inner, cols, n, narrow):
    """-> (w, x, the Python integers' words); but for "random" every ciphertext word is q - 1"""
    q = [int(v) for v in side.q(ci)]
    xc = _columns(side, ci, "random" if pattern == "random" else "max", rng, (size, inner * cols))
    w = weight_pattern(side, ci, pattern, rng, rows, inner, narrow)
    return w, np.ascontiguousarray(np.tile(xc, n // 2)), np.tile(integers(w, xc, q, rows, inner, cols), n // 2)


def case_flush(n, bits, narrow, patterns=("max", "top", "alternating", "random"), size=2, seed=61):
    """the inner index around the form's flush interval, R + 1 rows (a full tile and a short one) and two columns, one launch, all
    residues q - 1 and the extreme weights: every word equals the sum formed with Python integers - through the raw seam, whose
    threads add the whole inner index, and (at the longest) for the evaluator's own schedule"""
    flush, R = flush_interval(narrow), row_tile(narrow)
    assert flush == (1024 if narrow else BR.DOT_FLUSH), "include/sealhip.h"
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, cols = side.first, R + 1, 2
    for inner in (flush - 1, flush, flush + 1, 2 * flush + 1):
        for pattern in (p for p in patterns if narrow or p != "top"):   # (wide: "top" is "max")
            w, x, want = pattern_operands(side, ci, pattern, rng, size, rows, inner, cols, n, narrow)
            got, used = raw(side, ci, w, x, rows, inner, cols, slices=1)
            assert used == 1 and np.array_equal(got, want), ("flush", n, narrow, inner, pattern)
    buf = S.DeviceBuffer.from_int32(w) if narrow else S.DeviceBuffer.from_numpy(w)
    out = side.ev.matmul_scalars_items(buf, side.dev_ct(x, ci, True), rows, inner, cols, 0, side.scale, narrow)
    assert np.array_equal(out.to_numpy(), want), ("flush, evaluator", n, narrow)


def case_cuts(scheme, n, bits, inner=11, size=2, seed=67):
    """forced cuts of an inner index of 11, every slice count up to 8, at (R + 1) x 2, both forms: the words of the uncut call,
    which are MatMulPlainItems', in both ciphertext layouts, and slices_used as documented (asserted in raw); the natural slice
    count is the documented rule's, asked with the tiled thread count"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, cols = side.first, 2
    K = len(side.ctx.coeff_modulus_at(ci))
    for narrow in (False, True):
        R = row_tile(narrow)
        rows = R + 1
        x = side.rand_ct(rng, ci, inner * cols, size)
        xt = transposed(x, inner, cols)
        w = Weights(side, rng, ci, rows, inner, narrow)
        one, used = raw(side, ci, w.host, x, rows, inner, cols, slices=1)
        assert used == 1
        assert np.array_equal(one, yardstick(side, w, side.dev_ct(x, ci, True), rows, inner, cols).to_numpy()), "uncut and MatMulPlainItems"
        for s in range(1, min(inner, 8) + 1):
            assert np.array_equal(raw(side, ci, w.host, x, rows, inner, cols, slices=s)[0], one), ("cut", narrow, s)
            assert np.array_equal(raw(side, ci, w.host, xt, rows, inner, cols, 1, slices=s)[0], one), ("cut, transposed", narrow, s)
            assert np.array_equal(raw(side, ci, w.host, x, rows, inner, cols, 2, slices=s)[0], result_transposed(one, rows, cols)), ("cut, result transposed", narrow, s)
        for r, i, c in ((rows, inner, cols), (1, 64, 1), (rows, 64, cols), (4 * rows, 8, 4 * cols)):
            hr, natural = query(side, ci, size, r, i, c, narrow)
            assert hr == 0 and natural == BR.rule_slices(threads(size, r, c, K, n, R), i), ("the library's rule is the documented one", narrow, r, i, c)


def case_natural_slices(scheme, n, bits, inner=23, size=2, seed=71):
    """no forcing: a shape the documented rule cuts (asserted from the rule, not assumed) gives the one-launch words through the
    seam and through the evaluator, in both forms"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, cols = side.first, 1
    K = len(side.ctx.coeff_modulus_at(ci))
    for narrow in (False, True):
        R = row_tile(narrow)
        rows = R + 1
        want = BR.rule_slices(threads(size, rows, cols, K, n, R), inner)
        assert want > 1, ("the rule does not cut this shape", n, K)
        x = side.rand_ct(rng, ci, inner * cols, size)
        w = Weights(side, rng, ci, rows, inner, narrow)
        got, used = raw(side, ci, w.host, x, rows, inner, cols)
        assert used == want == query(side, ci, size, rows, inner, cols, narrow)[1]
        one, _ = raw(side, ci, w.host, x, rows, inner, cols, slices=1)
        assert np.array_equal(got, one), "rule and one launch"
        assert np.array_equal(call(side, w, side.dev_ct(x, ci, True), rows, inner, cols).to_numpy(), one), "the evaluator's choice"


def case_tiles(n, bits, inner=5, size=2, patterns=("max", "alternating", "random"), seed=83):
    """every row tile the library is built with - the rate tool sweeps them -, in both forms, gives the Python integers' words at
    2 R + 1 rows (two full tiles and a lone row) and at R - 1 (a short tile alone), two columns: both layouts of the ciphertexts and
    of the result, one launch and cut in two; a tile that is not built is refused"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, cols = side.first, 2
    for narrow in (False, True):
        for R in TILES:
            for rows in (2 * R + 1, R - 1):
                for p, pattern in enumerate(patterns):
                    w, x, want = pattern_operands(side, ci, pattern, rng, size, rows, inner, cols, n, narrow)
                    for flags in FLAGS:
                        xs, ws = laid_out(x, want, rows, inner, cols, (flags & 1, flags & 2))
                        slices = 1 + (flags + p) % 2   # one launch and cut in two in turn: every layout and pattern meets both
                        got, used = raw(side, ci, w, xs, rows, inner, cols, flags, slices, R)
                        assert used == slices and np.array_equal(got, ws), ("tile", n, narrow, R, rows, pattern, flags, slices)
        for bad in (1, 2, 3, 16, 1 << 8 | 4, 1 << 32):
            assert query(side, ci, size, 3, inner, cols, narrow, bad)[0] == S._native.E_INVALIDARG, ("a row tile that is not built", bad)


# ---- life cycle
def case_out_of_place(scheme, n, bits, size=2, seed=17):
    """the operands are unchanged; a destination that held another size, level or form is reshaped to the operand's size and level"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, inner, cols = side.first, 2, 2
    for narrow in (False, True):
        rows = row_tile(narrow) + 1
        out = rows * cols
        x = side.rand_ct(rng, ci, inner * cols, size)
        w = Weights(side, rng, ci, rows, inner, narrow)
        want = None
        for dest in (S.Ciphertext(side.ctx, batch=out), side.dev_ct(side.rand_ct(rng, 0, out, 2), 0, True),
                     side.dev_ct(side.rand_ct(rng, ci, out, 4), ci, False)):
            c = side.dev_ct(x, ci, True)
            got = call(side, w, c, rows, inner, cols, destination=dest)
            assert got is dest and np.array_equal(c.to_numpy(), x) and meta(c) == (True, side.scale, side.cf), "the operand changed"
            assert w.unchanged(), "the weights changed"
            assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), size, out)
            if want is None:
                plain = yardstick(side, w, c, rows, inner, cols)
                assert np.array_equal(dest.to_numpy(), plain.to_numpy()) and meta(dest) == meta(plain)
                want = dest.to_numpy(), meta(dest)
            assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], "reshaped destination"


def case_transparent_check(scheme, n, bits):
    """with the check on the RESULT batch is checked: an all-zero second polynomial is refused (and computed with the check off),
    and so are all-zero weights in either form; a proper result passes"""
    side = Side(scheme, n, bits)
    ci, rows, inner, cols = side.first, 2, 2, 2
    K = len(side.ctx.coeff_modulus_at(ci))
    x = side.rand_ct(np.random.default_rng(3), ci, inner * cols, 2)
    x0 = x.copy()
    x0[1] = 0
    for narrow in (False, True):
        w = Weights(side, np.random.default_rng(4), ci, rows, inner, narrow)
        zeros = Weights(side, np.random.default_rng(4), ci, rows, inner, narrow)
        zeros.buf = S.DeviceBuffer.from_numpy(np.zeros(rows * inner * K, dtype=np.uint64))
        zero = call(side, w, side.dev_ct(x0, ci, True), rows, inner, cols).to_numpy()
        assert not np.any(zero[1]) and np.any(zero[0])
        assert not np.any(call(side, zeros, side.dev_ct(x, ci, True), rows, inner, cols).to_numpy())
        side.ev.set_transparent_check(True)
        try:
            _expect(S.LogicError, lambda: call(side, w, side.dev_ct(x0, ci, True), rows, inner, cols), "transparent result")
            _expect(S.LogicError, lambda: call(side, zeros, side.dev_ct(x, ci, True), rows, inner, cols), "all-zero weights")
            c = side.dev_ct(x, ci, True)
            out = call(side, w, c, rows, inner, cols)
        finally:
            side.ev.set_transparent_check(False)
        assert np.array_equal(out.to_numpy(), yardstick(side, w, c, rows, inner, cols).to_numpy())


def case_pending(n, bits, seed=73):
    """the operand is the result of relinearize with its key-switch tail still deferred, and - in a second call - a tensor product
    that has not been formed; the destination holds a pending product of its own.  The words are those of the eager sequence
    (SEALHIP_LAZY_PRODUCT=0 SEALHIP_KS_EAGER_TAIL=1) and of MatMulPlainItems on the settled operands, in both forms"""
    from parity_cases import _Env
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, inner, cols = side.first, 2, 1
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    for narrow in (False, True):
        rows = row_tile(narrow) + 1
        bx, out_items = inner * cols, rows * cols
        a, b = side.rand_ct(rng, ci, bx, 2), side.rand_ct(rng, ci, bx, 2)
        z = side.rand_ct(rng, ci, out_items, 2), side.rand_ct(rng, ci, out_items, 2)
        w = Weights(side, rng, ci, rows, inner, narrow)

        def run():
            ca, cb = side.dev_ct(a, ci, True), side.dev_ct(b, ci, True)
            prod = side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=bx))
            of_product = call(side, w, prod, rows, inner, cols)                                                    # a pending product is formed first
            relin = side.ev.relinearize_inplace(side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=bx)), rlk)   # a deferred tail
            z0, z1 = side.dev_ct(z[0], ci, True), side.dev_ct(z[1], ci, True)   # (alive: a product is formed when an operand goes away)
            dest = side.ev.multiply(z0, z1, S.Ciphertext(side.ctx, batch=out_items))                               # the destination's own
            call(side, w, relin, rows, inner, cols, destination=dest)
            shape = (dest.size(), dest.batch(), meta(dest), of_product.size(), meta(of_product))
            return [v.to_numpy() for v in (of_product, dest, prod, relin)], shape

        with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT_MIN_WGS=0, SEALHIP_LAZY_PRODUCT=None, SEALHIP_KS_EAGER_TAIL=None):
            tails0, products0 = S.tail_stats(), S.product_stats()
            lazy, shape = run()
            tails1, products1 = S.tail_stats(), S.product_stats()
        with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT=0, SEALHIP_KS_EAGER_TAIL=1):
            eager, shape_e = run()
        if two_pass_ring(n):   # the sizes at which the library defers
            assert tails1[1] - tails0[1] >= 1, "the call completed a deferred tail"
            assert products1[1] - products0[1] >= 1, "the call formed a pending product"
            assert products1[2] - products0[2] >= 1, "the destination's pending product was discarded"
        assert shape == shape_e == (2, out_items, (True, side.scale ** 3, 1), 3, (True, side.scale ** 3, 1))
        for got, want, what in zip(lazy, eager, ("of a product", "into a pending destination", "product", "relinearized")):
            assert np.array_equal(got, want), (what, narrow)
        saved, side.scale = side.scale, side.scale ** 2   # the operands carry the product's scale
        try:
            for src, got in ((lazy[2], lazy[0]), (lazy[3], lazy[1])):
                assert np.array_equal(yardstick(side, w, side.dev_ct(src, ci, True), rows, inner, cols, scale=saved).to_numpy(), got), ("MatMulPlainItems", narrow)
        finally:
            side.scale = saved


def case_capture(n, bits, narrow, inner=16, size=2, seed=47):
    """CKKS: one call recorded in a graph at a shape the documented rule cuts (pool scratch inside the recording), replayed twice
    with the ciphertexts' and the weights' words refreshed in place: each replay equals the eager result and MatMulPlainItems"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    R = row_tile(narrow)
    ci, rows, cols = side.first, R, 3   # one row of tiles: few enough threads at N = 8192 for the rule to cut
    K = len(side.ctx.coeff_modulus_at(ci))
    assert BR.rule_slices(threads(size, rows, cols, K, n, R), inner) > 1, "the recorded call is cut"
    c = side.dev_ct(side.rand_ct(rng, ci, inner * cols, size), ci, True)
    w = Weights(side, rng, ci, rows, inner, narrow)
    outs = [S.Ciphertext(side.ctx, batch=rows * cols) for _ in range(2)]
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        fresh = Weights(side, rng, ci, rows, inner, narrow)   # (its own buffers are dropped: the words go into the recorded ones)
        h = np.ascontiguousarray(fresh.host)
        S._native.check(h2d(C.c_void_p(w.buf.ptr), h.ctypes.data_as(C.c_void_p), C.c_uint64(h.nbytes)))
        w.host, w.plain = h, fresh.plain
        x = np.ascontiguousarray(side.rand_ct(rng, ci, inner * cols, size))
        S._native.check(h2d(C.c_void_p(c.device_ptr()[0]), x.ctypes.data_as(C.c_void_p), C.c_uint64(x.nbytes)))
        state["x"] = x

    def step(o=outs[0]):
        call(side, w, c, rows, inner, cols, 3, destination=o)

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
        assert np.array_equal(replay, yardstick(side, w, c, rows, inner, cols, 3).to_numpy()), ("replay and MatMulPlainItems", trial)
        assert np.array_equal(c.to_numpy(), state["x"]) and w.unchanged(), "the operands are only read"
        seen.append(replay)
    assert not np.array_equal(seen[0], seen[1]), "the replays saw different operand words"


# ---- errors
def case_errors(scheme, n, bits):
    """every refusal of the contract returns its HRESULT and leaves the destination's words and metadata as they were; a valid call
    afterwards works"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, lib, ev = side.first, S._native.lib(), side.ev._h
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    rows, inner, cols = 3, 2, 2
    x = side.rand_ct(rng, ci, inner * cols, 2)
    c = side.dev_ct(x, ci, True)
    dest = side.dev_ct(side.rand_ct(rng, ci, rows * cols, 3), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)

    def call_c(ev_h, ptr, ct_h, r, i, cc, flags, scale, dest_h):
        return lib.Evaluator_MatMulScalarsItems(ev_h, C.c_void_p(ptr), ct_h, C.c_uint64(r), C.c_uint64(i), C.c_uint64(cc), C.c_uint64(flags),
                                                C.c_double(scale), dest_h) & 0xFFFFFFFF

    for narrow in (False, True):
        w = Weights(side, rng, ci, rows, inner, narrow)
        form = NARROW if narrow else 0
        good = (ev, w.buf.ptr, c._h, rows, inner, cols, form, side.scale, dest._h)
        for k in (0, 2, 8):
            args = list(good)
            args[k] = None
            assert call_c(*args) == POINTER, ("NULL handle", k)
        for k in (3, 4, 5):
            args = list(good)
            args[k] = 0
            assert call_c(*args) == INVALID, ("a zero dimension", k)
            args[k] = 1 << 32
            assert call_c(*args) == INVALID, ("a dimension beyond 32 bits", k)
            args[k] = 1 << 63
            assert call_c(*args) == INVALID, ("a dimension beyond 32 bits", k)
        assert call_c(ev, w.buf.ptr, c._h, 1 << 31, 2, 1, form, side.scale, dest._h) == INVALID, "rows * inner >= 2^32"
        assert call_c(ev, w.buf.ptr, c._h, 1, 2, 1 << 31, form, side.scale, dest._h) == INVALID, "inner * cols >= 2^32"
        assert call_c(ev, w.buf.ptr, c._h, 1 << 16, 1, 1 << 16, form, side.scale, dest._h) == INVALID, "rows * cols >= 2^32"
        for flags in (8, 15, 1 << 8, 1 << 63):
            assert call_c(*good[:6], flags | form, *good[7:]) == INVALID, ("an unknown flag", flags)
        assert call_c(ev, w.buf.ptr, c._h, rows, inner, cols + 1, form, side.scale, dest._h) == INVALID, "the ciphertext's batch != inner * cols"
        assert call_c(ev, w.buf.ptr, c._h, rows, inner + 1, cols, form, side.scale, dest._h) == INVALID, "the ciphertext's batch != inner * cols"
        assert call_c(ev, w.buf.ptr, c._h, rows + 1, inner, cols, form, side.scale, dest._h) == INVALID, "the destination's batch != rows * cols"
        assert call_c(*good[:8], S.Ciphertext(side.ctx, batch=rows * cols + 1)._h) == INVALID, "the destination's batch"
        assert call_c(ev, w.buf.ptr, c._h, 2, 2, 2, form, side.scale, c._h) == INVALID, "destination == encrypted"
        assert call_c(ev, None, *good[2:]) == INVALID, "NULL device_weights"
        assert call_c(ev, w.buf.ptr + 8, *good[2:]) == INVALID, "misaligned device_weights"
        ptr, _ = c.device_ptr()
        assert call_c(ev, ptr + 16, *good[2:]) == INVALID, "device_weights inside encrypted"
        ptr, words = dest.device_ptr()
        assert call_c(ev, ptr + 16, *good[2:]) == INVALID, "device_weights inside destination"
        invalid = side.dev_ct(x, ci, True)
        invalid.set_scale(0.0 if scheme == "ckks" else 2.0)   # is_metadata_valid_for fails
        foreign = Side(scheme, n, bits).dev_ct(x, ci, True)
        for bad, what in ((invalid, "an invalid ciphertext"), (foreign, "a ciphertext of another context"), (side.dev_ct(x, ci, False), "coefficient form")):
            assert call_c(ev, w.buf.ptr, bad._h, *good[3:]) == INVALID, what
        if scheme == "ckks":
            assert call_c(*good[:7], 0.0, dest._h) == INVALID, "CKKS weight scale"
            assert call_c(*good[:7], 2.0 ** 400, dest._h) == INVALID, "scale out of bounds"
        _expect(ValueError, lambda: side.ev.matmul_scalars_items(S.DeviceBuffer(2), c, rows, inner, cols, 0, side.scale, narrow, dest), "too few weight words")
        # a result the flat grid refuses: its rows are numbered in 32 bits (asked of the seam, which allocates nothing for a query)
        K, R, big = len(side.ctx.coeff_modulus_at(ci)), row_tile(narrow), 46340
        assert big * big < 1 << 32 <= 16 * K * -(-big // R) * big, "the premise"
        assert query(side, ci, 16, big, 1, big, narrow)[0] == INVALID, "a result the flat grid refuses"
        assert query(side, ci, 1, R, 1, 1, narrow) == (0, 1)
        assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
        assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
        assert np.array_equal(c.to_numpy(), x) and w.unchanged()
    # a valid call afterwards
    call(side, w, c, rows, inner, cols, destination=dest)
    plain = yardstick(side, w, c, rows, inner, cols)
    assert np.array_equal(dest.to_numpy(), plain.to_numpy()) and meta(dest) == meta(plain)
