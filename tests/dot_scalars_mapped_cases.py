"""A sparse matrix of scalar weights times a batch over an item map (Evaluator_DotScalarsMapped; shl_dot_scalars_mapped), shared by
the CPU (emulated kernels) and `-m gpu` suites.  Exact word equality and the metadata triple everywhere, no tolerances.  The weights
have the two forms of Evaluator_MatMulScalarsItems: WIDE, [count][K] words, and NARROW, [count] signed 32-bit integers.  The
yardsticks: Evaluator_DotPlainMapped with the same map on plaintexts each filled with its weight's K words; Evaluator_DotScalarsDevice
over the dense map and Evaluator_Conv2dScalarsItems over the map of the in-image taps; the library's unchanged per-object forms on
batches of one (the constant plaintext, multiply_plain_inplace, add_many) and, where oracle/_ref is built, the REAL reference doing
the same on its own objects; and, for the shapes only this call has, around both flush intervals and across the cuts,
Python-integer arithmetic, which depends on neither library.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import batch_reduce_cases as BR
import dot_scalars_cases as DS
import item_map_cases as IM
import matmul_scalars_cases as MS
import conv2d_scalars_cases as CV
from harness import two_pass_ring
from batch_reduce_cases import meta, _columns
from item_map_cases import SOURCE, ROWS, SECOND_OF_3, CUT_LENGTHS, draw_rows
from matmul_scalars_cases import INT_MIN, INT_MAX
from plain_batch_cases import Side, _expect

NARROW = 4   # bit 2 of the C call's flags: Evaluator_MatMulScalarsItems' bit
WIDE_FLUSH, NARROW_FLUSH = 256, 1024   # include/sealhip.h
# long and short rows in one map: on a ring of 8 the lanes of one wave sit in all of them and flush at different trips
FLUSH_LENGTHS = {False: [1, WIDE_FLUSH - 1, WIDE_FLUSH, WIDE_FLUSH + 1, 3, 2 * WIDE_FLUSH + 3],
                 True: [1, NARROW_FLUSH - 1, NARROW_FLUSH, NARROW_FLUSH + 1, 3]}


def flush_intervals():
    a, b = C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_dot_scalars_mapped_info(C.byref(a), C.byref(b)))
    return a.value, b.value


def weights(side, rng, ci, count, narrow):
    """`count` weights in one form (matmul_scalars_cases.Weights as one row): .buf, .words [count][K], .plain, .values[0]"""
    return MS.Weights(side, rng, ci, 1, count, narrow)


def make_map(side, rows, second, first_batch, count):
    """rows / second: the first and second list, row by row; second None: "the same list\""""
    if second is None:
        return S.ItemMap(side.ctx, rows, first_batch)
    return S.ItemMap(side.ctx, rows, first_batch, second=second, second_batch=count)


def call(side, w, c, m, count, destination=None, scale=None):
    return side.ev.dot_scalars_mapped(c, w.buf, count, m, 0, side.scale if scale is None else scale, w.narrow, destination)


def yardstick(side, w, c, m, count, scale=None):
    """Evaluator_DotPlainMapped with the same map on the expanded plaintexts"""
    return side.ev.dot_plain_mapped(c, w.plain, count, m, side.scale if scale is None else scale)


def same(got, want, what):
    assert (got.batch(), got.size(), got.parms_id()) == (want.batch(), want.size(), want.parms_id()), what
    assert np.array_equal(got.to_numpy(), want.to_numpy()) and meta(got) == meta(want), what


def integers(w, xc, q, rows, second):
    """Python integers: w [count][K] words or [count] signed integers, xc [size][items][K][2] -> [size][rows][K][2]"""
    xo = xc.astype(object)
    wo = np.array([[int(v)] * len(q) for v in w], dtype=object) if w.ndim == 1 else w.astype(object)
    want = np.zeros((xc.shape[0], len(rows), len(q), 2), dtype=np.uint64)
    for o, row in enumerate(rows):
        sec = second[o] if second is not None else row
        for k in range(len(q)):
            want[:, o, k] = ((xo[:, row, k] * wo[sec, k][None, :, None]).sum(axis=1) % q[k]).astype(np.uint64)
    return want


# ---- parity
def case_parity(scheme, n, bits, sizes=(2, 3), ci=None, source=SOURCE, rows=ROWS, second=SECOND_OF_3, per_object=True, seed=5):
    """the parity map of the item maps - a one-term row, an item named twice, a weight named twice - with its second list into 3
    weights and as a map without a second list (one weight per input item), both forms: the words and metadata of DotPlainMapped
    on the expanded plaintexts; the wide form's longest row also through the per-object forms and the reference"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    other = 1 + max(i for r in second for i in r)
    assert any(len(r) == 1 for r in rows) and any(len(set(r)) < len(r) for r in rows) and any(len(set(r)) < len(r) for r in second)
    for narrow in (False, True):
        for size in sizes:
            for sec, count in ((second, other), (None, source)):
                what = (scheme, n, "narrow" if narrow else "wide", size, "two lists" if sec else "one list")
                m = make_map(side, rows, sec, source, count)
                x = side.rand_ct(rng, ci, source, size)
                w = weights(side, rng, ci, count, narrow)
                c = side.dev_ct(x, ci, True)
                out = call(side, w, c, m, count)
                assert (out.batch(), out.size(), out.parms_id()) == (len(rows), size, side.ctx.parms_id_at(ci)), what
                same(out, yardstick(side, w, c, m, count), ("DotPlainMapped", what))
                assert np.array_equal(c.to_numpy(), x) and w.unchanged(), "the operands are only read"
                if per_object and not narrow and sec is None and size == sizes[-1]:
                    got = out.to_numpy()
                    for o, row in enumerate(rows):
                        words, mt = DS.expect_row(side, x[:, row], [w.values[0][j] for j in row], ci)
                        assert np.array_equal(got[:, o], words) and meta(out) == mt, ("per-object forms", what, o)


# ---- the shapes that other calls have too
def case_dense(scheme, n, bits, rows=5, batch=3, size=2, seed=7):
    """the dense map - row o names the items 0 .. B - 1, term (o, b) names weight o B + b - gives DotScalarsDevice's words"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    m = make_map(side, [list(range(batch))] * rows, [[o * batch + b for b in range(batch)] for o in range(rows)], batch, rows * batch)
    x = side.rand_ct(rng, ci, batch, size)
    c = side.dev_ct(x, ci, True)
    w = MS.Weights(side, rng, ci, rows, batch, False)
    same(call(side, w, c, m, rows * batch), side.ev.dot_scalars_device(c, w.buf, rows, side.scale), ("DotScalarsDevice", scheme, n))


def case_conv(scheme, n, bits, oc=3, size=2, seed=8):
    """the map of the in-image taps of the padded 3 x 3 shape, weight o * inner + tap: Conv2dScalarsItems' words, in both forms"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    s = CV.shape_of(CV.SAME_3X3, oc)
    taps = CV.tap_rows(s)
    items, count = s.in_channels * s.height * s.width, oc * CV.inner_of(s)
    m = make_map(side, [[t[0] for t in r] for r in taps], [[t[1] for t in r] for r in taps], items, count)
    x = side.rand_ct(rng, ci, items, size)
    c = side.dev_ct(x, ci, True)
    for narrow in (False, True):
        w = MS.Weights(side, rng, ci, oc, CV.inner_of(s), narrow)
        same(call(side, w, c, m, count), side.ev.conv2d_scalars_items(w.buf, c, s, 0, side.scale, narrow), ("Conv2dScalarsItems", scheme, n, narrow))


# ---- what only this call can do
def depthwise_rows(channels=2, height=3, width=3, k=3, pad=1):
    """output (c, y, x) adds the taps (dy, dx) of ITS channel inside the image: weight c * k * k + dy * k + dx"""
    rows, second = [], []
    for c in range(channels):
        for y in range(height):
            for x in range(width):
                taps = [(dy, dx) for dy in range(k) for dx in range(k) if 0 <= y + dy - pad < height and 0 <= x + dx - pad < width]
                rows.append([(c * height + y + dy - pad) * width + x + dx - pad for dy, dx in taps])
                second.append([(c * k + dy) * k + dx for dy, dx in taps])
    return rows, second, channels * height * width, channels * k * k


def dilated_rows(height=4, width=5, k=2, dilation=2, oc=2):
    """a k x k kernel whose taps are `dilation` pixels apart, one input channel, no padding: weight (o * k + dy) * k + dx"""
    oh, ow = height - dilation * (k - 1), width - dilation * (k - 1)
    rows, second = [], []
    for o in range(oc):
        for y in range(oh):
            for x in range(ow):
                rows.append([(y + dilation * dy) * width + x + dilation * dx for dy in range(k) for dx in range(k)])
                second.append([(o * k + dy) * k + dx for dy in range(k) for dx in range(k)])
    return rows, second, height * width, oc * k * k


def pooling_rows(channels=2, height=3, width=5, k=2):
    """k x k average pooling with stride k; the last window of a row / column is ragged.  One weight per window size (the
    reciprocal of its count, as the caller encodes it): weight number = the position of the size in the sorted list of sizes"""
    oh, ow = -(-height // k), -(-width // k)
    windows = []
    for c in range(channels):
        for y in range(oh):
            for x in range(ow):
                windows.append([(c * height + iy) * width + ix for iy in range(y * k, min(height, (y + 1) * k))
                                for ix in range(x * k, min(width, (x + 1) * k))])
    sizes = sorted({len(r) for r in windows})
    assert len(sizes) > 1, "a ragged window"
    return windows, [[sizes.index(len(r))] * len(r) for r in windows], channels * height * width, max(len(sizes), 2)


ONLY_HERE = (("depthwise 3 x 3, pad 1, C = 2 of 3 x 3", depthwise_rows), ("2 x 2 kernel, dilation 2", dilated_rows),
             ("2 x 2 average pooling, ragged last window", pooling_rows))


def case_only_here(scheme, n, bits, size=2, seed=13):
    """depthwise and dilated convolution and average pooling with a ragged window, both forms: DotPlainMapped's words and metadata
    on the expanded plaintexts and the sums formed with Python integers"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    for what, make in ONLY_HERE:
        rows, second, items, count = make()
        m = make_map(side, rows, second, items, count)
        for narrow in (False, True):
            xc = _columns(side, ci, "random", rng, (size, items))
            x = np.ascontiguousarray(np.tile(xc, n // 2))
            w = weights(side, rng, ci, count, narrow)
            c = side.dev_ct(x, ci, True)
            out = call(side, w, c, m, count)
            same(out, yardstick(side, w, c, m, count), ("DotPlainMapped", what, scheme, n, narrow))
            assert np.array_equal(out.to_numpy(), np.tile(integers(w.words, xc, q, rows, second), n // 2)), ("integers", what, scheme, n, narrow)


# ---- narrow equals wide
def case_narrow_equals_wide(scheme, n, bits, size=2, seed=9):
    """integer weights - 0, 1, -1, 2^31 - 1 and -2^31 for CKKS, the ends of the centred range for BFV / BGV, random ones - given
    narrow and given wide as the words the public producers write for them: the same words and metadata, with and without a
    second list; and the producers' words are w mod q_k"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    for sec, count in ((None, SOURCE), ([[4], [0, 2, 2], [0, 1, 2, 3, 4, 5, 1], [3, 0]], 6)):
        ints = MS.int_weights(side, rng, 1, count)
        flat = ints[0]
        assert {0, 1, -1} <= set(flat)
        if scheme == "ckks":   # (below 2^31 a prime meets the reference's wrap of q + w for w < -q: include/sealhip.h)
            assert INT_MAX in flat and INT_MIN in flat and all(int(q) > 2 ** 31 for q in side.q(ci)), "the premise"
        wide = MS.produced_words(side, ci, ints)
        assert np.array_equal(wide.to_numpy((count, K)), MS.words_of(side, ci, ints)), "the producers' words are w mod q"
        narrow = S.DeviceBuffer.from_int32(np.array(flat, dtype=np.int32))
        m = make_map(side, ROWS, sec, SOURCE, count)
        c = side.dev_ct(side.rand_ct(rng, ci, SOURCE, size), ci, True)
        a = side.ev.dot_scalars_mapped(c, wide, count, m, 0, side.scale)
        b = side.ev.dot_scalars_mapped(c, narrow, count, m, 0, side.scale, narrow=True)
        same(a, b, ("narrow and wide", scheme, n, count))
        if scheme == "ckks":   # the result's scale is ct.scale * scale, whatever the form
            assert meta(b)[1] == side.scale * side.scale
            assert meta(side.ev.dot_scalars_mapped(c, narrow, count, m, 0, 1.0, narrow=True))[1] == side.scale


# ---- the raw seam
def _guarded(words, guard, fill):
    sentinel = np.full(guard, fill, dtype=np.uint64)
    return np.concatenate([sentinel, words, sentinel])


def raw(side, ci, w, x, item_map, slices=0, guard=0):
    """shl_dot_scalars_mapped on raw words with a given cut (0: the library's rule): w [count][K] uint64 or [count] int32 (which
    selects the narrow form), x [size][a_batch][K][N] -> (words [size][rows][K][N], slices run).  guard: words of a sentinel in front
    of and behind the input, the weights and the result, inside the same device allocations; they must be intact afterwards"""
    size, a_batch, K, n = x.shape
    narrow = w.dtype == np.int32
    rows, _, longest, _, count = item_map.info()
    assert guard % 2 == 0 and count == w.shape[0]
    flat = np.ascontiguousarray(w).reshape(-1)
    if narrow:
        flat = np.concatenate([flat, np.zeros(flat.size % 2, dtype=np.int32)]).view(np.uint64)
    out_words = size * rows * K * n
    images = [_guarded(x.reshape(-1), guard, 0xA5A5A5A5A5A5A5A5), _guarded(flat, guard, 0xC3C3C3C3C3C3C3C3),
              _guarded(np.full(out_words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), guard, 0x9696969696969696)]
    a, wb, r = (S.DeviceBuffer.from_numpy(v) for v in images)
    used = C.c_uint64()
    lib = S._native.lib()

    def run(rp, scratch):
        S._native.check(lib.shl_dot_scalars_mapped(side.ctx._h, C.c_uint64(ci), C.c_void_p(wb.ptr + 8 * guard), C.c_uint64(count),
                                                   C.c_int(int(narrow)), C.c_void_p(a.ptr + 8 * guard), C.c_uint64(a_batch), C.c_void_p(rp),
                                                   C.c_uint64(size), item_map._h, C.c_uint64(slices), C.c_void_p(scratch), C.byref(used), None))
    run(None, None)   # the slices this will run in
    scratch = S.DeviceBuffer(max(used.value * out_words, 1))
    run(r.ptr + 8 * guard, scratch.ptr)
    S.device_synchronize()
    if slices:   # include/sealhip.h: the slices that ceil(longest_row / slices) terms each leave non-empty
        per = -(-longest // slices)
        assert used.value == -(-longest // per), ("slices run", used.value, slices)
    back = r.to_numpy(out_words + 2 * guard)
    if guard:
        assert np.array_equal(back[:guard], images[2][:guard]) and np.array_equal(back[-guard:], images[2][-guard:]), "words next to the result were written"
        assert np.array_equal(a.to_numpy(images[0].size), images[0]), "the input's allocation was written"
        assert np.array_equal(wb.to_numpy(images[1].size), images[1]), "the weights' allocation was written"
    return back[guard:guard + out_words].reshape(size, rows, K, n), used.value


def host_weights(side, ci, pattern, rng, count, narrow):
    """matmul_scalars_cases.weight_pattern for `count` weights: "max" q - 1 / -2^31, "top" 2^31 - 1, "alternating", "random\""""
    return MS.weight_pattern(side, ci, pattern, rng, 1, count, narrow)


def device_weights(w):
    return S.DeviceBuffer.from_int32(w) if w.dtype == np.int32 else S.DeviceBuffer.from_numpy(w)


# ---- flush boundaries: Python-integer arithmetic
def case_flush(n, bits, narrow, patterns=("max", "alternating", "half", "random"), source=SOURCE, count=5, size=2, seed=61):
    """one map whose rows have 1, F - 1, F, F + 1 and 3 terms (wide: and 2 F + 3) around the form's flush interval F, in this order,
    drawn with repeats from 7 items and 5 weights.  Operand words all q - 1, alternating, q / 2 and random; weights q - 1 (wide) and
    -2^31, 2^31 - 1 and the two in turn (narrow).  Every word equals the sum formed with Python integers, for the one-launch form
    whose threads walk whole rows and for the evaluator's own schedule"""
    assert flush_intervals() == (WIDE_FLUSH, NARROW_FLUSH) == (BR.DOT_FLUSH, MS.flush_interval(True)), "include/sealhip.h"
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    lengths = FLUSH_LENGTHS[narrow]
    rows, second = draw_rows(rng, lengths, source), draw_rows(rng, lengths, count)
    m = make_map(side, rows, second, source, count)
    weight_patterns = ("max", "top", "alternating", "random") if narrow else ("max", "max", "max", "random")
    for pattern, wp in zip(patterns, weight_patterns):
        xc = _columns(side, ci, pattern, rng, (size, source))
        x = np.ascontiguousarray(np.tile(xc, n // 2))
        w = host_weights(side, ci, wp, rng, count, narrow)
        want = np.tile(integers(w, xc, q, rows, second), n // 2)
        got, used = raw(side, ci, w, x, m, slices=1)
        assert used == 1 and np.array_equal(got, want), ("flush, one launch", n, narrow, pattern, wp)
        out = side.ev.dot_scalars_mapped(side.dev_ct(x, ci, True), device_weights(w), count, m, 0, side.scale, narrow)
        assert np.array_equal(out.to_numpy(), want), ("flush, evaluator", n, narrow, pattern, wp)


# ---- cuts
def case_cuts(n, bits, slice_counts=(1, 2, 3, 5, 23), sizes=(1, 3), patterns=("max", "random"), source=SOURCE, count=3, seed=67):
    """rows of 1, 4, 23 and 9 terms in 1, 2, 3, 5 and 23 slices through the raw seam, both forms: most slices of the short rows are
    empty and must store zeros.  Every word equals the sum formed with Python integers, whatever the cut"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    rows, second = draw_rows(rng, CUT_LENGTHS, source), draw_rows(rng, CUT_LENGTHS, count)
    m = make_map(side, rows, second, source, count)
    for narrow in (False, True):
        for pattern in patterns:
            for size in sizes:
                xc = _columns(side, ci, pattern, rng, (size, source))
                x = np.ascontiguousarray(np.tile(xc, n // 2))
                w = host_weights(side, ci, pattern, rng, count, narrow)
                want = np.tile(integers(w, xc, q, rows, second), n // 2)
                for s in slice_counts:
                    assert np.array_equal(raw(side, ci, w, x, m, slices=s)[0], want), ("cut", narrow, pattern, size, s)


def threads(size, rows, K, n):
    """include/sealhip.h: one thread per coefficient pair of a plane, an output item and a prime"""
    return size * rows * K * n // 2


def case_natural_slices(n, bits, source=SOURCE, size=2, seed=71):
    """no forcing: by the documented rule the map of rows 1, 4, 23, 9 (mean 10) is cut - into slices sized from the longest row -
    and a map of the same number of short rows (mean below 8) is not; both slices_used values are asserted from the rule, and the
    words of the library's run are those of the one-launch form, of the evaluator and of DotPlainMapped"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    long_rows, short_rows = draw_rows(rng, CUT_LENGTHS, source), draw_rows(rng, [1, 4, 9, 5], source)
    t = threads(size, len(long_rows), K, n)
    assert IM.rule_mapped(t, long_rows) == 2 and IM.rule_mapped(t, short_rows) == 1, "the premise: mean 10 is cut in two, mean 5 is not"
    x = side.rand_ct(rng, ci, source, size)
    for narrow in (False, True):
        w = weights(side, rng, ci, source, narrow)
        for rows in (long_rows, short_rows):
            m = make_map(side, rows, None, source, source)
            got, used = raw(side, ci, w.host.reshape(-1) if narrow else w.host, x, m)
            assert used == IM.rule_mapped(t, rows), ("the library's rule is the documented one", narrow, used)
            assert np.array_equal(got, raw(side, ci, w.host.reshape(-1) if narrow else w.host, x, m, slices=1)[0]), ("rule and one launch", narrow)
            c = side.dev_ct(x, ci, True)
            out = call(side, w, c, m, source)
            assert np.array_equal(out.to_numpy(), got), "the evaluator's choice"
            same(out, yardstick(side, w, c, m, source), ("natural slices", narrow))


def case_neighbours(scheme, n, bits, size=2, seed=89):
    """the library's own cut and a forced one over the parity map and the depthwise map, with the raw input, weights and result
    inside larger device allocations filled with sentinels: the words are DotPlainMapped's and the sentinel words are intact"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    d_rows, d_second, d_items, d_count = depthwise_rows()
    for rows, second, items, count in ((ROWS, SECOND_OF_3, SOURCE, 3), (d_rows, d_second, d_items, d_count)):
        m = make_map(side, rows, second, items, count)
        x = side.rand_ct(rng, ci, items, size)
        for narrow in (False, True):
            w = weights(side, rng, ci, count, narrow)
            want = yardstick(side, w, side.dev_ct(x, ci, True), m, count).to_numpy()
            for slices in (0, 2):
                got, _ = raw(side, ci, w.host.reshape(-1) if narrow else w.host, x, m, slices=slices, guard=2 * n)
                assert np.array_equal(got, want), ("neighbours", scheme, n, narrow, slices)


# ---- life cycle
def case_out_of_place(scheme, n, bits, size=2, seed=17):
    """the operands are unchanged; a destination that held another size, level, form or context's words is reshaped"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, out = side.first, len(ROWS)
    m = make_map(side, ROWS, SECOND_OF_3, SOURCE, 3)
    foreign = Side(scheme, n, bits)
    for narrow in (False, True):
        x = side.rand_ct(rng, ci, SOURCE, size)
        w = weights(side, rng, ci, 3, narrow)
        want = None
        for dest in (S.Ciphertext(side.ctx, batch=out), side.dev_ct(side.rand_ct(rng, 0, out, 2), 0, True),
                     side.dev_ct(side.rand_ct(rng, ci, out, 4), ci, False), foreign.dev_ct(x[:, :out], ci, True)):
            c = side.dev_ct(x, ci, True)
            got = call(side, w, c, m, 3, destination=dest)
            assert got is dest and np.array_equal(c.to_numpy(), x) and meta(c) == (True, side.scale, side.cf), "the operand changed"
            assert w.unchanged(), "the weights changed"
            assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), size, out)
            if want is None:
                same(dest, yardstick(side, w, c, m, 3), "out of place")
                want = dest.to_numpy(), meta(dest)
            assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], "reshaped destination"


def case_transparent_check(scheme, n, bits):
    """with the check on the RESULT batch is checked: an all-zero second polynomial is refused (and computed with the check off),
    and so are all-zero weights in either form; a proper result passes"""
    side = Side(scheme, n, bits)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    x = side.rand_ct(np.random.default_rng(3), ci, SOURCE, 2)
    x0 = x.copy()
    x0[1] = 0
    m = make_map(side, ROWS, SECOND_OF_3, SOURCE, 3)
    for narrow in (False, True):
        w = weights(side, np.random.default_rng(4), ci, 3, narrow)
        zeros = weights(side, np.random.default_rng(4), ci, 3, narrow)
        zeros.buf = S.DeviceBuffer.from_numpy(np.zeros(3 * K, dtype=np.uint64))
        zero = call(side, w, side.dev_ct(x0, ci, True), m, 3).to_numpy()
        assert not np.any(zero[1]) and np.any(zero[0])
        assert not np.any(call(side, zeros, side.dev_ct(x, ci, True), m, 3).to_numpy())
        side.ev.set_transparent_check(True)
        try:
            _expect(S.LogicError, lambda: call(side, w, side.dev_ct(x0, ci, True), m, 3), "transparent result")
            _expect(S.LogicError, lambda: call(side, zeros, side.dev_ct(x, ci, True), m, 3), "all-zero weights")
            c = side.dev_ct(x, ci, True)
            out = call(side, w, c, m, 3)
        finally:
            side.ev.set_transparent_check(False)
        same(out, yardstick(side, w, c, m, 3), "transparent check on")


def case_pending(n, bits, seed=73):
    """the operand is the result of relinearize with its key-switch tail still deferred, and - in a second call - a tensor product
    that has not been formed; the destination holds a pending product of its own.  The words are those of the eager sequence
    (SEALHIP_LAZY_PRODUCT=0 SEALHIP_KS_EAGER_TAIL=1) and of DotPlainMapped on the settled operands, in both forms"""
    from parity_cases import _Env
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, batch = side.first, 3
    rows, second = [[2], [0, 1, 1]], [[0], [2, 2, 1]]
    m = make_map(side, rows, second, batch, 3)
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    for narrow in (False, True):
        a, b = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)
        z = side.rand_ct(rng, ci, len(rows), 2), side.rand_ct(rng, ci, len(rows), 2)
        w = weights(side, rng, ci, 3, narrow)

        def run():
            ca, cb = side.dev_ct(a, ci, True), side.dev_ct(b, ci, True)
            prod = side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=batch))
            of_product = call(side, w, prod, m, 3)                                                                    # a pending product is formed first
            relin = side.ev.relinearize_inplace(side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=batch)), rlk)   # a deferred tail
            z0, z1 = side.dev_ct(z[0], ci, True), side.dev_ct(z[1], ci, True)   # (alive: a product is formed when an operand goes away)
            dest = side.ev.multiply(z0, z1, S.Ciphertext(side.ctx, batch=len(rows)))                                  # the destination's own
            call(side, w, relin, m, 3, destination=dest)
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
        assert shape == shape_e == (2, len(rows), (True, side.scale ** 3, 1), 3, (True, side.scale ** 3, 1))
        for got, want, what in zip(lazy, eager, ("of a product", "into a pending destination", "product", "relinearized")):
            assert np.array_equal(got, want), (what, narrow)
        saved, side.scale = side.scale, side.scale ** 2   # the operands carry the product's scale
        try:
            for src, got in ((lazy[2], lazy[0]), (lazy[3], lazy[1])):
                assert np.array_equal(yardstick(side, w, side.dev_ct(src, ci, True), m, 3, scale=saved).to_numpy(), got), ("DotPlainMapped", narrow)
        finally:
            side.scale = saved


def case_destroy_after_call(scheme, n, bits, seed=53):
    """a map destroyed right after the call that used it, its block taken again at once: the queued call still reads its lists"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    x = side.rand_ct(rng, ci, SOURCE, 2)
    c = side.dev_ct(x, ci, True)
    w = weights(side, rng, ci, 3, False)
    outs = []
    for trial in range(3):
        order = slice(None, None, -1) if trial == 1 else slice(None)
        m = make_map(side, ROWS[order], SECOND_OF_3[order], SOURCE, 3)
        outs.append(call(side, w, c, m, 3))
        m.destroy()
        assert m._h is None
    same(outs[0], yardstick(side, w, c, make_map(side, ROWS, SECOND_OF_3, SOURCE, 3), 3), "destroyed map")
    same(outs[1], yardstick(side, w, c, make_map(side, ROWS[::-1], SECOND_OF_3[::-1], SOURCE, 3), 3), "destroyed map, reversed")
    assert np.array_equal(outs[2].to_numpy(), outs[0].to_numpy())


def case_capture(n, bits, lengths=(16, 12), source=SOURCE, count=3, size=2, seed=47):
    """CKKS: a cut call (asserted from the documented rule: pool scratch inside the recording) and an uncut one, wide and narrow,
    recorded in a graph and replayed twice with the ciphertext's and the weights' words refreshed in place: each replay equals the
    eager result and DotPlainMapped"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    rows, second = draw_rows(rng, lengths, source), draw_rows(rng, lengths, count)
    assert IM.rule_mapped(threads(size, len(rows), K, n), rows) > 1, "the recorded call over the long rows is cut"
    assert IM.rule_mapped(threads(size, len(ROWS), K, n), ROWS) == 1
    maps = (make_map(side, rows, second, source, count), make_map(side, ROWS, SECOND_OF_3, source, count))
    c = side.dev_ct(side.rand_ct(rng, ci, source, size), ci, True)
    ws = [weights(side, rng, ci, count, narrow) for narrow in (False, True)]
    outs = [[S.Ciphertext(side.ctx, batch=len(r)) for r in (rows, ROWS) for _ in ws] for _ in range(2)]
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        for w in ws:
            fresh = weights(side, rng, ci, count, w.narrow)   # (its own buffers are dropped: the words go into the recorded ones)
            h = np.ascontiguousarray(fresh.host)
            S._native.check(h2d(C.c_void_p(w.buf.ptr), h.ctypes.data_as(C.c_void_p), C.c_uint64(h.nbytes)))
            w.host, w.plain = h, fresh.plain
        x = np.ascontiguousarray(side.rand_ct(rng, ci, source, size))
        S._native.check(h2d(C.c_void_p(c.device_ptr()[0]), x.ctypes.data_as(C.c_void_p), C.c_uint64(x.nbytes)))
        state["x"] = x

    def step(o=outs[0]):
        for i, m in enumerate(maps):
            for j, w in enumerate(ws):
                call(side, w, c, m, count, destination=o[2 * i + j])

    refresh()
    step()   # eager once
    graph = side.ev.capture(step)
    seen = []
    for trial in range(2):
        refresh()
        graph.launch()
        replay = [o.to_numpy() for o in outs[0]]
        step(outs[1])
        for k in range(4):
            assert np.array_equal(replay[k], outs[1][k].to_numpy()) and meta(outs[0][k]) == meta(outs[1][k]), ("graph replay", trial, k)
            assert np.array_equal(replay[k], yardstick(side, ws[k % 2], c, maps[k // 2], count).to_numpy()), ("replay and DotPlainMapped", trial, k)
        assert np.array_equal(c.to_numpy(), state["x"]) and all(w.unchanged() for w in ws), "the operands are only read"
        seen.append(replay[0])
    assert not np.array_equal(seen[0], seen[1]), "the replays saw different operand words"


# ---- errors
def case_errors(scheme, n, bits):
    """every refusal of the contract returns its HRESULT and leaves the destination's words and metadata as they were; a valid call
    afterwards works"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, lib, ev = side.first, S._native.lib(), side.ev._h
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    out = len(ROWS)
    x = side.rand_ct(rng, ci, SOURCE, 2)
    c = side.dev_ct(x, ci, True)
    m = make_map(side, ROWS, SECOND_OF_3, SOURCE, 3)
    dest = side.dev_ct(side.rand_ct(rng, ci, out, 3), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)
    other_side = Side(scheme, n, bits)
    foreign = other_side.dev_ct(x, ci, True)
    foreign_map = make_map(other_side, ROWS, SECOND_OF_3, SOURCE, 3)
    invalid = side.dev_ct(x, ci, True)
    invalid.set_scale(0.0 if scheme == "ckks" else 2.0)   # is_metadata_valid_for fails
    fewer = side.dev_ct(x[:, :SOURCE - 1], ci, True)
    gather7 = S.ItemMap(side.ctx, [[i] for i in range(SOURCE)], SOURCE)

    def call_c(ev_h, ct_h, ptr, count, m_h, flags, scale, dest_h):
        return lib.Evaluator_DotScalarsMapped(ev_h, ct_h, C.c_void_p(ptr), C.c_uint64(count), m_h, C.c_uint64(flags), C.c_double(scale),
                                              dest_h) & 0xFFFFFFFF

    for narrow in (False, True):
        w = weights(side, rng, ci, 3, narrow)
        w7 = weights(side, rng, ci, SOURCE, narrow)
        form = NARROW if narrow else 0
        good = (ev, c._h, w.buf.ptr, 3, m._h, form, side.scale, dest._h)
        for k in (0, 1, 4, 7):
            args = list(good)
            args[k] = None
            assert call_c(*args) == POINTER, ("NULL handle", k)
        for flags in (1, 2, 3, 8, 15, 1 << 8, 1 << 63):
            assert call_c(*good[:5], flags | form, *good[6:]) == INVALID, ("an unknown flag", flags)
        assert call_c(*good[:3], 4, *good[4:]) == INVALID and call_c(*good[:3], 0, *good[4:]) == INVALID, "weight_count != second_batch"
        assert call_c(ev, fewer._h, *good[2:]) == INVALID, "the ciphertext's batch != first_batch"
        assert call_c(*good[:7], S.Ciphertext(side.ctx, batch=out + 1)._h) == INVALID, "the destination's batch != rows"
        assert call_c(ev, c._h, w7.buf.ptr, SOURCE, gather7._h, form, side.scale, c._h) == INVALID, "destination == encrypted"
        assert call_c(ev, c._h, None, *good[3:]) == INVALID, "NULL device_weights"
        assert call_c(ev, c._h, w.buf.ptr + 8, *good[3:]) == INVALID, "misaligned device_weights"
        ptr, _ = c.device_ptr()
        assert call_c(ev, c._h, ptr + 16, *good[3:]) == INVALID, "device_weights inside encrypted"
        ptr, _ = dest.device_ptr()
        assert call_c(ev, c._h, ptr + 16, *good[3:]) == INVALID, "device_weights inside destination"
        for bad, what in ((invalid, "an invalid ciphertext"), (foreign, "a ciphertext of another context"), (side.dev_ct(x, ci, False), "coefficient form")):
            assert call_c(ev, bad._h, *good[2:]) == INVALID, what
        assert call_c(*good[:4], foreign_map._h, *good[5:]) == INVALID, "a map of another context"
        if scheme == "ckks":
            assert call_c(*good[:6], 0.0, dest._h) == INVALID, "CKKS weight scale"
            assert call_c(*good[:6], 2.0 ** 400, dest._h) == INVALID, "scale out of bounds"
        _expect(ValueError, lambda: side.ev.dot_scalars_mapped(c, S.DeviceBuffer(1), 3, m, 0, side.scale, narrow, dest), "too few weight words")
        _expect(ValueError, lambda: side.ev.dot_scalars_mapped(c, w.buf, 3, m, 1, side.scale, narrow, dest), "a flag through Python")
        assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
        assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
        assert np.array_equal(c.to_numpy(), x) and w.unchanged()
    # the raw seam's shape checks
    used = C.c_uint64()
    for size, a_batch, count in ((0, SOURCE, 3), (17, SOURCE, 3), (2, SOURCE - 1, 3), (2, SOURCE, 4)):
        hr = lib.shl_dot_scalars_mapped(side.ctx._h, C.c_uint64(ci), None, C.c_uint64(count), C.c_int(0), None, C.c_uint64(a_batch), None,
                                        C.c_uint64(size), m._h, C.c_uint64(0), None, C.byref(used), None) & 0xFFFFFFFF
        assert hr == INVALID, ("the raw seam's shape", size, a_batch, count)
    # a valid call afterwards
    call(side, w, c, m, 3, destination=dest)
    same(dest, yardstick(side, w, c, m, 3), "after the failures")
