"""A 2-D convolution of scalar weights over a grid of ciphertexts, one per (channel, pixel) (Evaluator_Conv2dScalarsItems;
shl_conv2d_scalars), shared by the CPU (emulated kernels) and `-m gpu` suites.  Exact word equality and the metadata triple
everywhere, no tolerances.  The yardsticks: Evaluator_DotPlainMapped over the map of the taps inside the image, on plaintexts each
filled with its weight's K words (it covers padding and stride); Evaluator_MatMulScalarsItems where the shape degenerates (a 1 x 1
kernel; a kernel that is the whole image); the library's unchanged per-object forms on batches of one (the constant plaintext,
multiply_plain_inplace, add_many) and, where oracle/_ref is built, the REAL reference doing the same on its own objects; and, around
the two flush intervals, across the cuts and for every built row tile and hint, Python-integer arithmetic, which depends on neither
library.  The map is built here from the definition of the convolution: it shares no code with the kernel's walk.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import batch_reduce_cases as BR
import dot_scalars_cases as DS
import matmul_scalars_cases as MS
from harness import two_pass_ring
from batch_reduce_cases import meta, _columns
from matmul_scalars_cases import Weights, row_tile, flush_interval, row_counts, INT_MIN, INT_MAX, NARROW, TILES
from plain_batch_cases import Side, _expect
from seal_amd.api import Conv2dShape

FLAGS = (0, 1, 2, 3)    # bit 0: the input is stored channel-last; bit 1: the result is stored channel-last
HINTS = (1, 2)          # include/sealhip.h (shl_conv2d_scalars_tile): operand loads with / without the non-temporal hint
# (C, H, W, kh, kw, sh, sw, ph, pw): the issue's list
SAME_3X3 = (2, 3, 4, 3, 3, 1, 1, 1, 1)        # every corner, edge and interior class of the tap range
ASYMMETRIC = (3, 4, 5, 2, 3, 2, 1, 1, 2)      # asymmetric everything
STRIDE_GAPS = (2, 5, 5, 1, 1, 2, 2, 0, 0)     # a stride larger than the kernel: input items nobody reads
POINTWISE = (3, 2, 3, 1, 1, 1, 1, 0, 0)       # MatMulScalarsItems with cols = 6
WHOLE_IMAGE = (2, 3, 2, 3, 2, 1, 1, 0, 0)     # kernel = the whole image: MatMulScalarsItems with cols = 1
ONE_D = (1, 1, 4, 1, 3, 1, 1, 0, 1)           # a 1-D convolution
# one more than the list: in ASYMMETRIC as listed 4 + 2 - 2 IS divisible by the stride 2, so the remainder has a shape of its own
REMAINDER = (2, 5, 5, 2, 3, 2, 3, 1, 1)       # H + 2 ph - kh = 5 and W + 2 pw - kw = 4 leave a remainder: padded rows and columns no window reaches
GEOMETRIES = (SAME_3X3, ASYMMETRIC, STRIDE_GAPS, POINTWISE, WHOLE_IMAGE, ONE_D, REMAINDER)


def shape_of(geometry, oc):
    c, h, w, kh, kw, sh, sw, ph, pw = geometry
    return Conv2dShape(c, h, w, oc, kh, kw, sh, sw, ph, pw)


def shapes(R):
    """the geometries with the output channels taken in turn from the row counts of the tile"""
    counts = row_counts(R)
    return [shape_of(g, counts[i % len(counts)]) for i, g in enumerate(GEOMETRIES)]


def inner_of(s):
    return s.in_channels * s.kernel_h * s.kernel_w


def in_item(s, c, y, x, last):
    return (y * s.width + x) * s.in_channels + c if last else (c * s.height + y) * s.width + x


def out_item(s, o, y, x, last):
    oh, ow = s.out_size()
    return (y * ow + x) * s.out_channels + o if last else (o * oh + y) * ow + x


def tap_rows(s, flags=0):
    """the definition: for every output item, in the order of the result's layout, the (input item, weight) of its taps inside the image"""
    oh, ow = s.out_size()
    rows = [None] * (s.out_channels * oh * ow)
    for o in range(s.out_channels):
        for y in range(oh):
            for x in range(ow):
                row = []
                for c in range(s.in_channels):
                    for dy in range(s.kernel_h):
                        for dx in range(s.kernel_w):
                            iy, ix = y * s.stride_h + dy - s.pad_h, x * s.stride_w + dx - s.pad_w
                            if 0 <= iy < s.height and 0 <= ix < s.width:
                                row.append((in_item(s, c, iy, ix, flags & 1), o * inner_of(s) + (c * s.kernel_h + dy) * s.kernel_w + dx))
                assert row, "pad < kernel: every output has a tap"
                rows[out_item(s, o, y, x, flags & 2)] = row
    return rows


def threads(size, s, K, n, R):
    """include/sealhip.h: one thread per coefficient pair of a plane, a TILE of R output channels, an output position and a prime"""
    oh, ow = s.out_size()
    return size * -(-s.out_channels // R) * oh * ow * K * n // 2


def channel_last(x, channels):
    """[size][channels * positions]... with item (c, pos) at c * positions + pos -> the same items with (c, pos) at pos * channels + c"""
    size, items = x.shape[:2]
    return np.ascontiguousarray(x.reshape((size, channels, items // channels) + x.shape[2:]).swapaxes(1, 2).reshape(x.shape))


def call(side, w, c, s, flags=0, destination=None, scale=None):
    return side.ev.conv2d_scalars_items(w.buf, c, s, flags, side.scale if scale is None else scale, w.narrow, destination)


def yardstick(side, w, c, s, flags=0, scale=None):
    """Evaluator_DotPlainMapped over the taps inside the image, on the expanded plaintexts"""
    rows = tap_rows(s, flags)
    m = S.ItemMap(side.ctx, [[t[0] for t in r] for r in rows], s.in_channels * s.height * s.width, second=[[t[1] for t in r] for r in rows],
                  second_batch=s.out_channels * inner_of(s))
    return side.ev.dot_plain_mapped(c, w.plain, s.out_channels * inner_of(s), m, side.scale if scale is None else scale)


def degenerate(s):
    """(rows, inner, cols) of the MatMulScalarsItems the shape is, or None; the second: only for a channel-first input"""
    if (s.kernel_h, s.kernel_w, s.stride_h, s.stride_w, s.pad_h, s.pad_w) == (1, 1, 1, 1, 0, 0):
        return (s.out_channels, s.in_channels, s.height * s.width), False
    if (s.kernel_h, s.kernel_w, s.pad_h, s.pad_w) == (s.height, s.width, 0, 0):
        return (s.out_channels, inner_of(s), 1), True
    return None, False


def case_parity(scheme, n, bits, sizes=(2, 3), ci=None, shape_list=None, per_object=True, seed=5):
    """every shape, all four combinations of flag bits 0 and 1, both forms: the words and metadata of DotPlainMapped over the tap
    map; the flags permute items and nothing else; where the shape degenerates MatMulScalarsItems' words; at the largest shape
    (ASYMMETRIC: the most input items) also the per-object forms and the reference"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    for narrow in (False, True):
        for size in sizes:
            for s in (shapes(row_tile(narrow)) if shape_list is None else shape_list):
                oc, oh, ow = s.out_channels, *s.out_size()
                what = (scheme, n, "narrow" if narrow else "wide", size, tuple(getattr(s, f) for f, _ in s._fields_))
                x = side.rand_ct(rng, ci, s.in_channels * s.height * s.width, size)
                w = Weights(side, rng, ci, oc, inner_of(s), narrow)
                c, cl = side.dev_ct(x, ci, True), side.dev_ct(channel_last(x, s.in_channels), ci, True)
                for flags in FLAGS:
                    src = cl if flags & 1 else c
                    out, want = call(side, w, src, s, flags), yardstick(side, w, src, s, flags)
                    got = out.to_numpy()
                    assert got.shape == (size, oc * oh * ow) + x.shape[2:], (what, got.shape)
                    assert (out.batch(), out.size(), out.parms_id()) == (oc * oh * ow, size, side.ctx.parms_id_at(ci))
                    assert np.array_equal(got, want.to_numpy()) and meta(out) == meta(want), ("DotPlainMapped", what, flags)
                    if flags == 0:
                        plain = got
                    else:   # the flags permute items and nothing else
                        assert np.array_equal(got, channel_last(plain, oc) if flags & 2 else plain), ("layout", what, flags)
                    mm, first_only = degenerate(s)
                    if mm and not (first_only and flags & 1):
                        prod = side.ev.matmul_scalars_items(w.buf, src, *mm, flags, side.scale, narrow)
                        assert np.array_equal(got, prod.to_numpy()) and meta(out) == meta(prod), ("MatMulScalarsItems", what, flags)
                assert np.array_equal(c.to_numpy(), x) and w.unchanged(), "the operands are only read"
                if per_object and not narrow and shape_list is None and s.height * s.width == 20:
                    for item, row in enumerate(tap_rows(s)):
                        o = item // (oh * ow)
                        values = [w.values[o][t[1] - o * inner_of(s)] for t in row]
                        words, m = DS.expect_row(side, x[:, [t[0] for t in row]], values, ci)
                        assert np.array_equal(plain[:, item], words) and meta(want) == m, ("per-object forms", what, item)


def case_narrow_equals_wide(scheme, n, bits, size=2, seed=9):
    """integer weights - 0, 1, -1, 2^31 - 1 and -2^31 for CKKS, the ends of the centred range for BFV / BGV, random ones - given
    narrow and given wide as the words the public producers write for them: the same words and metadata, in every layout, on the
    padded 3 x 3 shape"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    for R in sorted({row_tile(True), row_tile(False)}):
        s = shape_of(SAME_3X3, R + 1)
        ints = MS.int_weights(side, rng, s.out_channels, inner_of(s))
        flat = [v for row in ints for v in row]
        assert {0, 1, -1} <= set(flat)
        if scheme == "ckks":
            assert INT_MAX in flat and INT_MIN in flat and all(int(q) > 2 ** 31 for q in side.q(ci)), "the premise"
        wide = MS.produced_words(side, ci, ints)
        assert np.array_equal(wide.to_numpy((len(flat), K)), MS.words_of(side, ci, ints)), "the producers' words are w mod q"
        narrow = S.DeviceBuffer.from_int32(np.array(ints, dtype=np.int32))
        x = side.rand_ct(rng, ci, s.in_channels * s.height * s.width, size)
        c, cl = side.dev_ct(x, ci, True), side.dev_ct(channel_last(x, s.in_channels), ci, True)
        for flags in FLAGS:
            src = cl if flags & 1 else c
            a = side.ev.conv2d_scalars_items(wide, src, s, flags, side.scale)
            b = side.ev.conv2d_scalars_items(narrow, src, s, flags, side.scale, narrow=True)
            assert np.array_equal(a.to_numpy(), b.to_numpy()) and meta(a) == meta(b), ("narrow and wide", scheme, n, R, flags)
        if scheme == "ckks":
            assert meta(b)[1] == side.scale * side.scale


# ---- the raw seam
def c_shape(s):
    return C.byref(s) if s is not None else None


def raw(side, ci, w, x, s, flags=0, slices=0, tile=None, hint=0, guard=0):
    """shl_conv2d_scalars (tile None) / shl_conv2d_scalars_tile on raw words: w [OC * inner][K] uint64 or [OC * inner] int32 (which
    selects the narrow form), x [size][C * H * W][K][N] in the layout flags bit 0 says -> (words [size][OC * OH * OW][K][N] in the
    layout bit 1 says, slices run).  guard: words of a sentinel in front of and behind the input and the result, inside the same
    device allocations; they must be intact afterwards"""
    size, _, K, n = x.shape
    narrow = w.dtype == np.int32
    wb = S.DeviceBuffer.from_int32(w) if narrow else S.DeviceBuffer.from_numpy(w)
    out_words = size * s.out_items() * K * n
    sentinel = np.full(guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    a = S.DeviceBuffer.from_numpy(np.concatenate([sentinel, x.reshape(-1), sentinel]))
    r = S.DeviceBuffer.from_numpy(np.concatenate([sentinel, np.full(out_words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), sentinel]))
    used = C.c_uint64()
    lib = S._native.lib()
    args = (side.ctx._h, C.c_uint64(ci), C.c_void_p(wb.ptr), C.c_void_p(a.ptr + 8 * guard), C.c_void_p(r.ptr + 8 * guard), C.c_uint64(size),
            c_shape(s), C.c_uint64(flags | (NARROW if narrow else 0)), C.c_uint64(slices), C.byref(used))
    if tile is None:
        S._native.check(lib.shl_conv2d_scalars(*args))
    else:
        S._native.check(lib.shl_conv2d_scalars_tile(*args, C.c_uint64(tile), C.c_uint64(hint), None))
    if slices:   # include/sealhip.h: the slices that ceil(inner / slices) terms each leave non-empty
        per = -(-inner_of(s) // slices)
        assert used.value == -(-inner_of(s) // per), ("slices run", used.value, slices)
    back = r.to_numpy(out_words + 2 * guard)   # (the copy back waits for the device)
    if guard:
        assert np.array_equal(back[:guard], sentinel) and np.array_equal(back[-guard:], sentinel), "words next to the result were written"
        assert np.array_equal(a.to_numpy(x.size + 2 * guard), np.concatenate([sentinel, x.reshape(-1), sentinel])), "the input's allocation was written"
    return back[guard:guard + out_words].reshape(size, s.out_items(), K, n), used.value


def query(side, ci, size, s, narrow=False, tile=0, hint=0, slices=0):
    """the seam's answer without a result: -> (HRESULT, slices the library would run)"""
    used = C.c_uint64()
    hr = S._native.lib().shl_conv2d_scalars_tile(side.ctx._h, C.c_uint64(ci), None, None, None, C.c_uint64(size), c_shape(s),
                                                 C.c_uint64(NARROW if narrow else 0), C.c_uint64(slices), C.byref(used), C.c_uint64(tile),
                                                 C.c_uint64(hint), None) & 0xFFFFFFFF
    return hr, used.value


def integers(w, xc, q, s, flags=0):
    """Python integers: w [OC * inner][K] words or [OC * inner] signed integers, xc [size][C * H * W][K][2] in the layout flags bit 0
    says -> [size][OC * OH * OW][K][2] in the layout bit 1 says"""
    xo = xc.astype(object)
    wo = np.array([[int(v)] * len(q) for v in w], dtype=object) if w.ndim == 1 else w.astype(object)
    rows = tap_rows(s, flags)
    want = np.zeros((xc.shape[0], len(rows), len(q), 2), dtype=np.uint64)
    for item, row in enumerate(rows):
        items, weights = [t[0] for t in row], [t[1] for t in row]
        for k in range(len(q)):
            prods = wo[weights, k][None, :, None] * xo[:, items, k]   # [size][taps][2]
            want[:, item, k] = (prods.sum(axis=1) % q[k]).astype(np.uint64)
    return want


def pattern_operands(side, ci, pattern, rng, size, s, n, narrow, flags=0):
    """-> (w, x, the Python integers' words); but for "random" every ciphertext word is q - 1"""
    q = [int(v) for v in side.q(ci)]
    xc = _columns(side, ci, "random" if pattern == "random" else "max", rng, (size, s.in_channels * s.height * s.width))
    w = MS.weight_pattern(side, ci, pattern, rng, s.out_channels, inner_of(s), narrow)
    return w, np.ascontiguousarray(np.tile(xc, n // 2)), np.tile(integers(w, xc, q, s, flags), n // 2)


def flush_channels(narrow):
    """3 x 3 image, 3 x 3 kernel, pad 1: the centre output runs 9 C taps, an edge 6 C, a corner 4 C.  9 C cannot equal the interval
    or its neighbours (256 and 1024 +- 1 are no multiples of 9), so C is the last count with 9 C below the interval, the first with
    9 C above it - the centre crosses, the corners do not - and interval / 4, where the corners run EXACTLY one interval, the edges
    cross once and the centre twice"""
    f = flush_interval(narrow)
    return (f // 9, f // 9 + 1, f // 4)


def case_flush(n, bits, narrow, size=2):
    """all residues q - 1 and the weights at their extremes (q - 1; -2^31 and 2^31 - 1), so that a missed reduction overflows: every
    word equals the count of taps times the product, formed with Python integers - through the raw seam in one launch, whose
    threads run all their taps, and (at the last count) through the evaluator's own schedule"""
    flush, R = flush_interval(narrow), row_tile(narrow)
    assert flush == (1024 if narrow else BR.DOT_FLUSH), "include/sealhip.h"
    side = Side("ckks", n, bits)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    below, above, exact = flush_channels(narrow)
    assert 9 * below < flush < 9 * above and 4 * above < flush, "the centre output crosses the boundary, the corners do not"
    assert 4 * exact == flush < 6 * exact and 2 * flush < 9 * exact < 3 * flush, "the corners end on the boundary"
    for ch in (below, above, exact):
        s = Conv2dShape(ch, 3, 3, R + 1, 3, 3, 1, 1, 1, 1)
        count = np.array([len(r) for r in tap_rows(Conv2dShape(ch, 3, 3, 1, 3, 3, 1, 1, 1, 1))], dtype=object)   # taps of the 9 positions
        assert sorted(set(count)) == [4 * ch, 6 * ch, 9 * ch]
        x = np.ascontiguousarray(np.broadcast_to((side.q(ci) - 1)[None, None, :, None], (size, ch * 9, len(q), n)))
        for value in ((INT_MIN, INT_MAX) if narrow else (None,)):
            if narrow:
                w = np.full(s.out_channels * inner_of(s), value, dtype=np.int32)
            else:
                w = np.ascontiguousarray(np.broadcast_to(side.q(ci) - 1, (s.out_channels * inner_of(s), len(q))))
            want = np.zeros((size, s.out_channels, 9, len(q), n), dtype=np.uint64)
            for k, qk in enumerate(q):
                for pos in range(9):
                    want[:, :, pos, k, :] = int(count[pos]) * (qk - 1) * (value if narrow else qk - 1) % qk
            want = want.reshape(size, s.out_channels * 9, len(q), n)
            got, used = raw(side, ci, w, x, s, slices=1)
            assert used == 1 and np.array_equal(got, want), ("flush", n, narrow, ch, value)
    buf = S.DeviceBuffer.from_int32(w) if narrow else S.DeviceBuffer.from_numpy(w)
    out = side.ev.conv2d_scalars_items(buf, side.dev_ct(x, ci, True), s, 0, side.scale, narrow)
    assert np.array_equal(out.to_numpy(), want), ("flush, evaluator", n, narrow)


def case_cuts(scheme, n, bits, size=2, seed=67):
    """forced cuts through the raw seam - 1, 2, 3 slices, and every count up to 8 on the padded 3 x 3 shape -, both forms: the words of
    the uncut call, which are DotPlainMapped's, in every layout, and slices_used as documented (asserted in raw); more slices than
    terms are refused.  With one channel, a 3 x 3 kernel and pad 1, three slices are the three rows of the kernel: the first is
    entirely outside the image for the top outputs, the last for the bottom ones.  The natural slice count is the documented
    rule's, asked with the tiled thread count"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    for narrow in (False, True):
        R = row_tile(narrow)
        for geometry, counts in (((1, 3, 3, 3, 3, 1, 1, 1, 1), (1, 2, 3)), (SAME_3X3, range(1, 9)), (ASYMMETRIC, (1, 2, 3))):
            s = shape_of(geometry, R + 1)
            if geometry[0] == 1:
                dead = [[t[1] % 9 // 3 for t in row] for row in tap_rows(s)[:3]]
                assert all(0 not in d for d in dead), "slice 0 of 3 (dy = 0) has no live term for the top outputs"
            x = side.rand_ct(rng, ci, s.in_channels * s.height * s.width, size)
            w = Weights(side, rng, ci, s.out_channels, inner_of(s), narrow)
            one, used = raw(side, ci, w.host, x, s, slices=1)
            assert used == 1
            assert np.array_equal(one, yardstick(side, w, side.dev_ct(x, ci, True), s).to_numpy()), "uncut and DotPlainMapped"
            for cut in counts:
                for flags in FLAGS:
                    xs = channel_last(x, s.in_channels) if flags & 1 else x
                    want = channel_last(one, s.out_channels) if flags & 2 else one
                    assert np.array_equal(raw(side, ci, w.host, xs, s, flags, slices=cut, tile=0)[0], want), ("cut", narrow, geometry, cut, flags)
            for bad in (inner_of(s) + 1, 65):
                assert query(side, ci, size, s, narrow, slices=bad)[0] == S._native.E_INVALIDARG, ("more slices than terms, or than 64", bad)
        for s in (shape_of(SAME_3X3, R + 1), shape_of(WHOLE_IMAGE, 1), Conv2dShape(64, 1, 1, R, 1, 1, 1, 1, 0, 0), shape_of(ASYMMETRIC, 4 * R)):
            hr, natural = query(side, ci, size, s, narrow)
            assert hr == 0 and natural == BR.rule_slices(threads(size, s, K, n, R), inner_of(s)), ("the library's rule is the documented one", narrow)


def case_natural_slices(scheme, n, bits, size=2, seed=71):
    """no forcing: a shape the documented rule cuts (asserted from the rule, not assumed) gives the one-launch words through the
    seam and through the evaluator, in both forms; padded, so that slices differ in their live terms"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    for narrow in (False, True):
        R = row_tile(narrow)
        s = Conv2dShape(2, 2, 2, R - 1, 3, 3, 1, 1, 1, 1)   # a short tile alone: few enough threads at N = 8192 for the rule to cut
        want = BR.rule_slices(threads(size, s, K, n, R), inner_of(s))
        assert want > 1, ("the rule does not cut this shape", n, K)
        x = side.rand_ct(rng, ci, s.in_channels * s.height * s.width, size)
        w = Weights(side, rng, ci, s.out_channels, inner_of(s), narrow)
        got, used = raw(side, ci, w.host, x, s)
        assert used == want == query(side, ci, size, s, narrow)[1]
        one, _ = raw(side, ci, w.host, x, s, slices=1)
        assert np.array_equal(got, one), "rule and one launch"
        c = side.dev_ct(x, ci, True)
        assert np.array_equal(call(side, w, c, s).to_numpy(), one), "the evaluator's choice"
        assert np.array_equal(yardstick(side, w, c, s).to_numpy(), one), "DotPlainMapped"


def case_tiles(n, bits, size=2, patterns=("max", "alternating", "random"), seed=83):
    """every row tile the library is built with and both hint choices, in both forms, give the Python integers' words on the padded
    3 x 3 shape at 2 R + 1 output channels (two full tiles and a lone channel) and at R - 1 (a short tile alone): every layout, one
    launch and cut in two, the input and the result inside larger allocations whose other words stay as they were; a tile or a hint
    that is not built is refused"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    for narrow in (False, True):
        for R in TILES:
            for oc in (2 * R + 1, R - 1):
                s = shape_of(SAME_3X3, oc)
                for p, pattern in enumerate(patterns):
                    w, x, want = pattern_operands(side, ci, pattern, rng, size, s, n, narrow)
                    for flags in FLAGS:
                        xs = channel_last(x, s.in_channels) if flags & 1 else x
                        ws = channel_last(want, oc) if flags & 2 else want
                        hint = HINTS[(flags + p) % 2]
                        slices = 1 + (flags // 2 + p) % 2   # one launch and cut in two in turn: every layout and pattern meets both
                        got, used = raw(side, ci, w, xs, s, flags, slices, R, hint, guard=64)
                        assert used == slices and np.array_equal(got, ws), ("tile", n, narrow, R, oc, pattern, flags, hint, slices)
                w, x, want = pattern_operands(side, ci, "random", rng, size, shape_of(ASYMMETRIC, R + 1), n, narrow)
                for hint in HINTS:   # both hints on one problem
                    got, _ = raw(side, ci, w, x, shape_of(ASYMMETRIC, R + 1), 0, 1, R, hint, guard=64)
                    assert np.array_equal(got, want), ("hint", n, narrow, R, hint)
        for bad in (1, 2, 3, 16, 1 << 8 | 4, 1 << 32):
            assert query(side, ci, size, shape_of(SAME_3X3, 3), narrow, bad)[0] == S._native.E_INVALIDARG, ("a row tile that is not built", bad)
        for bad in (3, 1 << 16, 1 << 32):
            assert query(side, ci, size, shape_of(SAME_3X3, 3), narrow, 0, bad)[0] == S._native.E_INVALIDARG, ("a hint that does not exist", bad)


def case_neighbours(scheme, n, bits, size=2, seed=89):
    """the library's own tile, hint and cut over the whole shape list, in every layout, with the raw input and result inside larger
    device allocations filled with a sentinel: the words are DotPlainMapped's and the sentinel words are intact - what a run can
    show of the padding's reads and writes staying inside the batch"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    for narrow in (False, True):
        for s in shapes(row_tile(narrow)):
            x = side.rand_ct(rng, ci, s.in_channels * s.height * s.width, size)
            w = Weights(side, rng, ci, s.out_channels, inner_of(s), narrow)
            want = yardstick(side, w, side.dev_ct(x, ci, True), s).to_numpy()
            for flags in FLAGS:
                xs = channel_last(x, s.in_channels) if flags & 1 else x
                got, _ = raw(side, ci, w.host, xs, s, flags, guard=2 * n)
                assert np.array_equal(got, channel_last(want, s.out_channels) if flags & 2 else want), ("neighbours", narrow, flags)


# ---- life cycle
def case_out_of_place(scheme, n, bits, size=2, seed=17):
    """the operands are unchanged; a destination that held another size, level or form is reshaped to the operand's size and level"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    for narrow in (False, True):
        s = Conv2dShape(2, 2, 2, row_tile(narrow) + 1, 2, 2, 1, 1, 1, 0)
        out = s.out_items()
        x = side.rand_ct(rng, ci, 8, size)
        w = Weights(side, rng, ci, s.out_channels, inner_of(s), narrow)
        want = None
        for dest in (S.Ciphertext(side.ctx, batch=out), side.dev_ct(side.rand_ct(rng, 0, out, 2), 0, True),
                     side.dev_ct(side.rand_ct(rng, ci, out, 4), ci, False)):
            c = side.dev_ct(x, ci, True)
            got = call(side, w, c, s, destination=dest)
            assert got is dest and np.array_equal(c.to_numpy(), x) and meta(c) == (True, side.scale, side.cf), "the operand changed"
            assert w.unchanged(), "the weights changed"
            assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), size, out)
            if want is None:
                plain = yardstick(side, w, c, s)
                assert np.array_equal(dest.to_numpy(), plain.to_numpy()) and meta(dest) == meta(plain)
                want = dest.to_numpy(), meta(dest)
            assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], "reshaped destination"


def case_transparent_check(scheme, n, bits):
    """with the check on the RESULT batch is checked: an all-zero second polynomial is refused (and computed with the check off),
    and so are all-zero weights in either form; a proper result passes"""
    side = Side(scheme, n, bits)
    ci = side.first
    s = Conv2dShape(2, 2, 2, 2, 2, 2, 1, 1, 1, 1)
    K = len(side.ctx.coeff_modulus_at(ci))
    x = side.rand_ct(np.random.default_rng(3), ci, 8, 2)
    x0 = x.copy()
    x0[1] = 0
    for narrow in (False, True):
        w = Weights(side, np.random.default_rng(4), ci, 2, inner_of(s), narrow)
        zeros = Weights(side, np.random.default_rng(4), ci, 2, inner_of(s), narrow)
        zeros.buf = S.DeviceBuffer.from_numpy(np.zeros(2 * inner_of(s) * K, dtype=np.uint64))
        zero = call(side, w, side.dev_ct(x0, ci, True), s).to_numpy()
        assert not np.any(zero[1]) and np.any(zero[0])
        assert not np.any(call(side, zeros, side.dev_ct(x, ci, True), s).to_numpy())
        side.ev.set_transparent_check(True)
        try:
            _expect(S.LogicError, lambda: call(side, w, side.dev_ct(x0, ci, True), s), "transparent result")
            _expect(S.LogicError, lambda: call(side, zeros, side.dev_ct(x, ci, True), s), "all-zero weights")
            c = side.dev_ct(x, ci, True)
            out = call(side, w, c, s)
        finally:
            side.ev.set_transparent_check(False)
        assert np.array_equal(out.to_numpy(), yardstick(side, w, c, s).to_numpy())


def case_pending(n, bits, seed=73):
    """the operand is the result of relinearize with its key-switch tail still deferred, and - in a second call - a tensor product
    that has not been formed; the destination holds a pending product of its own.  The words are those of the eager sequence
    (SEALHIP_LAZY_PRODUCT=0 SEALHIP_KS_EAGER_TAIL=1) and of DotPlainMapped on the settled operands, in both forms"""
    from parity_cases import _Env
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    for narrow in (False, True):
        s = Conv2dShape(1, 2, 2, row_tile(narrow) + 1, 2, 2, 1, 1, 1, 1)
        bx, out_items = 4, s.out_items()
        a, b = side.rand_ct(rng, ci, bx, 2), side.rand_ct(rng, ci, bx, 2)
        z = side.rand_ct(rng, ci, out_items, 2), side.rand_ct(rng, ci, out_items, 2)
        w = Weights(side, rng, ci, s.out_channels, inner_of(s), narrow)

        def run():
            ca, cb = side.dev_ct(a, ci, True), side.dev_ct(b, ci, True)
            prod = side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=bx))
            of_product = call(side, w, prod, s)                                                                    # a pending product is formed first
            relin = side.ev.relinearize_inplace(side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=bx)), rlk)   # a deferred tail
            z0, z1 = side.dev_ct(z[0], ci, True), side.dev_ct(z[1], ci, True)   # (alive: a product is formed when an operand goes away)
            dest = side.ev.multiply(z0, z1, S.Ciphertext(side.ctx, batch=out_items))                               # the destination's own
            call(side, w, relin, s, destination=dest)
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
                assert np.array_equal(yardstick(side, w, side.dev_ct(src, ci, True), s, scale=saved).to_numpy(), got), ("DotPlainMapped", narrow)
        finally:
            side.scale = saved


def case_capture(n, bits, narrow, size=2, seed=47):
    """CKKS: one call recorded in a graph at a padded shape the documented rule cuts (pool scratch inside the recording), replayed
    twice with the ciphertexts' and the weights' words refreshed in place: each replay equals the eager result and DotPlainMapped"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    R = row_tile(narrow)
    ci = side.first
    s = Conv2dShape(2, 2, 2, R, 3, 3, 1, 1, 1, 1)   # one tile of channels, four positions: few enough threads at N = 8192 for the rule to cut
    K = len(side.ctx.coeff_modulus_at(ci))
    assert BR.rule_slices(threads(size, s, K, n, R), inner_of(s)) > 1, "the recorded call is cut"
    items = s.in_channels * s.height * s.width
    c = side.dev_ct(side.rand_ct(rng, ci, items, size), ci, True)
    w = Weights(side, rng, ci, s.out_channels, inner_of(s), narrow)
    outs = [S.Ciphertext(side.ctx, batch=s.out_items()) for _ in range(2)]
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        fresh = Weights(side, rng, ci, s.out_channels, inner_of(s), narrow)   # (its own buffers are dropped: the words go into the recorded ones)
        h = np.ascontiguousarray(fresh.host)
        S._native.check(h2d(C.c_void_p(w.buf.ptr), h.ctypes.data_as(C.c_void_p), C.c_uint64(h.nbytes)))
        w.host, w.plain = h, fresh.plain
        x = np.ascontiguousarray(side.rand_ct(rng, ci, items, size))
        S._native.check(h2d(C.c_void_p(c.device_ptr()[0]), x.ctypes.data_as(C.c_void_p), C.c_uint64(x.nbytes)))
        state["x"] = x

    def step(o=outs[0]):
        call(side, w, c, s, 2, destination=o)

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
        assert np.array_equal(replay, yardstick(side, w, c, s, 2).to_numpy()), ("replay and DotPlainMapped", trial)
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
    good_shape = (2, 3, 3, 3, 2, 2, 1, 1, 1, 1)   # C, H, W, OC, kh, kw, sh, sw, ph, pw -> 4 x 4 outputs
    s = Conv2dShape(*good_shape)
    FIELDS = [f for f, _ in Conv2dShape._fields_]
    x = side.rand_ct(rng, ci, 18, 2)
    c = side.dev_ct(x, ci, True)
    dest = side.dev_ct(side.rand_ct(rng, ci, s.out_items(), 3), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)

    def call_c(ev_h, ptr, ct_h, shape, flags, scale, dest_h):
        return lib.Evaluator_Conv2dScalarsItems(ev_h, C.c_void_p(ptr), ct_h, c_shape(shape), C.c_uint64(flags), C.c_double(scale), dest_h) & 0xFFFFFFFF

    def changed(**fields):
        v = dict(zip(FIELDS, good_shape))
        v.update(fields)
        return Conv2dShape(**v)

    for narrow in (False, True):
        w = Weights(side, rng, ci, s.out_channels, inner_of(s), narrow)
        form = NARROW if narrow else 0
        good = (ev, w.buf.ptr, c._h, s, form, side.scale, dest._h)
        for k in (0, 2, 6):
            args = list(good)
            args[k] = None
            assert call_c(*args) == POINTER, ("NULL handle", k)
        assert call_c(*good[:3], None, *good[4:]) == INVALID, "NULL shape"
        for f in FIELDS[:8]:
            assert call_c(*good[:3], changed(**{f: 0}), *good[4:]) == INVALID, ("an extent or stride of 0", f)
        for f in FIELDS:
            for big in (1 << 32, 1 << 63, (1 << 64) - 1):
                assert call_c(*good[:3], changed(**{f: big}), *good[4:]) == INVALID, ("a field beyond 32 bits", f, big)
        for bad, what in ((changed(pad_h=2), "pad_h >= kernel_h"), (changed(pad_w=2), "pad_w >= kernel_w"), (changed(pad_h=3, pad_w=3), "pad > kernel"),
                          (changed(height=1, kernel_h=4, pad_h=1), "height + 2 pad_h < kernel_h"),
                          (changed(width=1, kernel_w=5, pad_w=1), "width + 2 pad_w < kernel_w"),
                          (changed(in_channels=1 << 16, height=1 << 8, width=1 << 8), "C H W >= 2^32"),
                          (changed(out_channels=1 << 16, height=1 << 8, width=1 << 8), "OC OH OW >= 2^32"),
                          (changed(out_channels=1 << 16, in_channels=1 << 14), "OC inner >= 2^32"),
                          (changed(in_channels=1 << 14, height=1 << 8, width=1 << 8), "the terms of one launch >= 2^32"),
                          (changed(in_channels=3), "the ciphertext's batch != C H W"), (changed(height=4), "the ciphertext's batch != C H W"),
                          (changed(out_channels=4), "the destination's batch != OC OH OW"), (changed(stride_h=2), "the destination's batch != OC OH OW"),
                          (changed(pad_w=0), "the destination's batch != OC OH OW")):
            assert call_c(*good[:3], bad, *good[4:]) == INVALID, what
        for flags in (8, 15, 1 << 8, 1 << 63):
            assert call_c(*good[:4], flags | form, *good[5:]) == INVALID, ("an unknown flag", flags)
        assert call_c(*good[:6], S.Ciphertext(side.ctx, batch=s.out_items() + 1)._h) == INVALID, "the destination's batch"
        same = Conv2dShape(2, 3, 3, 2, 1, 1, 1, 1, 0, 0)   # 18 items in, 18 out
        assert call_c(ev, w.buf.ptr, c._h, same, form, side.scale, c._h) == INVALID, "destination == encrypted"
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
            assert call_c(*good[:5], 0.0, dest._h) == INVALID, "CKKS weight scale"
            assert call_c(*good[:5], 2.0 ** 400, dest._h) == INVALID, "scale out of bounds"
        _expect(ValueError, lambda: side.ev.conv2d_scalars_items(S.DeviceBuffer(2), c, s, 0, side.scale, narrow, dest), "too few weight words")
        _expect(ValueError, lambda: side.ev.conv2d_scalars_items(w.buf, c, s, 4, side.scale, narrow, dest), "the narrow bit is an argument")
        # a result the flat grid refuses: its rows are numbered in 32 bits (asked of the seam, which allocates nothing for a query)
        K, R, big = len(side.ctx.coeff_modulus_at(ci)), row_tile(narrow), 46340
        assert big * big < 1 << 32 <= 16 * K * -(-big // R) * big, "the premise"
        assert query(side, ci, 16, Conv2dShape(1, 1, big, big, 1, 1, 1, 1, 0, 0), narrow)[0] == INVALID, "a result the flat grid refuses"
        assert query(side, ci, 1, Conv2dShape(1, 1, 1, R, 1, 1, 1, 1, 0, 0), narrow) == (0, 1)
        for bad in (None, changed(stride_w=0), changed(pad_h=2), changed(kernel_h=6), changed(in_channels=1 << 32)):
            assert query(side, ci, 2, bad, narrow)[0] == INVALID, "the seam refuses what the call refuses"
        for size in (0, 17):
            assert query(side, ci, size, s, narrow)[0] == INVALID, "the seam's size"
        assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
        assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
        assert np.array_equal(c.to_numpy(), x) and w.unchanged()
    # a valid call afterwards
    call(side, w, c, s, destination=dest)
    plain = yardstick(side, w, c, s)
    assert np.array_equal(dest.to_numpy(), plain.to_numpy()) and meta(dest) == meta(plain)
