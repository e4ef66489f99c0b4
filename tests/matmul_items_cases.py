"""A matrix of ciphertexts times a matrix of ciphertexts over the items of two batches (Evaluator_MatMulItems; shl_matmul_items),
shared by the CPU (emulated kernels) and `-m gpu` suites.  Exact word equality and the metadata triple everywhere, no tolerances.
The yardsticks: Evaluator_DotItemsMapped over the dense pair map (row i * cols + j names the pairs (i * inner + k, k * cols + j));
the library's unchanged multiply on batches of one and add_many over the products; where oracle/_ref is built, the REAL reference
doing the same on its own objects; and, around the flush interval, across the cuts and for every built tile, Python-integer
arithmetic, which depends on neither library.  Dimensions are written in terms of the tile TR x TC the library reports, so that they
follow a change of tile.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import batch_reduce_cases as BR
import dot_items_cases as DI
from harness import two_pass_ring
from batch_reduce_cases import meta, _columns
from plain_batch_cases import Side, _expect

INNER = 3
FLUSH = DI.DOT_ITEMS_FLUSH
FLUSH_INNERS = [FLUSH - 1, FLUSH, FLUSH + 1, 2 * FLUSH + 3]
# include/sealhip.h (shl_matmul_items_tile): the built tiles and the words of a coefficient row one thread holds
TILES = {(1, 1): 2, (2, 2): 2, (2, 4): 1}
NON_TEMPORAL, CACHED = 1 << 16, 2 << 16


def info():
    """(TR, TC, values of the inner index between two reductions) as the library reports them"""
    r, c, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_matmul_items_info(C.byref(r), C.byref(c), C.byref(f)))
    return r.value, c.value, f.value


def edge(T):
    return sorted({1, T - 1, T, T + 1, 2 * T + 1} - {0})


def shapes():
    """a lone output, a short tile next to a full column tile and a lone column, a full tile, the same the other way round, two
    full tiles and a lone row and column"""
    TR, TC, _ = info()
    return [(1, 1), (TR - 1 or 1, TC + 1), (TR, TC), (TR + 1, TC - 1 or 1), (2 * TR + 1, 2 * TC + 1)]


def tile_id(tr, tc):
    return tr << 8 | tc


def threads(rows, cols, K, n, tile=None):
    """include/sealhip.h: one thread per tile of TR x TC outputs, prime and coefficient pair (2 x 4: coefficient)"""
    tr, tc = info()[:2] if tile is None else tile
    return -(-rows // tr) * -(-cols // tc) * K * n // TILES[(tr, tc)]


# ---- layouts and yardsticks
def transposed(y, inner, cols):
    """y [..][inner * cols][K][N] with item (k, j) at k * cols + j -> the same items stored [cols][inner]"""
    order = [k * cols + j for j in range(cols) for k in range(inner)]
    return np.ascontiguousarray(y[:, order])


def pair_map(side, rows, inner, cols, second_transposed=False):
    first = [[i * inner + k for k in range(inner)] for i in range(rows) for j in range(cols)]
    if second_transposed:
        second = [[j * inner + k for k in range(inner)] for i in range(rows) for j in range(cols)]
    else:
        second = [[k * cols + j for k in range(inner)] for i in range(rows) for j in range(cols)]
    return S.ItemMap(side.ctx, first, rows * inner, second=second, second_batch=inner * cols)


def via_map(side, cx, cy, rows, inner, cols, second_transposed=False):
    return side.ev.dot_items_mapped(cx, cy, pair_map(side, rows, inner, cols, second_transposed))


def check_per_object(side, what, out, x, y, ci, rows, inner, cols):
    """every output item against multiply on batches of one + add_many (and the reference, where it is built)"""
    got = out.to_numpy()
    for i in range(rows):
        for j in range(cols):
            words, m = DI.expect_group(side, x[:, i * inner:(i + 1) * inner], y[:, j::cols], ci)
            assert np.array_equal(got[:, i * cols + j], words), (what, "output item", i, j)
            assert meta(out) == m, (what, "metadata")


def case_parity(scheme, n, bits, ci=None, inner=INNER, shape_list=None, per_object=True, seed=5):
    """the five shapes, both layouts of Y: the words and metadata of DotItemsMapped over the dense pair map; at the largest shape
    also multiply + add_many on batches of one and the reference"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    shape_list = shapes() if shape_list is None else shape_list
    for rows, cols in shape_list:
        x, y = side.rand_ct(rng, ci, rows * inner, 2), side.rand_ct(rng, ci, inner * cols, 2)
        cx, cy, cyt = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), side.dev_ct(transposed(y, inner, cols), ci, True)
        mapped = via_map(side, cx, cy, rows, inner, cols)
        for flag, c2 in ((False, cy), (True, cyt)):
            out = side.ev.matmul_items(cx, c2, rows, inner, cols, flag)
            got = out.to_numpy()
            assert got.shape == (3, rows * cols) + x.shape[2:], (scheme, n, rows, cols, got.shape)
            assert (out.batch(), out.size(), out.parms_id()) == (rows * cols, 3, side.ctx.parms_id_at(ci))
            assert np.array_equal(got, mapped.to_numpy()) and meta(out) == meta(mapped), ("dense pair map", scheme, n, rows, cols, flag)
        assert np.array_equal(out.to_numpy(), via_map(side, cx, cyt, rows, inner, cols, True).to_numpy()), "the map over the stored layout"
        assert np.array_equal(cx.to_numpy(), x) and np.array_equal(cy.to_numpy(), y), "the operands are only read"
        if per_object and (rows, cols) == shape_list[-1]:
            check_per_object(side, (scheme, n), out, x, y, ci, rows, inner, cols)


def case_degenerate(scheme, n, bits, seed=7):
    """rows = cols = 1 is dot_items with group = inner; inner = 1 is multiply on the corresponding batches"""
    TR, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, inner = side.first, 5
    x, y = side.rand_ct(rng, ci, inner, 2), side.rand_ct(rng, ci, inner, 2)
    cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
    want = side.ev.dot_items(cx, cy, inner)
    for flag in (False, True):
        out = side.ev.matmul_items(cx, cy, 1, inner, 1, flag)
        assert np.array_equal(out.to_numpy(), want.to_numpy()) and meta(out) == meta(want), ("dot_items", flag)
    rows, cols = TR + 1, TC + 1
    x, y = side.rand_ct(rng, ci, rows, 2), side.rand_ct(rng, ci, cols, 2)
    xa = np.ascontiguousarray(x[:, [i for i in range(rows) for j in range(cols)]])
    yb = np.ascontiguousarray(y[:, [j for i in range(rows) for j in range(cols)]])
    want = side.ev.multiply(side.dev_ct(xa, ci, True), side.dev_ct(yb, ci, True), S.Ciphertext(side.ctx, batch=rows * cols))
    for flag in (False, True):   # one value of the inner index: both layouts hold the same items
        out = side.ev.matmul_items(side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), rows, 1, cols, flag)
        assert np.array_equal(out.to_numpy(), want.to_numpy()) and meta(out) == meta(want), ("multiply", flag)


def case_same_handle(scheme, n, bits, seed=11):
    """X X^T: the same handle twice with the transposed flag equals the mapped route and is symmetric word for word"""
    TR, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, r, inner = side.first, max(TR, TC) + 1, INNER
    x = side.rand_ct(rng, ci, r * inner, 2)
    cx = side.dev_ct(x, ci, True)
    out = side.ev.matmul_items(cx, cx, r, inner, r, True)
    mapped = via_map(side, cx, cx, r, inner, r, True)
    got = out.to_numpy()
    assert np.array_equal(got, mapped.to_numpy()) and meta(out) == meta(mapped), "dense pair map"
    other = side.ev.matmul_items(cx, side.dev_ct(x, ci, True), r, inner, r, True)
    assert np.array_equal(got, other.to_numpy()) and meta(out) == meta(other), "a copy of x as the second operand"
    g = got.reshape((3, r, r) + got.shape[2:])
    assert np.array_equal(g, g.transpose(0, 2, 1, 3, 4)), "out[i][j] == out[j][i]"
    assert np.array_equal(cx.to_numpy(), x), "the operand is only read"


# ---- the raw seam
def raw(side, ci, x, y, rows, inner, cols, flag=False, slices=0, tile=None, same=False):
    """shl_matmul_items (tile None) / shl_matmul_items_tile on raw words: x [2][rows * inner][K][N], y [2][inner * cols][K][N] in the
    layout `flag` says (same: x's buffer twice) -> (words [3][rows * cols][K][N], slices run)"""
    _, _, K, n = x.shape
    a = S.DeviceBuffer.from_numpy(x)
    b = a if same else S.DeviceBuffer.from_numpy(y)
    r = S.DeviceBuffer(3 * rows * cols * K * n)
    used = C.c_uint64()
    lib = S._native.lib()
    args = (side.ctx._h, C.c_uint64(ci), C.c_void_p(a.ptr), C.c_void_p(b.ptr), C.c_void_p(r.ptr), C.c_uint64(rows), C.c_uint64(inner),
            C.c_uint64(cols), C.c_int(1 if flag else 0), C.c_uint64(slices), C.byref(used))
    if tile is None:
        S._native.check(lib.shl_matmul_items(*args))
    else:
        S._native.check(lib.shl_matmul_items_tile(*args, C.c_uint64(tile), None))
    if slices:
        per = -(-inner // slices)
        assert used.value == -(-inner // per), ("slices run", used.value, slices)
    return r.to_numpy((3, rows * cols, K, n)), used.value   # (the copy back waits for the device)


def natural_slices(side, ci, rows, inner, cols):
    used = C.c_uint64()
    S._native.check(S._native.lib().shl_matmul_items(side.ctx._h, C.c_uint64(ci), None, None, None, C.c_uint64(rows), C.c_uint64(inner),
                                                     C.c_uint64(cols), C.c_int(0), C.c_uint64(0), C.byref(used)))
    return used.value


def integers(xc, yc, q, rows, inner, cols):
    """Python integers: xc [2][rows * inner][K][2], yc [2][inner * cols][K][2] (item (k, j) at k * cols + j) -> [3][rows * cols][K][2]"""
    xo, yo = xc.astype(object), yc.astype(object)
    want = np.zeros((3, rows * cols, len(q), 2), dtype=np.uint64)
    for i in range(rows):
        for j in range(cols):
            xs, ys = slice(i * inner, (i + 1) * inner), slice(j, None, cols)
            for k in range(len(q)):
                x0, x1, y0, y1 = xo[0, xs, k], xo[1, xs, k], yo[0, ys, k], yo[1, ys, k]
                want[0, i * cols + j, k] = ((x0 * y0).sum(axis=0) % q[k]).astype(np.uint64)
                want[1, i * cols + j, k] = ((x0 * y1 + x1 * y0).sum(axis=0) % q[k]).astype(np.uint64)
                want[2, i * cols + j, k] = ((x1 * y1).sum(axis=0) % q[k]).astype(np.uint64)
    return want


def pattern_operands(side, ci, pattern, rng, rows, inner, cols, n):
    """-> (x, y, the Python integers' words); with "max" every word is q - 1: the largest run the accumulators must hold"""
    q = [int(v) for v in side.q(ci)]
    xc = _columns(side, ci, pattern, rng, (2, rows * inner))
    yc = _columns(side, ci, pattern if pattern != "alternating" else "max", rng, (2, inner * cols))
    x, y = np.ascontiguousarray(np.tile(xc, n // 2)), np.ascontiguousarray(np.tile(yc, n // 2))
    return x, y, np.tile(integers(xc, yc, q, rows, inner, cols), n // 2)


def case_flush(n, bits, inners=None, patterns=("max", "alternating", "half", "random"), seed=61):
    """the inner index around the flush interval, TR + 1 rows (a full tile and a short one) and one column, one launch: every word
    equals the sum formed with Python integers - through the raw seam, whose threads add the whole inner index, and for the
    evaluator's own schedule"""
    TR, TC, flush = info()
    assert flush == DI.library_flush_interval() == FLUSH == 128 and FLUSH_INNERS == [127, 128, 129, 259]
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, rows = side.first, TR + 1
    for inner in (FLUSH_INNERS if inners is None else inners):
        for pattern in patterns:
            x, y, want = pattern_operands(side, ci, pattern, rng, rows, inner, 1, n)
            got, used = raw(side, ci, x, y, rows, inner, 1, slices=1)
            assert used == 1 and np.array_equal(got, want), ("flush", n, inner, pattern)
            out = side.ev.matmul_items(side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), rows, inner, 1)
            assert np.array_equal(out.to_numpy(), want), ("flush, evaluator", n, inner, pattern)


def case_cuts(scheme, n, bits, inner=7, slice_counts=(2, 3, 7), seed=67):
    """forced cuts of an inner index of 7 - slice counts that do not divide it among them - at (TR + 1) x (TC + 1): the words of the
    uncut call, which are the mapped route's; the natural slice count is the documented rule's, asked with the tiled thread count"""
    TR, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, cols = side.first, TR + 1, TC + 1
    K = len(side.ctx.coeff_modulus_at(ci))
    assert inner in slice_counts and any(inner % s for s in slice_counts)
    x, y = side.rand_ct(rng, ci, rows * inner, 2), side.rand_ct(rng, ci, inner * cols, 2)
    yt = transposed(y, inner, cols)
    one, used = raw(side, ci, x, y, rows, inner, cols, slices=1)
    assert used == 1
    mapped = via_map(side, side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), rows, inner, cols)
    assert np.array_equal(one, mapped.to_numpy()), "uncut and the dense pair map"
    for s in slice_counts:
        assert np.array_equal(raw(side, ci, x, y, rows, inner, cols, slices=s)[0], one), ("cut", s)
        assert np.array_equal(raw(side, ci, x, yt, rows, inner, cols, True, slices=s)[0], one), ("cut, transposed", s)
    for r, i, c in ((rows, inner, cols), (1, 64, 1), (rows, 64, cols), (4 * rows, 8, 4 * cols)):
        assert natural_slices(side, ci, r, i, c) == BR.rule_slices(threads(r, c, K, n), i), ("the library's rule is the documented one", r, i, c)


def case_natural_slices(scheme, n, bits, inner=23, seed=71):
    """no forcing: a shape the documented rule cuts (asserted from the rule, not assumed) gives the one-launch words through the
    seam and through the evaluator"""
    TR, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, cols = side.first, TR + 1, TC + 1
    K = len(side.ctx.coeff_modulus_at(ci))
    want = BR.rule_slices(threads(rows, cols, K, n), inner)
    assert want > 1, ("the rule does not cut this shape", n, K)
    x, y = side.rand_ct(rng, ci, rows * inner, 2), side.rand_ct(rng, ci, inner * cols, 2)
    got, used = raw(side, ci, x, y, rows, inner, cols)
    assert used == want == natural_slices(side, ci, rows, inner, cols)
    one, _ = raw(side, ci, x, y, rows, inner, cols, slices=1)
    assert np.array_equal(got, one), "rule and one launch"
    out = side.ev.matmul_items(side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), rows, inner, cols)
    assert np.array_equal(out.to_numpy(), one), "the evaluator's choice"


def case_tiles(n, bits, inner=5, seed=83):
    """every tile the library is built with - the rate tool sweeps them -, with and without the non-temporal hint on the operand
    loads, gives the Python integers' words at (2 TR + 1) x (2 TC + 1): both layouts of Y, one launch and cut in two, and the same
    buffer as both operands; a tile that is not built is refused"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    for (tr, tc) in TILES:
        rows, cols = 2 * tr + 1, 2 * tc + 1
        for pattern in ("max", "random"):
            x, y, want = pattern_operands(side, ci, pattern, rng, rows, inner, cols, n)
            yt = transposed(y, inner, cols)
            for hint in (0, NON_TEMPORAL, CACHED):
                for slices in (1, 2):
                    tile = tile_id(tr, tc) | hint
                    got, used = raw(side, ci, x, y, rows, inner, cols, False, slices, tile)
                    assert used == slices and np.array_equal(got, want), ("tile", n, tr, tc, pattern, hint, slices)
                    got, _ = raw(side, ci, x, yt, rows, inner, cols, True, slices, tile)
                    assert np.array_equal(got, want), ("tile, transposed", n, tr, tc, pattern, hint, slices)
        # x == y: a square of rows = cols = 2 tr + 1 against x times a copy of itself
        xc = _columns(side, ci, "random", rng, (2, rows * rows))
        xs = np.ascontiguousarray(np.tile(xc, n // 2))
        want = np.tile(integers(xc, xc, q, rows, rows, rows), n // 2)
        got, _ = raw(side, ci, xs, None, rows, rows, rows, False, 1, tile_id(tr, tc), same=True)
        assert np.array_equal(got, want), ("tile, x == y", n, tr, tc)
    for bad in (tile_id(3, 3), tile_id(4, 2), tile_id(2, 2) | 3 << 16, 1 << 20):
        _expect(S.InvalidArgument, lambda: raw(side, ci, x, y, rows, inner, cols, False, 1, bad), "a tile that is not built")


# ---- life cycle
def case_out_of_place(scheme, n, bits, seed=17):
    """the operands are unchanged; a destination that held another size, level or form is reshaped to size 3 at the operands' level"""
    TR, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, inner, cols = side.first, TR + 1, 2, TC - 1 or 1
    out = rows * cols
    x, y = side.rand_ct(rng, ci, rows * inner, 2), side.rand_ct(rng, ci, inner * cols, 2)
    want = None
    for dest in (S.Ciphertext(side.ctx, batch=out), side.dev_ct(side.rand_ct(rng, 0, out, 2), 0, True),
                 side.dev_ct(side.rand_ct(rng, ci, out, 4), ci, False)):
        cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
        got = side.ev.matmul_items(cx, cy, rows, inner, cols, destination=dest)
        assert got is dest and np.array_equal(cx.to_numpy(), x) and np.array_equal(cy.to_numpy(), y), "an operand changed"
        assert meta(cx) == meta(cy) == (True, side.scale, side.cf)
        assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), 3, out)
        if want is None:
            mapped = via_map(side, cx, cy, rows, inner, cols)
            assert np.array_equal(dest.to_numpy(), mapped.to_numpy()) and meta(dest) == meta(mapped)
            want = dest.to_numpy(), meta(dest)
        assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], "reshaped destination"


def case_transparent_check(scheme, n, bits):
    """with the check on the RESULT batch is checked: an all-zero second and third polynomial is refused (and computed with the
    check off), a proper result passes"""
    side = Side(scheme, n, bits)
    ci, rows, inner, cols = side.first, 2, 2, 1
    x, y = side.rand_ct(np.random.default_rng(3), ci, rows * inner, 2), side.rand_ct(np.random.default_rng(4), ci, inner * cols, 2)
    x0, y0 = x.copy(), y.copy()
    x0[1] = 0
    y0[1] = 0
    zero = side.ev.matmul_items(side.dev_ct(x0, ci, True), side.dev_ct(y0, ci, True), rows, inner, cols).to_numpy()
    assert not np.any(zero[1:]) and np.any(zero[0])
    side.ev.set_transparent_check(True)
    try:
        _expect(S.LogicError, lambda: side.ev.matmul_items(side.dev_ct(x0, ci, True), side.dev_ct(y0, ci, True), rows, inner, cols), "transparent result")
        cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
        out = side.ev.matmul_items(cx, cy, rows, inner, cols)
    finally:
        side.ev.set_transparent_check(False)
    assert np.array_equal(out.to_numpy(), via_map(side, cx, cy, rows, inner, cols).to_numpy())


def case_pending(n, bits, seed=73):
    """operand x is the result of relinearize with its key-switch tail still deferred; operand y is an input of a deferred product
    that has not been formed, and y is overwritten after the call; the destination holds a pending product of its own.  The words
    are those of the eager sequence (SEALHIP_LAZY_PRODUCT=0 SEALHIP_KS_EAGER_TAIL=1) and of the mapped route on the settled operands"""
    from parity_cases import _Env
    TR, TC, _ = info()
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, inner, cols = side.first, TR + 1, 2, 1
    bx, by, out_items = rows * inner, inner * cols, rows * cols
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    a, b = side.rand_ct(rng, ci, bx, 2), side.rand_ct(rng, ci, bx, 2)
    yw, c = side.rand_ct(rng, ci, by, 2), side.rand_ct(rng, ci, by, 2)
    z = side.rand_ct(rng, ci, out_items, 2), side.rand_ct(rng, ci, out_items, 2)

    def run():
        ca, cb, y, cc = side.dev_ct(a, ci, True), side.dev_ct(b, ci, True), side.dev_ct(yw, ci, True), side.dev_ct(c, ci, True)
        x = side.ev.relinearize_inplace(side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=bx)), rlk)     # a deferred tail
        w = side.ev.multiply(y, cc, S.Ciphertext(side.ctx, batch=by))                                        # a deferred product reading y
        z0, z1 = side.dev_ct(z[0], ci, True), side.dev_ct(z[1], ci, True)
        dest = side.ev.multiply(z0, z1, S.Ciphertext(side.ctx, batch=out_items))                             # the destination's own
        side.ev.matmul_items(x, y, rows, inner, cols, destination=dest)
        shape = (dest.size(), dest.batch(), meta(dest))
        side.ev.add_inplace(y, cc)                                                                           # y is overwritten afterwards
        return [v.to_numpy() for v in (dest, x, w, y)], shape

    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT_MIN_WGS=0, SEALHIP_LAZY_PRODUCT=None, SEALHIP_KS_EAGER_TAIL=None):
        tails0, products0 = S.tail_stats(), S.product_stats()
        lazy, shape = run()
        tails1, products1 = S.tail_stats(), S.product_stats()
    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT=0, SEALHIP_KS_EAGER_TAIL=1):
        eager, shape_e = run()
    if two_pass_ring(n):   # the sizes at which the library defers
        assert tails1[1] - tails0[1] >= 1, "matmul_items completed a deferred tail"
        assert products1[1] - products0[1] >= 1, "the product reading y was formed when y was overwritten"
        assert products1[2] - products0[2] >= 1, "the destination's pending product was discarded"
    assert shape == shape_e == (3, out_items, (True, side.scale ** 3, 1))
    for got, want, what in zip(lazy, eager, ("matmul_items", "relinearized x", "the product reading y", "y overwritten")):
        assert np.array_equal(got, want), what
    side.scale, saved = side.scale ** 2, side.scale   # x carries the product's scale
    try:
        cx = side.dev_ct(lazy[1], ci, True)
    finally:
        side.scale = saved
    want = via_map(side, cx, side.dev_ct(yw, ci, True), rows, inner, cols)
    assert np.array_equal(lazy[0], want.to_numpy()) and shape[2] == meta(want), "the mapped route on the settled operands"


def case_capture(n, bits, inner=16, seed=47):
    """CKKS: one call recorded in a graph at a shape the documented rule cuts (pool scratch inside the recording), replayed twice
    with both operands' words refreshed in place: each replay equals the eager result and the mapped route"""
    TR, TC, _ = info()
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, cols = side.first, TR + 1, TC + 1
    K = len(side.ctx.coeff_modulus_at(ci))
    assert BR.rule_slices(threads(rows, cols, K, n), inner) > 1, "the recorded call is cut"
    cx = side.dev_ct(side.rand_ct(rng, ci, rows * inner, 2), ci, True)
    cy = side.dev_ct(side.rand_ct(rng, ci, inner * cols, 2), ci, True)
    outs = [S.Ciphertext(side.ctx, batch=rows * cols) for _ in range(2)]
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        for name, c, batch in (("x", cx, rows * inner), ("y", cy, inner * cols)):
            w = np.ascontiguousarray(side.rand_ct(rng, ci, batch, 2))
            S._native.check(h2d(C.c_void_p(c.device_ptr()[0]), w.ctypes.data_as(C.c_void_p), C.c_uint64(w.nbytes)))
            state[name] = w

    def step(o=outs[0]):
        side.ev.matmul_items(cx, cy, rows, inner, cols, destination=o)

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
        assert np.array_equal(replay, via_map(side, cx, cy, rows, inner, cols).to_numpy()), ("replay and the mapped route", trial)
        assert np.array_equal(cx.to_numpy(), state["x"]) and np.array_equal(cy.to_numpy(), state["y"]), "the operands are only read"
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
    x, y = side.rand_ct(rng, ci, rows * inner, 2), side.rand_ct(rng, ci, inner * cols, 2)
    cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
    dest = side.dev_ct(side.rand_ct(rng, ci, rows * cols, 2), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)

    def call(ev_h, x_h, y_h, r, i, c, flags, dest_h):
        return lib.Evaluator_MatMulItems(ev_h, x_h, y_h, C.c_uint64(r), C.c_uint64(i), C.c_uint64(c), C.c_uint64(flags), dest_h) & 0xFFFFFFFF

    good = (ev, cx._h, cy._h, rows, inner, cols, 0, dest._h)
    for k in (0, 1, 2, 7):
        args = list(good)
        args[k] = None
        assert call(*args) == POINTER, ("NULL handle", k)
    for k in (3, 4, 5):
        args = list(good)
        args[k] = 0
        assert call(*args) == INVALID, ("a zero dimension", k)
        args[k] = 1 << 32
        assert call(*args) == INVALID, ("a dimension beyond 32 bits", k)
        args[k] = 1 << 63
        assert call(*args) == INVALID, ("a dimension beyond 32 bits", k)
    assert call(ev, cx._h, cy._h, 1 << 31, 2, 1, 0, dest._h) == INVALID, "rows * inner >= 2^32"
    assert call(ev, cx._h, cy._h, 1, 2, 1 << 31, 0, dest._h) == INVALID, "inner * cols >= 2^32"
    assert call(ev, cx._h, cy._h, 1 << 16, 1, 1 << 16, 0, dest._h) == INVALID, "rows * cols >= 2^32"
    for flags in (2, 3, 1 << 8, 1 << 63):
        assert call(*good[:6], flags, dest._h) == INVALID, ("an unknown flag", flags)
    assert call(ev, cx._h, cy._h, rows + 1, inner, cols, 0, dest._h) == INVALID, "encrypted1's batch != rows * inner"
    assert call(ev, cx._h, cy._h, rows, inner, cols + 1, 0, dest._h) == INVALID, "encrypted2's batch != inner * cols"
    assert call(ev, cx._h, cy._h, rows * inner, 1, inner * cols, 0, dest._h) == INVALID, "destination's batch != rows * cols"
    assert call(ev, cx._h, cy._h, rows, inner, cols, 0, S.Ciphertext(side.ctx, batch=rows * cols + 1)._h) == INVALID, "destination's batch"
    sq = side.dev_ct(side.rand_ct(rng, ci, 4, 2), ci, True)   # 2 x 2 times 2 x 2 gives a batch of 4: the destination could be an operand
    other = side.dev_ct(side.rand_ct(rng, ci, 4, 2), ci, True)
    assert call(ev, sq._h, other._h, 2, 2, 2, 0, sq._h) == INVALID and call(ev, other._h, sq._h, 2, 2, 2, 0, sq._h) == INVALID, "destination == an operand"
    assert call(ev, sq._h, sq._h, 2, 2, 2, 1, sq._h) == INVALID, "destination == both operands"
    invalid = side.dev_ct(x, ci, True)
    invalid.set_scale(0.0 if scheme == "ckks" else 2.0)   # is_metadata_valid_for fails
    foreign = Side(scheme, n, bits).dev_ct(x, ci, True)
    for bad, what in ((invalid, "an invalid ciphertext"), (foreign, "a ciphertext of another context"),
                      (side.dev_ct(side.rand_ct(rng, ci - 1, rows * inner, 2), ci - 1, True), "mismatched levels"),
                      (side.dev_ct(x, ci, False), "coefficient form"), (side.dev_ct(side.rand_ct(rng, ci, rows * inner, 3), ci, True), "a size other than 2")):
        assert call(ev, bad._h, cy._h, rows, inner, cols, 0, dest._h) == INVALID, (what, "first")
    for bad, what in ((side.dev_ct(side.rand_ct(rng, ci - 1, inner * cols, 2), ci - 1, True), "mismatched levels"),
                      (side.dev_ct(y, ci, False), "coefficient form"), (side.dev_ct(side.rand_ct(rng, ci, inner * cols, 3), ci, True), "a size other than 2")):
        assert call(ev, cx._h, bad._h, rows, inner, cols, 0, dest._h) == INVALID, (what, "second")
    if scheme == "ckks":
        big = side.dev_ct(x, ci, True)
        big.set_scale(2.0 ** 100)   # valid by itself; the product's scale is beyond the level's modulus
        bigy = side.dev_ct(y, ci, True)
        bigy.set_scale(2.0 ** 100)
        assert call(ev, big._h, bigy._h, rows, inner, cols, 0, dest._h) == INVALID, "scale out of bounds"
    assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
    assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
    assert np.array_equal(cx.to_numpy(), x) and np.array_equal(cy.to_numpy(), y)
    # a valid call afterwards
    side.ev.matmul_items(cx, cy, rows, inner, cols, destination=dest)
    mapped = via_map(side, cx, cy, rows, inner, cols)
    assert np.array_equal(dest.to_numpy(), mapped.to_numpy()) and meta(dest) == meta(mapped)


def case_bfv_refused(n, bits):
    """BFV's product rounds per item: the scheme is refused as DotItems refuses it, in either form, with the destination untouched"""
    side = Side("bfv", n, bits)
    rng = np.random.default_rng(37)
    ci = side.first
    x = side.rand_ct(rng, ci, 2, 2)
    dest = side.dev_ct(side.rand_ct(rng, ci, 1, 2), ci, False)
    snapshot = dest.to_numpy()
    for ntt in (False, True):
        c = side.dev_ct(x, ci, ntt)
        hr = S._native.lib().Evaluator_MatMulItems(side.ev._h, c._h, c._h, C.c_uint64(1), C.c_uint64(2), C.c_uint64(1), C.c_uint64(0), dest._h) & 0xFFFFFFFF
        assert hr == S._native.E_INVALIDARG, ("BFV", ntt, hex(hr))
    try:
        side.ev.matmul_items(c, c, 1, 2, 1)
        raise AssertionError("BFV accepted")
    except S.InvalidArgument as e:
        assert "unsupported scheme" in e.message, e.message
    assert np.array_equal(dest.to_numpy(), snapshot) and dest.size() == 2 and not dest.is_ntt_form()


# ---- pipelines (the library's own keys)
def _items(ct):
    """the items of a batch as batches of one"""
    w = ct.to_numpy()
    return [S.Ciphertext.from_numpy(ct.context, np.ascontiguousarray(w[:, b:b + 1]), ct.parms_id(), ct.is_ntt_form(), ct.scale(), ct.correction_factor())
            for b in range(w.shape[1])]


def _composed(ev, ctx, xs, ys, rows, inner, cols):
    """multiply + add_many on batches of one, per output item"""
    outs = []
    for i in range(rows):
        for j in range(cols):
            prods = [ev.multiply(xs[i * inner + k], ys[k * cols + j], S.Ciphertext(ctx)) for k in range(inner)]
            outs.append(ev.add_many(prods, S.Ciphertext(ctx)))
    return outs


def case_pipeline_bgv(n=1024, bits=(40, 40, 40, 60), rows=3, inner=3, cols=2, seed=43):
    """BGV: two small matrices of slot vectors are encoded and encrypted, matmul_items -> relinearize -> decrypt -> decode gives the
    integer matrix product modulo t in every slot, exactly - at parameters at which the per-object composition of the same library
    (multiply, add_many, relinearize per output) decrypts to the same values, which is asserted first"""
    import encrypt_batch_cases as EB
    side = EB.Side("bgv", n, list(bits))
    ev, t = side.d.ev, side.t
    be = S.BatchEncoder(side.ctx)
    rlk = side.kg.create_relin_keys()
    rng = np.random.default_rng(seed)
    a = rng.integers(0, t, (rows * inner, n), dtype=np.uint64)
    b = rng.integers(0, t, (inner * cols, n), dtype=np.uint64)
    want = np.zeros((rows * cols, n), dtype=np.uint64)
    ao, bo = a.astype(object), b.astype(object)
    for i in range(rows):
        for j in range(cols):
            want[i * cols + j] = (sum(ao[i * inner + k] * bo[k * cols + j] for k in range(inner)) % t).astype(np.uint64)
    A = side.enc.encrypt_device(be.encode_device(S.DeviceBuffer.from_numpy(a), rows * inner), rows * inner)
    B = side.enc.encrypt_device(be.encode_device(S.DeviceBuffer.from_numpy(b), inner * cols), inner * cols)
    assert A.is_ntt_form() and B.is_ntt_form()

    def decode(ct):
        coeffs, _ = side.dec.decrypt_batch(ct)
        return be.decode_device(coeffs, ct.batch()).to_numpy((ct.batch(), n))

    composed = _composed(ev, side.ctx, _items(A), _items(B), rows, inner, cols)
    for o, c in enumerate(composed):
        ev.relinearize_inplace(c, rlk)
        assert np.array_equal(decode(c)[0], want[o]), ("the per-object composition decrypts to the product", o)
    R = ev.matmul_items(A, B, rows, inner, cols)
    assert (R.batch(), R.size()) == (rows * cols, 3)
    ev.relinearize_inplace(R, rlk)
    assert R.size() == 2
    got = R.to_numpy()
    for o, c in enumerate(composed):
        assert np.array_equal(got[:, o], c.to_numpy()[:, 0]) and meta(R) == meta(c), ("relinearized words", o)
    assert np.array_equal(decode(R), want), "A B modulo t in every slot"


def case_pipeline_ckks(n, bits, rows=3, inner=2, cols=3, seed=41):
    """CKKS: matmul_items -> relinearize -> rescale_to_next equals, word for word and in its metadata, the per-object composition
    (multiply + add_many per output item) through the same two calls"""
    import encrypt_batch_cases as EB
    side = EB.Side("ckks", n, list(bits))
    ev = side.d.ev
    enc = S.CKKSEncoder(side.ctx)
    rlk = side.kg.create_relin_keys()
    rng = np.random.default_rng(seed)
    pid, slots, scale = side.ctx.first_parms_id(), n // 2, 2.0 ** bits[-2]
    a, b = rng.standard_normal((rows * inner, slots)), rng.standard_normal((inner * cols, slots))
    A = side.enc.encrypt_symmetric_device(enc.encode_device(S.DeviceBuffer.from_array(a), rows * inner, pid, scale), rows * inner, pid, scale)
    B = side.enc.encrypt_symmetric_device(enc.encode_device(S.DeviceBuffer.from_array(b), inner * cols, pid, scale), inner * cols, pid, scale)
    composed = _composed(ev, side.ctx, _items(A), _items(B), rows, inner, cols)
    Bt = S.Ciphertext.from_numpy(side.ctx, transposed(B.to_numpy(), inner, cols), B.parms_id(), True, B.scale(), B.correction_factor())
    for flag, second in ((False, B), (True, Bt)):
        R = ev.matmul_items(A, second, rows, inner, cols, flag)
        summed = R.to_numpy()
        for o, c in enumerate(composed):
            assert np.array_equal(summed[:, o], c.to_numpy()[:, 0]) and meta(R) == meta(c), ("matmul_items", flag, o)
        ev.relinearize_inplace(R, rlk)
        ev.rescale_to_next_inplace(R)
        got = R.to_numpy()
        for o, c in enumerate(composed):
            d = ev.rescale_to_next_inplace(ev.relinearize_inplace(S.Ciphertext.from_numpy(side.ctx, c.to_numpy(), c.parms_id(), True, c.scale(), c.correction_factor()), rlk))
            assert np.array_equal(got[:, o], d.to_numpy()[:, 0]) and meta(R) == meta(d) and R.parms_id() == d.parms_id(), ("rescaled", flag, o)
