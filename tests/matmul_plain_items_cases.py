"""A matrix of plaintexts times a matrix of ciphertexts over the items of a batch (Evaluator_MatMulPlainItems;
shl_matmul_plain_items), shared by the CPU (emulated kernels) and `-m gpu` suites.  Exact word equality and the metadata triple
everywhere, no tolerances.  The yardsticks: Evaluator_DotPlainMapped over the dense map (row i * cols + j names, for k < inner,
ciphertext item k * cols + j and plaintext i * inner + k); multiply_plain_device + sum_items; the library's unchanged
multiply_plain_inplace on batches of one and add_many over the products and, where oracle/_ref is built, the REAL reference doing
the same on its own objects; and, around the flush interval, across the cuts and for every built tile, Python-integer arithmetic,
which depends on neither library.  Dimensions are written in terms of the tile TP x TC the library reports, so that they follow a
change of tile.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import batch_reduce_cases as BR
from harness import two_pass_ring
from batch_reduce_cases import meta, _columns
from plain_batch_cases import Side, _expect

INNER = 3
FLUSH = BR.DOT_FLUSH
FLUSH_INNERS = [FLUSH - 1, FLUSH, FLUSH + 1, 2 * FLUSH + 3]
# include/sealhip.h (shl_matmul_plain_items_tile): the built tiles and the words of a coefficient row one thread holds
TILES = {(1, 1): 2, (2, 4): 1, (4, 4): 1, (4, 8): 1}
NON_TEMPORAL, CACHED = 1 << 16, 2 << 16
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def info():
    """(TP, TC, values of the inner index between two reductions) as the library reports them"""
    r, c, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_matmul_plain_items_info(C.byref(r), C.byref(c), C.byref(f)))
    return r.value, c.value, f.value


def shapes():
    """a lone output, a short tile next to a full column tile and a lone column, a full tile, the same the other way round, two
    full tiles and a lone row and column"""
    TP, TC, _ = info()
    return [(1, 1), (TP - 1 or 1, TC + 1), (TP, TC), (TP + 1, TC - 1 or 1), (2 * TP + 1, 2 * TC + 1)]


def tile_id(tp, tc):
    return tp << 8 | tc


def threads(size, rows, cols, K, n, tile=None):
    """include/sealhip.h: one thread per plane, tile of TP x TC outputs, prime and coefficient (1 x 1: coefficient pair)"""
    tp, tc = info()[:2] if tile is None else tile
    return size * -(-rows // tp) * -(-cols // tc) * K * n // TILES[(tp, tc)]


# ---- layouts and yardsticks
def transposed(x, inner, cols):
    """x [..][inner * cols][K][N] with item (k, j) at k * cols + j -> the same items stored [cols][inner]"""
    return np.ascontiguousarray(x[:, [k * cols + j for j in range(cols) for k in range(inner)]])


def result_transposed(r, rows, cols):
    """r [..][rows * cols][K][N] with item (i, j) at i * cols + j -> the same items stored [cols][rows]"""
    return np.ascontiguousarray(r[:, [i * cols + j for j in range(cols) for i in range(rows)]])


def laid_out(x, want, rows, inner, cols, flags):
    """the ciphertext words as the flags say they are stored and the expected words as the flags say they come out"""
    return (transposed(x, inner, cols) if flags[0] else x), (result_transposed(want, rows, cols) if flags[1] else want)


def dense_map(side, rows, inner, cols, second_transposed=False):
    if second_transposed:
        first = [[j * inner + k for k in range(inner)] for i in range(rows) for j in range(cols)]
    else:
        first = [[k * cols + j for k in range(inner)] for i in range(rows) for j in range(cols)]
    second = [[i * inner + k for k in range(inner)] for i in range(rows) for j in range(cols)]
    return S.ItemMap(side.ctx, first, inner * cols, second=second, second_batch=rows * inner)


def via_map(side, c, buf, rows, inner, cols, second_transposed=False, scale=None):
    return side.ev.dot_plain_mapped(c, buf, rows * inner, dense_map(side, rows, inner, cols, second_transposed),
                                    side.scale if scale is None else scale)


def composed(side, x, pl, ci, rows, inner, cols):
    """multiply_plain_device on the gathered pairs, then sum_items over each output's run of `inner` products"""
    xs = np.ascontiguousarray(x[:, [k * cols + j for i in range(rows) for j in range(cols) for k in range(inner)]])
    ps = np.ascontiguousarray(pl[[i * inner + k for i in range(rows) for j in range(cols) for k in range(inner)]])
    prod = side.ev.multiply_plain_device(side.dev_ct(xs, ci, True), S.DeviceBuffer.from_numpy(ps), True, side.scale)
    return side.ev.sum_items(prod, inner)


def check_per_object(side, what, out, x, pl, ci, rows, inner, cols):
    """every output item against multiply_plain_inplace on batches of one + add_many (and the reference, where it is built)"""
    got = out.to_numpy()
    for i in range(rows):
        for j in range(cols):
            words, m = BR.expect_group(side, x[:, j::cols], pl[i * inner:(i + 1) * inner], ci, True)
            assert np.array_equal(got[:, i * cols + j], words), (what, "output item", i, j)
            assert meta(out) == m, (what, "metadata")


def case_parity(scheme, n, bits, sizes=(2, 3), ci=None, inner=INNER, shape_list=None, per_object=True, seed=5):
    """the five shapes, all four flag combinations: the words and metadata of DotPlainMapped over the dense map (with bit 1 the same
    words, items permuted); at the largest shape also multiply_plain_device + sum_items, and multiply_plain_inplace + add_many on
    batches of one with the reference"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    shape_list = shapes() if shape_list is None else shape_list
    for size in sizes:
        for rows, cols in shape_list:
            x, pl = side.rand_ct(rng, ci, inner * cols, size), side.rand_plain(rng, ci, rows * inner, True)
            buf = S.DeviceBuffer.from_numpy(pl)
            c, ct = side.dev_ct(x, ci, True), side.dev_ct(transposed(x, inner, cols), ci, True)
            mapped = via_map(side, c, buf, rows, inner, cols)
            want = mapped.to_numpy()
            assert np.array_equal(want, via_map(side, ct, buf, rows, inner, cols, True).to_numpy()), "the map over the stored layout"
            for flags in FLAGS:
                out = side.ev.matmul_plain_items(buf, ct if flags[0] else c, rows, inner, cols, side.scale, *flags)
                got = out.to_numpy()
                assert got.shape == (size, rows * cols) + x.shape[2:], (scheme, n, rows, cols, got.shape)
                assert (out.batch(), out.size(), out.parms_id()) == (rows * cols, size, side.ctx.parms_id_at(ci))
                assert np.array_equal(got, laid_out(x, want, rows, inner, cols, flags)[1]), ("dense map", scheme, n, size, rows, cols, flags)
                assert meta(out) == meta(mapped), ("metadata", scheme, n, size, rows, cols, flags)
            assert np.array_equal(c.to_numpy(), x) and np.array_equal(buf.to_numpy(pl.shape), pl), "the operands are only read"
            if per_object and (rows, cols) == shape_list[-1]:
                two = composed(side, x, pl, ci, rows, inner, cols)
                assert np.array_equal(want, two.to_numpy()) and meta(mapped) == meta(two), ("multiply_plain_device + sum_items", scheme, n, size)
                check_per_object(side, (scheme, n, size), mapped, x, pl, ci, rows, inner, cols)


def case_degenerate(scheme, n, bits, size=2, seed=7):
    """rows = cols = 1 is dot_plain_device with group = inner; inner = 1 is multiply_plain_device on the gathered pairs"""
    TP, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, inner = side.first, 5
    x, pl = side.rand_ct(rng, ci, inner, size), side.rand_plain(rng, ci, inner, True)
    c, buf = side.dev_ct(x, ci, True), S.DeviceBuffer.from_numpy(pl)
    want = side.ev.dot_plain_device(c, buf, side.scale, inner)
    for flags in FLAGS:   # one row and one column: every layout holds the same items
        out = side.ev.matmul_plain_items(buf, c, 1, inner, 1, side.scale, *flags)
        assert np.array_equal(out.to_numpy(), want.to_numpy()) and meta(out) == meta(want), ("dot_plain_device", flags)
    rows, cols = TP + 1, TC + 1
    x, pl = side.rand_ct(rng, ci, cols, size), side.rand_plain(rng, ci, rows, True)
    xa = np.ascontiguousarray(x[:, [j for i in range(rows) for j in range(cols)]])
    pa = np.ascontiguousarray(pl[[i for i in range(rows) for j in range(cols)]])
    want = side.ev.multiply_plain_device(side.dev_ct(xa, ci, True), S.DeviceBuffer.from_numpy(pa), True, side.scale)
    buf = S.DeviceBuffer.from_numpy(pl)
    for flag in (False, True):   # one value of the inner index: both layouts of the ciphertexts hold the same items
        out = side.ev.matmul_plain_items(buf, side.dev_ct(x, ci, True), rows, 1, cols, side.scale, flag)
        assert np.array_equal(out.to_numpy(), want.to_numpy()) and meta(out) == meta(want), ("multiply_plain_device", flag)


# ---- the raw seam
def raw(side, ci, pl, x, rows, inner, cols, flags=(False, False), slices=0, tile=None):
    """shl_matmul_plain_items (tile None) / shl_matmul_plain_items_tile on raw words: pl [rows * inner][K][N], x [size][inner *
    cols][K][N] in the layout flags[0] says -> (words [size][rows * cols][K][N] in the layout flags[1] says, slices run)"""
    size, _, K, n = x.shape
    p, a = S.DeviceBuffer.from_numpy(pl), S.DeviceBuffer.from_numpy(x)
    r = S.DeviceBuffer(size * rows * cols * K * n)
    used = C.c_uint64()
    lib = S._native.lib()
    args = (side.ctx._h, C.c_uint64(ci), C.c_void_p(p.ptr), C.c_void_p(a.ptr), C.c_void_p(r.ptr), C.c_uint64(size), C.c_uint64(rows),
            C.c_uint64(inner), C.c_uint64(cols), C.c_uint64((1 if flags[0] else 0) | (2 if flags[1] else 0)), C.c_uint64(slices), C.byref(used))
    if tile is None:
        S._native.check(lib.shl_matmul_plain_items(*args))
    else:
        S._native.check(lib.shl_matmul_plain_items_tile(*args, C.c_uint64(tile), None))
    if slices:
        per = -(-inner // slices)
        assert used.value == -(-inner // per), ("slices run", used.value, slices)
    return r.to_numpy((size, rows * cols, K, n)), used.value   # (the copy back waits for the device)


def query(side, ci, size, rows, inner, cols, tile=0):
    """the seam's answer without a result: -> (HRESULT, slices the library would run)"""
    used = C.c_uint64()
    hr = S._native.lib().shl_matmul_plain_items_tile(side.ctx._h, C.c_uint64(ci), None, None, None, C.c_uint64(size), C.c_uint64(rows),
                                                     C.c_uint64(inner), C.c_uint64(cols), C.c_uint64(0), C.c_uint64(0), C.byref(used),
                                                     C.c_uint64(tile), None) & 0xFFFFFFFF
    return hr, used.value


def natural_slices(side, ci, size, rows, inner, cols):
    hr, used = query(side, ci, size, rows, inner, cols)
    assert hr == 0, hex(hr)
    return used


def integers(pc, xc, q, rows, inner, cols):
    """Python integers: pc [rows * inner][K][2], xc [size][inner * cols][K][2] (item (k, j) at k * cols + j) -> [size][rows * cols][K][2]"""
    po, xo = pc.astype(object), xc.astype(object)
    want = np.zeros((xc.shape[0], rows * cols, len(q), 2), dtype=np.uint64)
    for i in range(rows):
        for j in range(cols):
            for k in range(len(q)):
                prods = po[None, i * inner:(i + 1) * inner, k] * xo[:, j::cols, k]   # [size][inner][2]
                want[:, i * cols + j, k] = (prods.sum(axis=1) % q[k]).astype(np.uint64)
    return want


def pattern_operands(side, ci, pattern, rng, size, rows, inner, cols, n):
    """-> (pl, x, the Python integers' words); with "max" every word is q - 1: the largest run the accumulators must hold"""
    q = [int(v) for v in side.q(ci)]
    xc = _columns(side, ci, pattern, rng, (size, inner * cols))
    pc = _columns(side, ci, pattern if pattern != "alternating" else "max", rng, (rows * inner,))
    pl, x = np.ascontiguousarray(np.tile(pc, n // 2)), np.ascontiguousarray(np.tile(xc, n // 2))
    return pl, x, np.tile(integers(pc, xc, q, rows, inner, cols), n // 2)


def case_flush(n, bits, inners=None, patterns=("max", "alternating", "half", "random"), size=2, seed=61):
    """the inner index around the flush interval, TP + 1 rows (a full tile and a short one) and one column, one launch: every word
    equals the sum formed with Python integers - through the raw seam, whose threads add the whole inner index, and for the
    evaluator's own schedule"""
    TP, TC, flush = info()
    assert flush == BR.library_flush_intervals()[1] == FLUSH == 256 and FLUSH_INNERS == [255, 256, 257, 515]
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, rows = side.first, TP + 1
    for inner in (FLUSH_INNERS if inners is None else inners):
        for pattern in patterns:
            pl, x, want = pattern_operands(side, ci, pattern, rng, size, rows, inner, 1, n)
            got, used = raw(side, ci, pl, x, rows, inner, 1, slices=1)
            assert used == 1 and np.array_equal(got, want), ("flush", n, inner, pattern)
            out = side.ev.matmul_plain_items(S.DeviceBuffer.from_numpy(pl), side.dev_ct(x, ci, True), rows, inner, 1, side.scale)
            assert np.array_equal(out.to_numpy(), want), ("flush, evaluator", n, inner, pattern)


def case_cuts(scheme, n, bits, inner=7, slice_counts=(2, 3, 7), size=2, seed=67):
    """forced cuts of an inner index of 7 - slice counts that do not divide it among them - at (TP + 1) x (TC + 1): the words of the
    uncut call, which are the mapped route's, in both ciphertext layouts; the natural slice count is the documented rule's, asked
    with the tiled thread count"""
    TP, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, cols = side.first, TP + 1, TC + 1
    K = len(side.ctx.coeff_modulus_at(ci))
    assert inner in slice_counts and any(inner % s for s in slice_counts)
    x, pl = side.rand_ct(rng, ci, inner * cols, size), side.rand_plain(rng, ci, rows * inner, True)
    xt = transposed(x, inner, cols)
    one, used = raw(side, ci, pl, x, rows, inner, cols, slices=1)
    assert used == 1
    mapped = via_map(side, side.dev_ct(x, ci, True), S.DeviceBuffer.from_numpy(pl), rows, inner, cols)
    assert np.array_equal(one, mapped.to_numpy()), "uncut and the dense map"
    for s in slice_counts:
        assert np.array_equal(raw(side, ci, pl, x, rows, inner, cols, slices=s)[0], one), ("cut", s)
        assert np.array_equal(raw(side, ci, pl, xt, rows, inner, cols, (True, False), slices=s)[0], one), ("cut, transposed", s)
    for r, i, c in ((rows, inner, cols), (1, 64, 1), (rows, 64, cols), (4 * rows, 8, 4 * cols)):
        assert natural_slices(side, ci, size, r, i, c) == BR.rule_slices(threads(size, r, c, K, n), i), ("the library's rule is the documented one", r, i, c)


def case_natural_slices(scheme, n, bits, inner=23, size=2, seed=71):
    """no forcing: a shape the documented rule cuts (asserted from the rule, not assumed) gives the one-launch words through the
    seam and through the evaluator"""
    TP, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, cols = side.first, TP, TC + 1   # one row of tiles: few enough threads at N = 8192 for the rule to cut
    K = len(side.ctx.coeff_modulus_at(ci))
    want = BR.rule_slices(threads(size, rows, cols, K, n), inner)
    assert want > 1, ("the rule does not cut this shape", n, K)
    x, pl = side.rand_ct(rng, ci, inner * cols, size), side.rand_plain(rng, ci, rows * inner, True)
    got, used = raw(side, ci, pl, x, rows, inner, cols)
    assert used == want == natural_slices(side, ci, size, rows, inner, cols)
    one, _ = raw(side, ci, pl, x, rows, inner, cols, slices=1)
    assert np.array_equal(got, one), "rule and one launch"
    out = side.ev.matmul_plain_items(S.DeviceBuffer.from_numpy(pl), side.dev_ct(x, ci, True), rows, inner, cols, side.scale)
    assert np.array_equal(out.to_numpy(), one), "the evaluator's choice"


def case_tiles(n, bits, inner=5, size=2, patterns=("max", "random"), seed=83):
    """every tile the library is built with - the rate tool sweeps them -, with, without and with the default hint on the operand
    loads, gives the Python integers' words at (2 TP + 1) x (2 TC + 1): both layouts of the ciphertexts and of the result, one
    launch and cut in two; a tile that is not built is refused"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    for (tp, tc) in TILES:
        rows, cols = 2 * tp + 1, 2 * tc + 1
        for pattern in patterns:
            pl, x, want = pattern_operands(side, ci, pattern, rng, size, rows, inner, cols, n)
            for f, flags in enumerate(FLAGS):
                xs, ws = laid_out(x, want, rows, inner, cols, flags)
                for h, hint in enumerate((0, NON_TEMPORAL, CACHED)):
                    # one launch and cut in two in turn: every layout and every hint meets both, the two patterns swap them
                    slices = 1 + (f + h + (pattern == "max")) % 2
                    got, used = raw(side, ci, pl, xs, rows, inner, cols, flags, slices, tile_id(tp, tc) | hint)
                    assert used == slices and np.array_equal(got, ws), ("tile", n, tp, tc, pattern, flags, hint, slices)
    for bad in (tile_id(3, 3), tile_id(2, 2), tile_id(8, 4), tile_id(4, 4) | 3 << 16, 1 << 20, 1 << 32):
        assert query(side, ci, size, rows, inner, cols, bad)[0] == S._native.E_INVALIDARG, ("a tile that is not built", hex(bad))


# ---- life cycle
def case_out_of_place(scheme, n, bits, size=2, seed=17):
    """the operands are unchanged; a destination that held another size, level or form is reshaped to the operand's size and level"""
    TP, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, inner, cols = side.first, TP + 1, 2, TC - 1 or 1
    out = rows * cols
    x, pl = side.rand_ct(rng, ci, inner * cols, size), side.rand_plain(rng, ci, rows * inner, True)
    buf = S.DeviceBuffer.from_numpy(pl)
    want = None
    for dest in (S.Ciphertext(side.ctx, batch=out), side.dev_ct(side.rand_ct(rng, 0, out, 2), 0, True),
                 side.dev_ct(side.rand_ct(rng, ci, out, 4), ci, False)):
        c = side.dev_ct(x, ci, True)
        got = side.ev.matmul_plain_items(buf, c, rows, inner, cols, side.scale, destination=dest)
        assert got is dest and np.array_equal(c.to_numpy(), x) and meta(c) == (True, side.scale, side.cf), "the operand changed"
        assert np.array_equal(buf.to_numpy(pl.shape), pl), "the plaintexts changed"
        assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), size, out)
        if want is None:
            mapped = via_map(side, c, buf, rows, inner, cols)
            assert np.array_equal(dest.to_numpy(), mapped.to_numpy()) and meta(dest) == meta(mapped)
            want = dest.to_numpy(), meta(dest)
        assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], "reshaped destination"


def case_transparent_check(scheme, n, bits):
    """with the check on the RESULT batch is checked: an all-zero second polynomial is refused (and computed with the check off),
    and so are all-zero plaintexts; a proper result passes"""
    side = Side(scheme, n, bits)
    ci, rows, inner, cols = side.first, 2, 2, 1
    x = side.rand_ct(np.random.default_rng(3), ci, inner * cols, 2)
    pl = side.rand_plain(np.random.default_rng(4), ci, rows * inner, True)
    x0 = x.copy()
    x0[1] = 0
    buf, zeros = S.DeviceBuffer.from_numpy(pl), S.DeviceBuffer.from_numpy(np.zeros_like(pl))
    zero = side.ev.matmul_plain_items(buf, side.dev_ct(x0, ci, True), rows, inner, cols, side.scale).to_numpy()
    assert not np.any(zero[1]) and np.any(zero[0])
    assert not np.any(side.ev.matmul_plain_items(zeros, side.dev_ct(x, ci, True), rows, inner, cols, side.scale).to_numpy())
    side.ev.set_transparent_check(True)
    try:
        _expect(S.LogicError, lambda: side.ev.matmul_plain_items(buf, side.dev_ct(x0, ci, True), rows, inner, cols, side.scale), "transparent result")
        _expect(S.LogicError, lambda: side.ev.matmul_plain_items(zeros, side.dev_ct(x, ci, True), rows, inner, cols, side.scale), "all-zero plaintexts")
        c = side.dev_ct(x, ci, True)
        out = side.ev.matmul_plain_items(buf, c, rows, inner, cols, side.scale)
    finally:
        side.ev.set_transparent_check(False)
    assert np.array_equal(out.to_numpy(), via_map(side, c, buf, rows, inner, cols).to_numpy())


def case_pending(n, bits, seed=73):
    """the operand is the result of relinearize with its key-switch tail still deferred, and - in a second call - a tensor product
    that has not been formed; the destination holds a pending product of its own.  The words are those of the eager sequence
    (SEALHIP_LAZY_PRODUCT=0 SEALHIP_KS_EAGER_TAIL=1) and of the mapped route on the settled operands"""
    from parity_cases import _Env
    TP, TC, _ = info()
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, inner, cols = side.first, TP + 1, 2, 1
    bx, out_items = inner * cols, rows * cols
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    a, b = side.rand_ct(rng, ci, bx, 2), side.rand_ct(rng, ci, bx, 2)
    z = side.rand_ct(rng, ci, out_items, 2), side.rand_ct(rng, ci, out_items, 2)
    pl = side.rand_plain(rng, ci, rows * inner, True)
    buf = S.DeviceBuffer.from_numpy(pl)

    def run():
        ca, cb = side.dev_ct(a, ci, True), side.dev_ct(b, ci, True)
        prod = side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=bx))
        of_product = side.ev.matmul_plain_items(buf, prod, rows, inner, cols, side.scale)                     # a pending product is formed first
        relin = side.ev.relinearize_inplace(side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=bx)), rlk)   # a deferred tail
        z0, z1 = side.dev_ct(z[0], ci, True), side.dev_ct(z[1], ci, True)   # (alive: a product is formed when an operand goes away)
        dest = side.ev.multiply(z0, z1, S.Ciphertext(side.ctx, batch=out_items))                               # the destination's own
        side.ev.matmul_plain_items(buf, relin, rows, inner, cols, side.scale, destination=dest)
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
        assert np.array_equal(got, want), what
    saved, side.scale = side.scale, side.scale ** 2   # the operands carry the product's scale
    try:
        for src, got in ((lazy[2], lazy[0]), (lazy[3], lazy[1])):
            assert np.array_equal(via_map(side, side.dev_ct(src, ci, True), buf, rows, inner, cols, scale=saved).to_numpy(), got), "the mapped route"
    finally:
        side.scale = saved


def case_capture(n, bits, inner=16, size=2, seed=47):
    """CKKS: one call recorded in a graph at a shape the documented rule cuts (pool scratch inside the recording), replayed twice
    with the ciphertexts' and the plaintexts' words refreshed in place: each replay equals the eager result and the mapped route"""
    TP, TC, _ = info()
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, rows, cols = side.first, TP, TC + 1   # one row of tiles: few enough threads at N = 8192 for the rule to cut
    K = len(side.ctx.coeff_modulus_at(ci))
    assert BR.rule_slices(threads(size, rows, cols, K, n), inner) > 1, "the recorded call is cut"
    c = side.dev_ct(side.rand_ct(rng, ci, inner * cols, size), ci, True)
    buf = S.DeviceBuffer(rows * inner * K * n)
    outs = [S.Ciphertext(side.ctx, batch=rows * cols) for _ in range(2)]
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        p = np.ascontiguousarray(side.rand_plain(rng, ci, rows * inner, True))
        S._native.check(h2d(C.c_void_p(buf.ptr), p.ctypes.data_as(C.c_void_p), C.c_uint64(p.nbytes)))
        w = np.ascontiguousarray(side.rand_ct(rng, ci, inner * cols, size))
        S._native.check(h2d(C.c_void_p(c.device_ptr()[0]), w.ctypes.data_as(C.c_void_p), C.c_uint64(w.nbytes)))
        state["p"], state["x"] = p, w

    def step(o=outs[0]):
        side.ev.matmul_plain_items(buf, c, rows, inner, cols, side.scale, True, True, destination=o)

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
        want = via_map(side, c, buf, rows, inner, cols, True).to_numpy()
        assert np.array_equal(replay, result_transposed(want, rows, cols)), ("replay and the mapped route", trial)
        assert np.array_equal(c.to_numpy(), state["x"]) and np.array_equal(buf.to_numpy(state["p"].shape), state["p"]), "the operands are only read"
        seen.append(replay)
    assert not np.array_equal(seen[0], seen[1]), "the replays saw different operand words"


# ---- errors
def case_errors(scheme, n, bits):
    """every refusal of the contract returns its HRESULT and leaves the destination's words and metadata as they were; a valid call
    afterwards works"""
    TP, TC, _ = info()
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, lib, ev = side.first, S._native.lib(), side.ev._h
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    rows, inner, cols = 3, 2, 2
    x, pl = side.rand_ct(rng, ci, inner * cols, 2), side.rand_plain(rng, ci, rows * inner, True)
    c, buf = side.dev_ct(x, ci, True), S.DeviceBuffer.from_numpy(pl)
    dest = side.dev_ct(side.rand_ct(rng, ci, rows * cols, 3), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)

    def call(ev_h, ptr, ct_h, r, i, cc, flags, scale, dest_h):
        return lib.Evaluator_MatMulPlainItems(ev_h, C.c_void_p(ptr), ct_h, C.c_uint64(r), C.c_uint64(i), C.c_uint64(cc), C.c_uint64(flags),
                                              C.c_double(scale), dest_h) & 0xFFFFFFFF

    good = (ev, buf.ptr, c._h, rows, inner, cols, 0, side.scale, dest._h)
    for k in (0, 2, 8):
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
    assert call(ev, buf.ptr, c._h, 1 << 31, 2, 1, 0, side.scale, dest._h) == INVALID, "rows * inner >= 2^32"
    assert call(ev, buf.ptr, c._h, 1, 2, 1 << 31, 0, side.scale, dest._h) == INVALID, "inner * cols >= 2^32"
    assert call(ev, buf.ptr, c._h, 1 << 16, 1, 1 << 16, 0, side.scale, dest._h) == INVALID, "rows * cols >= 2^32"
    for flags in (4, 7, 1 << 8, 1 << 63):
        assert call(*good[:6], flags, *good[7:]) == INVALID, ("an unknown flag", flags)
    assert call(ev, buf.ptr, c._h, rows, inner, cols + 1, 0, side.scale, dest._h) == INVALID, "the ciphertext's batch != inner * cols"
    assert call(ev, buf.ptr, c._h, rows, inner + 1, cols, 0, side.scale, dest._h) == INVALID, "the ciphertext's batch != inner * cols"
    assert call(ev, buf.ptr, c._h, rows + 1, inner, cols, 0, side.scale, dest._h) == INVALID, "the destination's batch != rows * cols"
    assert call(*good[:8], S.Ciphertext(side.ctx, batch=rows * cols + 1)._h) == INVALID, "the destination's batch"
    assert call(ev, buf.ptr, c._h, 2, 2, 2, 0, side.scale, c._h) == INVALID, "destination == encrypted"
    assert call(ev, None, *good[2:]) == INVALID, "NULL device_plain"
    assert call(ev, buf.ptr + 8, *good[2:]) == INVALID, "misaligned device_plain"
    ptr, _ = c.device_ptr()
    assert call(ev, ptr + 16, *good[2:]) == INVALID, "device_plain inside encrypted"
    ptr, _ = dest.device_ptr()
    assert call(ev, ptr + 16, *good[2:]) == INVALID, "device_plain inside destination"
    invalid = side.dev_ct(x, ci, True)
    invalid.set_scale(0.0 if scheme == "ckks" else 2.0)   # is_metadata_valid_for fails
    foreign = Side(scheme, n, bits).dev_ct(x, ci, True)
    for bad, what in ((invalid, "an invalid ciphertext"), (foreign, "a ciphertext of another context"), (side.dev_ct(x, ci, False), "coefficient form")):
        assert call(ev, buf.ptr, bad._h, *good[3:]) == INVALID, what
    if scheme == "ckks":
        assert call(*good[:7], 0.0, dest._h) == INVALID, "CKKS plaintext scale"
        assert call(*good[:7], 2.0 ** 400, dest._h) == INVALID, "scale out of bounds"
    _expect(ValueError, lambda: side.ev.matmul_plain_items(S.DeviceBuffer(pl.size - 1), c, rows, inner, cols, side.scale, destination=dest), "too few plaintext words")
    # a result the flat grid refuses: its rows are numbered in 32 bits (asked of the seam, which allocates nothing for a query)
    K, big = len(side.ctx.coeff_modulus_at(ci)), 46340
    assert big * big < 1 << 32 <= 16 * K * -(-big // TP) * -(-big // TC), "the premise"
    assert query(side, ci, 16, big, 1, big)[0] == INVALID, "a result the flat grid refuses"
    assert query(side, ci, 1, TP, 1, TC) == (0, 1)
    assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
    assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
    assert np.array_equal(c.to_numpy(), x) and np.array_equal(buf.to_numpy(pl.shape), pl)
    # a valid call afterwards
    side.ev.matmul_plain_items(buf, c, rows, inner, cols, side.scale, destination=dest)
    mapped = via_map(side, c, buf, rows, inner, cols)
    assert np.array_equal(dest.to_numpy(), mapped.to_numpy()) and meta(dest) == meta(mapped)


# ---- pipelines (the library's own keys and encoders)
def _items(ct):
    """the items of a batch as batches of one"""
    w = ct.to_numpy()
    return [S.Ciphertext.from_numpy(ct.context, np.ascontiguousarray(w[:, b:b + 1]), ct.parms_id(), ct.is_ntt_form(), ct.scale(), ct.correction_factor())
            for b in range(w.shape[1])]


def _composed(ev, ctx, plains, xs, rows, inner, cols):
    """multiply_plain + add_many on batches of one, per output item"""
    outs = []
    for i in range(rows):
        for j in range(cols):
            prods = [ev.multiply_plain(xs[k * cols + j], plains[i * inner + k], S.Ciphertext(ctx)) for k in range(inner)]
            outs.append(ev.add_many(prods, S.Ciphertext(ctx)))
    return outs


def case_pipeline_bgv(n=1024, bits=(40, 40, 40, 60), rows=3, inner=3, cols=2, seed=43):
    """BGV: a matrix of slot vectors is encoded and lifted to NTT form, another encoded and encrypted; matmul_plain_items ->
    decrypt -> decode gives the integer matrix product modulo t in every slot, exactly - at parameters at which the per-object
    composition of the same library (multiply_plain, add_many per output) decrypts to the same values, which is asserted first"""
    import encrypt_batch_cases as EB
    side = EB.Side("bgv", n, list(bits))
    ev, t = side.d.ev, side.t
    be = S.BatchEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    p = rng.integers(0, t, (rows * inner, n), dtype=np.uint64)
    b = rng.integers(0, t, (inner * cols, n), dtype=np.uint64)
    want = np.zeros((rows * cols, n), dtype=np.uint64)
    po, bo = p.astype(object), b.astype(object)
    for i in range(rows):
        for j in range(cols):
            want[i * cols + j] = (sum(po[i * inner + k] * bo[k * cols + j] for k in range(inner)) % t).astype(np.uint64)
    B = side.enc.encrypt_device(be.encode_device(S.DeviceBuffer.from_numpy(b), inner * cols), inner * cols)
    assert B.is_ntt_form()
    K = B.coeff_modulus_size()
    P = ev.transform_plain_to_ntt_device(be.encode_device(S.DeviceBuffer.from_numpy(p), rows * inner), rows * inner, B.parms_id())
    pw = P.to_numpy((rows * inner, K, n))
    plains = [S.Plaintext.from_numpy(side.ctx, pw[o], B.parms_id(), 1.0) for o in range(rows * inner)]

    def decode(ct):
        coeffs, _ = side.dec.decrypt_batch(ct)
        return be.decode_device(coeffs, ct.batch()).to_numpy((ct.batch(), n))

    composed_outs = _composed(ev, side.ctx, plains, _items(B), rows, inner, cols)
    for o, c in enumerate(composed_outs):
        assert np.array_equal(decode(c)[0], want[o]), ("the per-object composition decrypts to the product", o)
    R = ev.matmul_plain_items(P, B, rows, inner, cols)
    assert (R.batch(), R.size()) == (rows * cols, 2)
    got = R.to_numpy()
    for o, c in enumerate(composed_outs):
        assert np.array_equal(got[:, o], c.to_numpy()[:, 0]) and meta(R) == meta(c), ("the composition's words", o)
    assert np.array_equal(decode(R), want), "P X modulo t in every slot"


def case_pipeline_ckks(n, bits, rows=3, inner=2, cols=3, seed=41):
    """CKKS: matmul_plain_items -> rescale_to_next equals, word for word and in its metadata, the per-object composition
    (multiply_plain + add_many per output item) through the same call, in every layout"""
    import encrypt_batch_cases as EB
    side = EB.Side("ckks", n, list(bits))
    ev = side.d.ev
    enc = S.CKKSEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    pid, slots, scale = side.ctx.first_parms_id(), n // 2, 2.0 ** bits[-2]
    p, b = rng.standard_normal((rows * inner, slots)), rng.standard_normal((inner * cols, slots))
    P = enc.encode_device(S.DeviceBuffer.from_array(p), rows * inner, pid, scale)
    B = side.enc.encrypt_symmetric_device(enc.encode_device(S.DeviceBuffer.from_array(b), inner * cols, pid, scale), inner * cols, pid, scale)
    K = B.coeff_modulus_size()
    pw = P.to_numpy((rows * inner, K, n))
    plains = [S.Plaintext.from_numpy(side.ctx, pw[o], pid, scale) for o in range(rows * inner)]
    composed_outs = _composed(ev, side.ctx, plains, _items(B), rows, inner, cols)
    rescaled = [ev.rescale_to_next_inplace(S.Ciphertext.from_numpy(side.ctx, c.to_numpy(), c.parms_id(), True, c.scale(), c.correction_factor()))
                for c in composed_outs]
    Bt = S.Ciphertext.from_numpy(side.ctx, transposed(B.to_numpy(), inner, cols), B.parms_id(), True, B.scale(), B.correction_factor())
    for flags in FLAGS:
        R = ev.matmul_plain_items(P, Bt if flags[0] else B, rows, inner, cols, scale, *flags)
        where = [j * rows + i for i in range(rows) for j in range(cols)] if flags[1] else list(range(rows * cols))
        summed = R.to_numpy()
        for o, c in enumerate(composed_outs):
            assert np.array_equal(summed[:, where[o]], c.to_numpy()[:, 0]) and meta(R) == meta(c), ("matmul_plain_items", flags, o)
        ev.rescale_to_next_inplace(R)
        got = R.to_numpy()
        for o, d in enumerate(rescaled):
            assert np.array_equal(got[:, where[o]], d.to_numpy()[:, 0]) and meta(R) == meta(d) and R.parms_id() == d.parms_id(), ("rescaled", flags, o)
