"""Item maps (ItemMap_Create; Evaluator_SumItemsMapped / DotPlainMapped / DotItemsMapped; shl_reduce_mapped), shared by the CPU
(emulated kernels) and `-m gpu` suites.  Byte equality, per output item, against two yardsticks: the library's unchanged per-object
forms on batches of one holding the named items (multiply_plain_inplace / multiply, then add_many) and, where oracle/_ref is built,
the REAL reference doing the same on its own objects - batch_reduce_cases.expect_group and dot_items_cases.expect_group, fed with
the named items.  The flush-boundary and cut cases compare with Python-integer arithmetic, which depends on neither library.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import batch_reduce_cases as BR
import dot_items_cases as DI
from harness import two_pass_ring
from batch_reduce_cases import meta, forms, _columns, SUM_FLUSH, DOT_FLUSH
from plain_batch_cases import Side, _expect

# the parity map over a source of 7 items: a single, a repeat, a full row, a duplicate-only row
SOURCE = 7
ROWS = [[3], [0, 6, 6], [1, 2, 3, 4, 5, 6, 0], [5, 5]]
SECOND_OF_3 = [[1], [0, 2, 2], [0, 1, 2, 0, 1, 2, 1], [2, 0]]        # an independent second list into a batch of 3
SECOND_OF_7 = [[0], [1, 1, 5], [6, 5, 4, 3, 2, 1, 0], [5, 4]]        # another list into the same batch: not the square
FLUSH_LENGTHS = [1, SUM_FLUSH - 1, SUM_FLUSH, SUM_FLUSH + 1, DOT_FLUSH - 1, DOT_FLUSH, DOT_FLUSH + 1, 2 * DOT_FLUSH + 3]
DOT_ITEMS_LENGTHS = [DI.DOT_ITEMS_FLUSH - 1, DI.DOT_ITEMS_FLUSH, DI.DOT_ITEMS_FLUSH + 1]


def rule_mapped(threads, rows):
    """include/sealhip.h restated: whether and how often to cut follows from the mean row, the slices are sized from the longest"""
    lengths = [len(r) for r in rows]
    s = BR.rule_slices(threads, -(-sum(lengths) // len(lengths)))
    per = -(-max(lengths) // s)
    return -(-max(lengths) // per)


def draw_rows(rng, lengths, batch):
    """rows of the given lengths, in that order, drawn with repeats"""
    return [[int(v) for v in rng.integers(0, batch, n)] for n in lengths]


# ---- the yardsticks, per output row
def check_sum(side, what, got_ct, x, rows, ci, ct_ntt):
    got = got_ct.to_numpy()
    assert got.shape == (x.shape[0], len(rows)) + x.shape[2:], (what, got.shape)
    assert got_ct.batch() == len(rows) and got_ct.size() == x.shape[0] and got_ct.parms_id() == side.ctx.parms_id_at(ci), what
    for o, row in enumerate(rows):
        words, m = BR.expect_group(side, x[:, row], None, ci, ct_ntt)
        assert np.array_equal(got[:, o], words), (what, "output item", o)
        assert meta(got_ct) == m, (what, "metadata")


def check_dot_plain(side, what, got_ct, x, pl, rows, second, ci):
    got = got_ct.to_numpy()
    assert got.shape == (x.shape[0], len(rows)) + x.shape[2:], (what, got.shape)
    assert got_ct.batch() == len(rows) and got_ct.size() == x.shape[0] and got_ct.parms_id() == side.ctx.parms_id_at(ci), what
    for o, (row, sec) in enumerate(zip(rows, second)):
        words, m = BR.expect_group(side, x[:, row], pl[sec], ci, True)
        assert np.array_equal(got[:, o], words), (what, "output item", o)
        assert meta(got_ct) == m, (what, "metadata")


def check_dot_items(side, what, got_ct, x, y, rows, second, ci):
    """y None with second None: the squares"""
    got = got_ct.to_numpy()
    assert got.shape == (3, len(rows)) + x.shape[2:], (what, got.shape)
    assert got_ct.batch() == len(rows) and got_ct.size() == 3 and got_ct.parms_id() == side.ctx.parms_id_at(ci), what
    for o, row in enumerate(rows):
        other = None if y is None and second is None else (x if y is None else y)[:, second[o] if second is not None else row]
        words, m = DI.expect_group(side, x[:, row], other, ci)
        assert np.array_equal(got[:, o], words), (what, "output item", o)
        assert meta(got_ct) == m, (what, "metadata")


# ---- parity
def case_parity(scheme, n, bits, sizes=(2, 3), ci=None, source=SOURCE, rows=ROWS, second=SECOND_OF_3, second_same=SECOND_OF_7, seed=5):
    """the three mapped calls on the parity map: every output item equals the per-object forms on the named items and the reference"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    other = 1 + max(i for r in second for i in r)
    one = S.ItemMap(side.ctx, rows, source)
    two = S.ItemMap(side.ctx, rows, source, second=second, second_batch=other)
    assert one.info() == (len(rows), sum(map(len, rows)), max(map(len, rows)), source, source)
    assert two.info() == (len(rows), sum(map(len, rows)), max(map(len, rows)), source, other)
    for size in sizes:
        for ct_ntt in forms(scheme):
            x = side.rand_ct(rng, ci, source, size)
            c = side.dev_ct(x, ci, ct_ntt)
            out = side.ev.sum_items_mapped(c, one)
            check_sum(side, (scheme, n, "sum", ct_ntt, size), out, x, rows, ci, ct_ntt)
            assert np.array_equal(c.to_numpy(), x), "the operand is only read"
            # only the first list is used: the two-list map over the same first list gives the same words
            assert np.array_equal(side.ev.sum_items_mapped(c, two).to_numpy(), out.to_numpy())
        x = side.rand_ct(rng, ci, source, size)
        pl = side.rand_plain(rng, ci, other, True)
        c, buf = side.dev_ct(x, ci, True), S.DeviceBuffer.from_numpy(pl)
        out = side.ev.dot_plain_mapped(c, buf, other, two, side.scale)
        check_dot_plain(side, (scheme, n, "dot plain", size), out, x, pl, rows, second, ci)
    if scheme == "bfv":
        return
    x, y = side.rand_ct(rng, ci, source, 2), side.rand_ct(rng, ci, other, 2)
    cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
    out = side.ev.dot_items_mapped(cx, cy, two)
    check_dot_items(side, (scheme, n, "dot items, two batches"), out, x, y, rows, second, ci)
    assert np.array_equal(cx.to_numpy(), x) and np.array_equal(cy.to_numpy(), y), "the operands are only read"
    out = side.ev.dot_items_mapped(cx, cx, one)
    check_dot_items(side, (scheme, n, "dot items, square"), out, x, None, rows, None, ci)
    same = S.ItemMap(side.ctx, rows, source, second=second_same, second_batch=source)
    out = side.ev.dot_items_mapped(cx, cx, same)
    check_dot_items(side, (scheme, n, "dot items, one operand and two lists"), out, x, None, rows, second_same, ci)


# ---- gather
def case_gather(scheme, n, bits, source=SOURCE, seed=9):
    """gather_items with a permutation, a repetition and a compaction returns exactly the named items' words, in both forms"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    for ntt in (False, True):
        x = side.rand_ct(rng, ci, source, 2)
        c = side.dev_ct(x, ci, ntt)
        for what, idx in (("permutation", [int(v) for v in rng.permutation(source)]), ("repetition", [2, 2, 6, 2, 0, 0, 6, 6, 6]),
                          ("compaction", [1, 4, 5])):
            out = side.ev.gather_items(c, idx)
            assert out.batch() == len(idx) and out.size() == 2 and out.parms_id() == side.ctx.parms_id_at(ci), what
            assert np.array_equal(out.to_numpy(), x[:, idx]), (what, ntt)
            assert meta(out) == (ntt, side.scale, side.cf), (what, "metadata")
        assert np.array_equal(c.to_numpy(), x)


# ---- agreement with the contiguous forms (a cross-check, not the yardstick)
def case_identity(scheme, n, bits, batch=15, group=5, seed=11):
    """the identity map - rows of `group` consecutive items - gives the words and metadata of sum_items / dot_plain_device / dot_items"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    rows = [list(range(o * group, (o + 1) * group)) for o in range(batch // group)]
    m = S.ItemMap(side.ctx, rows, batch)
    x, y = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)
    pl = side.rand_plain(rng, ci, batch, True)
    cx, cy, buf = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), S.DeviceBuffer.from_numpy(pl)
    pairs = [(side.ev.sum_items_mapped(cx, m), side.ev.sum_items(cx, group)),
             (side.ev.dot_plain_mapped(cx, buf, batch, m, side.scale), side.ev.dot_plain_device(cx, buf, side.scale, group))]
    if scheme != "bfv":
        pairs += [(side.ev.dot_items_mapped(cx, cy, m), side.ev.dot_items(cx, cy, group)),
                  (side.ev.dot_items_mapped(cx, cx, m), side.ev.dot_items(cx, cx, group))]
    for k, (mapped, contiguous) in enumerate(pairs):
        assert np.array_equal(mapped.to_numpy(), contiguous.to_numpy()) and meta(mapped) == meta(contiguous), ("identity map", k)
        assert (mapped.size(), mapped.batch(), mapped.parms_id()) == (contiguous.size(), contiguous.batch(), contiguous.parms_id())


# ---- the raw seam
def raw_mapped(side, ci, kind, a, b, item_map, rows, slices, size=None):
    """shl_reduce_mapped on raw words with a given cut (0: the library's rule) -> (words [size or 3][rows][K][N], slices run);
    b None with kind 2: the same pointer twice (the square kernel when the map has one list)"""
    size = a.shape[0] if size is None else size
    _, a_batch, K, n = a.shape
    da = S.DeviceBuffer.from_numpy(a)
    db = None if kind == 0 else (da if b is None else S.DeviceBuffer.from_numpy(b))
    b_batch = 0 if kind == 0 else (a_batch if b is None else b.shape[-3])
    planes = 3 if kind == 2 else size
    out_words = planes * rows * K * n
    r = S.DeviceBuffer(out_words)
    used = C.c_uint64()
    lib = S._native.lib()

    def call(rp, scratch):
        S._native.check(lib.shl_reduce_mapped(side.ctx._h, C.c_uint64(ci), C.c_int(kind), C.c_void_p(da.ptr), C.c_uint64(a_batch),
                                              C.c_void_p(db.ptr if db else None), C.c_uint64(b_batch), C.c_void_p(rp), C.c_uint64(size),
                                              item_map._h, C.c_uint64(slices), C.c_void_p(scratch), C.byref(used), None))
    call(None, None)   # the slices this will run in
    scratch = S.DeviceBuffer(max(used.value * out_words, 1))
    call(r.ptr, scratch.ptr)
    S.device_synchronize()
    if slices:
        longest = item_map.info()[2]
        per = -(-longest // slices)
        assert used.value == -(-longest // per), ("slices run", used.value, slices)
    return r.to_numpy((planes, rows, K, n)), used.value


def _integers(xo, po, yo, rows, second, q):
    """Python integers over [..][K][2] columns: (sum [size][rows][K][2], dot plain, dot items [3][rows][K][2]); po / yo may be None"""
    size, K = xo.shape[0], len(q)
    want_sum = np.zeros((size, len(rows), K, 2), dtype=np.uint64)
    want_dot = np.zeros((size, len(rows), K, 2), dtype=np.uint64)
    want_items = np.zeros((3, len(rows), K, 2), dtype=np.uint64)
    for o, row in enumerate(rows):
        sec = second[o] if second is not None else row
        for k in range(K):
            want_sum[:, o, k] = (xo[:, row, k].sum(axis=1) % q[k]).astype(np.uint64)
            if po is not None:
                want_dot[:, o, k] = ((xo[:, row, k] * po[None, sec, k]).sum(axis=1) % q[k]).astype(np.uint64)
            if yo is not None:
                x0, x1, y0, y1 = xo[0, row, k], xo[1, row, k], yo[0, sec, k], yo[1, sec, k]
                want_items[0, o, k] = ((x0 * y0).sum(axis=0) % q[k]).astype(np.uint64)
                want_items[1, o, k] = ((x0 * y1 + x1 * y0).sum(axis=0) % q[k]).astype(np.uint64)
                want_items[2, o, k] = ((x1 * y1).sum(axis=0) % q[k]).astype(np.uint64)
    return want_sum, want_dot, want_items


# ---- ragged flush boundaries: Python-integer arithmetic
def case_flush(n, bits, patterns=("max", "alternating", "half", "random"), source=SOURCE, seed=61):
    """one map whose rows have 1, 15, 16, 17, 255, 256, 257 and 515 terms, in this order (on a ring of 8 the lanes of one wave sit
    in all of them and flush at different trips), drawn with repeats from 7 items whose words are all q - 1 (and the structured
    cases alternating / q / 2, and random ones): every word of the sum and of the plaintext dot product equals the sum formed with
    Python integers, for the evaluator's own schedule and for the one-launch form whose threads walk whole rows.  The ciphertext
    dot product has its interval at 128 items: the same with rows of 127, 128 and 129 terms added"""
    assert BR.library_flush_intervals() == (SUM_FLUSH, DOT_FLUSH) and DI.library_flush_interval() == DI.DOT_ITEMS_FLUSH == 128
    assert FLUSH_LENGTHS == [1, 15, 16, 17, 255, 256, 257, 515] and DOT_ITEMS_LENGTHS == [127, 128, 129]
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    rows = draw_rows(rng, FLUSH_LENGTHS, source)
    second = draw_rows(rng, FLUSH_LENGTHS, source)
    rows_items = rows + draw_rows(rng, DOT_ITEMS_LENGTHS, source)
    second_items = second + draw_rows(rng, DOT_ITEMS_LENGTHS, source)
    m = S.ItemMap(side.ctx, rows, source, second=second)
    m_items = S.ItemMap(side.ctx, rows_items, source, second=second_items)
    m_square = S.ItemMap(side.ctx, rows_items, source)
    for pattern in patterns:
        xc = _columns(side, ci, pattern, rng, (2, source))    # [2][source][K][2]
        yc = _columns(side, ci, pattern if pattern != "alternating" else "max", rng, (2, source))
        pc = yc[0]
        x, y = np.ascontiguousarray(np.tile(xc, n // 2)), np.ascontiguousarray(np.tile(yc, n // 2))
        pl = np.ascontiguousarray(y[0])
        assert np.array_equal(x[..., -2:], xc) and x.shape == (2, source, len(q), n)
        xo, yo, po = xc.astype(object), yc.astype(object), pc.astype(object)
        want_sum, want_dot, _ = _integers(xo, po, None, rows, second, q)
        _, _, want_items = _integers(xo, None, yo, rows_items, second_items, q)
        _, _, want_square = _integers(xo, None, xo, rows_items, None, q)
        want_sum, want_dot, want_items, want_square = (np.tile(w, n // 2) for w in (want_sum, want_dot, want_items, want_square))
        cx, cy, buf = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), S.DeviceBuffer.from_numpy(pl)
        assert np.array_equal(side.ev.sum_items_mapped(cx, m).to_numpy(), want_sum), ("sum", pattern, "evaluator")
        assert np.array_equal(side.ev.dot_plain_mapped(cx, buf, source, m, side.scale).to_numpy(), want_dot), ("dot plain", pattern, "evaluator")
        assert np.array_equal(side.ev.dot_items_mapped(cx, cy, m_items).to_numpy(), want_items), ("dot items", pattern, "evaluator")
        assert np.array_equal(side.ev.dot_items_mapped(cx, cx, m_square).to_numpy(), want_square), ("dot items, square", pattern, "evaluator")
        assert np.array_equal(raw_mapped(side, ci, 0, x, None, m, len(rows), 1)[0], want_sum), ("sum", pattern, "one launch")
        assert np.array_equal(raw_mapped(side, ci, 1, x, pl[None], m, len(rows), 1)[0], want_dot), ("dot plain", pattern, "one launch")
        assert np.array_equal(raw_mapped(side, ci, 2, x, y, m_items, len(rows_items), 1)[0], want_items), ("dot items", pattern, "one launch")
        assert np.array_equal(raw_mapped(side, ci, 2, x, None, m_square, len(rows_items), 1)[0], want_square), ("square", pattern, "one launch")


# ---- ragged cuts
CUT_LENGTHS = [1, 4, 23, 9]


def case_cuts(n, bits, slice_counts=(1, 2, 3, 5, 23), sizes=(1, 4, 5), patterns=("max", "random"), source=SOURCE, seed=67):
    """rows of 1, 4, 23 and 9 terms in 1, 2, 3, 5 and 23 slices through shl_reduce_mapped: most slices of the short rows are empty
    and must store zeros.  Planes 1, 4 and 5 (the product takes its planes three at a time, the sum has them in its grid), the
    ciphertext dot product and its square.  Every word equals the sum formed with Python integers, whatever the cut"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    q = [int(v) for v in side.q(ci)]
    rows, second = draw_rows(rng, CUT_LENGTHS, source), draw_rows(rng, CUT_LENGTHS, 3)
    m = S.ItemMap(side.ctx, rows, source, second=second, second_batch=3)
    m_one = S.ItemMap(side.ctx, rows, source)
    for pattern in patterns:
        for size in sizes:
            xc = _columns(side, ci, pattern, rng, (size, source))
            pc = _columns(side, ci, pattern, rng, (3,))
            x, pl = np.ascontiguousarray(np.tile(xc, n // 2)), np.ascontiguousarray(np.tile(pc, n // 2))
            want_sum, want_dot, _ = _integers(xc.astype(object), pc.astype(object), None, rows, second, q)
            for s in slice_counts:
                assert np.array_equal(raw_mapped(side, ci, 0, x, None, m, len(rows), s)[0], np.tile(want_sum, n // 2)), ("sum", size, pattern, s)
                assert np.array_equal(raw_mapped(side, ci, 1, x, pl[None], m, len(rows), s)[0], np.tile(want_dot, n // 2)), ("dot", size, pattern, s)
        xc, yc = _columns(side, ci, pattern, rng, (2, source)), _columns(side, ci, pattern, rng, (2, 3))
        x, y = np.ascontiguousarray(np.tile(xc, n // 2)), np.ascontiguousarray(np.tile(yc, n // 2))
        _, _, want = _integers(xc.astype(object), None, yc.astype(object), rows, second, q)
        _, _, want_sq = _integers(xc.astype(object), None, xc.astype(object), rows, None, q)
        for s in slice_counts:
            assert np.array_equal(raw_mapped(side, ci, 2, x, y, m, len(rows), s)[0], np.tile(want, n // 2)), ("dot items", pattern, s)
            assert np.array_equal(raw_mapped(side, ci, 2, x, None, m_one, len(rows), s)[0], np.tile(want_sq, n // 2)), ("square", pattern, s)


def case_natural_slices(n, bits, source=SOURCE, seed=71):
    """no forcing: by the documented rule the map of rows 1, 4, 23, 9 (mean 10) is cut - into slices sized from the longest row -
    and a map of the same number of short rows (mean below 8) is not; both slices_used values are asserted from the rule, and the
    words of the cut run are those of the one-launch form and of the per-object forms"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    long_rows, short_rows = draw_rows(rng, CUT_LENGTHS, source), draw_rows(rng, [1, 4, 9, 5], source)
    threads = len(long_rows) * K * n // 2   # one plane: the products
    assert rule_mapped(threads, long_rows) == 2 and -(-23 // 2) == 12, "mean 10 in two slices, of ceil(23 / 2) = 12 terms at most"
    assert rule_mapped(threads, short_rows) == 1 and rule_mapped(2 * threads, short_rows) == 1
    x = side.rand_ct(rng, ci, source, 2)
    pl = side.rand_plain(rng, ci, source, True)
    for rows in (long_rows, short_rows):
        m = S.ItemMap(side.ctx, rows, source)
        for kind, planes in ((0, 2), (1, 1), (2, 1)):
            got, used = raw_mapped(side, ci, kind, x, pl[None] if kind == 1 else None, m, len(rows), 0)
            assert used == rule_mapped(planes * threads, rows), ("the library's rule is the documented one", kind, used)
            assert np.array_equal(got, raw_mapped(side, ci, kind, x, pl[None] if kind == 1 else None, m, len(rows), 1)[0]), ("rule and one launch", kind)
        cx = side.dev_ct(x, ci, True)
        check_sum(side, "natural slices", side.ev.sum_items_mapped(cx, m), x, rows, ci, True)
        check_dot_plain(side, "natural slices", side.ev.dot_plain_mapped(cx, S.DeviceBuffer.from_numpy(pl), source, m, side.scale), x, pl, rows, rows, ci)
        check_dot_items(side, "natural slices", side.ev.dot_items_mapped(cx, cx, m), x, None, rows, None, ci)


# ---- life cycle
def case_out_of_place(scheme, n, bits, seed=17):
    """the operands are unchanged; a destination of another level, size, form or context's worth of words is reshaped"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, out = side.first, len(ROWS)
    x = side.rand_ct(rng, ci, SOURCE, 2)
    pl = side.rand_plain(rng, ci, 3, True)
    buf = S.DeviceBuffer.from_numpy(pl)
    m = S.ItemMap(side.ctx, ROWS, SOURCE, second=SECOND_OF_3, second_batch=3)
    m7 = S.ItemMap(side.ctx, ROWS, SOURCE, second=SECOND_OF_7)
    foreign = Side(scheme, n, bits)
    for op in ("sum", "dot plain") + (("dot items",) if scheme != "bfv" else ()):
        want = None
        for dest in (S.Ciphertext(side.ctx, batch=out), side.dev_ct(side.rand_ct(rng, 0, out, 2), 0, True),
                     side.dev_ct(side.rand_ct(rng, ci, out, 4), ci, False), foreign.dev_ct(x[:, :out], ci, True)):
            src = side.dev_ct(x, ci, True)
            got = (side.ev.sum_items_mapped(src, m, dest) if op == "sum" else
                   side.ev.dot_plain_mapped(src, buf, 3, m, side.scale, dest) if op == "dot plain" else side.ev.dot_items_mapped(src, src, m7, dest))
            assert got is dest and np.array_equal(src.to_numpy(), x) and meta(src) == (True, side.scale, side.cf), ("encrypted changed", op)
            assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), 3 if op == "dot items" else 2, out)
            if want is None:
                if op == "sum":
                    check_sum(side, (scheme, op), dest, x, ROWS, ci, True)
                elif op == "dot plain":
                    check_dot_plain(side, (scheme, op), dest, x, pl, ROWS, SECOND_OF_3, ci)
                else:
                    check_dot_items(side, (scheme, op), dest, x, None, ROWS, SECOND_OF_7, ci)
                want = dest.to_numpy(), meta(dest)
            assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], ("reshaped destination", op)


def case_transparent_check(scheme, n, bits):
    """an all-zero result is refused when the check is on (and computed when it is off); a proper one passes"""
    side = Side(scheme, n, bits)
    ci = side.first
    x = side.rand_ct(np.random.default_rng(3), ci, SOURCE, 2)
    x0 = x.copy()
    x0[1] = 0
    pl = side.rand_plain(np.random.default_rng(4), ci, SOURCE, True)
    buf = S.DeviceBuffer.from_numpy(pl)
    m = S.ItemMap(side.ctx, ROWS, SOURCE)
    assert not np.any(side.ev.sum_items_mapped(side.dev_ct(x0, ci, True), m).to_numpy()[1])
    side.ev.set_transparent_check(True)
    try:
        _expect(S.LogicError, lambda: side.ev.sum_items_mapped(side.dev_ct(x0, ci, True), m), "transparent sum")
        _expect(S.LogicError, lambda: side.ev.dot_plain_mapped(side.dev_ct(x0, ci, True), buf, SOURCE, m, side.scale), "transparent dot product")
        if scheme != "bfv":
            c0 = side.dev_ct(x0, ci, True)
            _expect(S.LogicError, lambda: side.ev.dot_items_mapped(c0, c0, m), "transparent ciphertext dot product")
        out = side.ev.sum_items_mapped(side.dev_ct(x, ci, True), m)
    finally:
        side.ev.set_transparent_check(False)
    check_sum(side, (scheme, "transparent check on"), out, x, ROWS, ci, True)


def case_pending(n, bits, seed=73):
    """operands with a pending tensor product and with a deferred key-switch tail are settled before the mapped calls read them, and
    a destination's own pending product is discarded: the words of the eager sequence (SEALHIP_LAZY_PRODUCT=0
    SEALHIP_KS_EAGER_TAIL=1), which are the sums of the named items of the settled operands"""
    from parity_cases import _Env
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, batch = side.first, 3
    rows, second = [[2], [0, 1, 1]], [[0], [2, 2, 1]]
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    x, y = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)
    m = S.ItemMap(side.ctx, rows, batch, second=second)

    def run():
        a, b = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
        prod = side.ev.multiply(a, b, S.Ciphertext(side.ctx, batch=batch))
        of_product = side.ev.sum_items_mapped(prod, m)            # a pending product is formed first
        relin = side.ev.relinearize_inplace(side.ev.multiply(a, b, S.Ciphertext(side.ctx, batch=batch)), rlk)
        of_tail = side.ev.sum_items_mapped(relin, m)              # a deferred tail is completed first
        relin2 = side.ev.relinearize_inplace(side.ev.multiply(a, b, S.Ciphertext(side.ctx, batch=batch)), rlk)
        dotted = side.ev.dot_items_mapped(relin2, b, m)           # the same for the first operand of the ciphertext dot product
        a1, b1 = side.dev_ct(x[:, :2], ci, True), side.dev_ct(y[:, :2], ci, True)   # (alive: a product is formed when an operand goes away)
        dest = side.ev.multiply(a1, b1, S.Ciphertext(side.ctx, batch=2))
        side.ev.sum_items_mapped(relin, m, dest)                  # pending state of the destination is discarded
        return [c.to_numpy() for c in (of_product, of_tail, dotted, dest, prod, relin)]

    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT_MIN_WGS=0, SEALHIP_LAZY_PRODUCT=None, SEALHIP_KS_EAGER_TAIL=None):
        tails0, products0 = S.tail_stats(), S.product_stats()
        lazy = run()
        tails1, products1 = S.tail_stats(), S.product_stats()
    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT=0, SEALHIP_KS_EAGER_TAIL=1):
        eager = run()
    if two_pass_ring(n):   # the sizes at which the library defers
        assert tails1[1] - tails0[1] >= 2, "the mapped calls completed deferred tails"
        assert products1[1] - products0[1] >= 1, "sum_items_mapped formed a pending product"
        assert products1[2] - products0[2] >= 1, "the destination's pending product was discarded"
    for got, want, what in zip(lazy, eager, ("sum of a product", "sum after relinearize", "dot after relinearize", "into a pending destination",
                                             "product", "relinearized")):
        assert np.array_equal(got, want), what
    assert np.array_equal(lazy[1], lazy[3])
    q = side.q(ci)[None, :, None]
    for src, got in ((lazy[4], lazy[0]), (lazy[5], lazy[1])):
        for o, row in enumerate(rows):
            acc = np.zeros_like(src[:, 0])
            for b in row:
                acc = (acc + src[:, b]) % q
            assert np.array_equal(got[:, o], acc), ("the sums are sums of the named items", o)
    # the ciphertext dot product on the settled words, through the per-object forms
    side.scale, saved = side.scale ** 2, side.scale   # relin carries the product's scale
    try:
        settled = side.dev_ct(lazy[5], ci, True)
    finally:
        side.scale = saved
    prods = side.ev.multiply(side.ev.gather_items(settled, [i for r in rows for i in r]),
                             side.ev.gather_items(side.dev_ct(y, ci, True), [i for r in second for i in r]), S.Ciphertext(side.ctx, batch=4))
    want = side.ev.sum_items_mapped(prods, S.ItemMap(side.ctx, [[0], [1, 2, 3]], 4))
    assert np.array_equal(lazy[2], want.to_numpy()), "multiply + sum on the settled operands"


def case_capture(n, bits, lengths=(16, 12), source=SOURCE, seed=47):
    """CKKS: dot_plain_mapped + sum_items_mapped + dot_items_mapped recorded in a graph, with a map whose result the documented rule
    cuts (pool scratch inside the recording).  Ciphertext and plaintext words are refreshed in place before each replay; the replay
    equals the eager result and the per-object forms"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    rows, second = draw_rows(rng, lengths, source), draw_rows(rng, lengths, 3)
    assert rule_mapped(len(rows) * K * n // 2, rows) > 1, "the recorded products are cut"
    m = S.ItemMap(side.ctx, rows, source, second=second, second_batch=3)
    gather = S.ItemMap(side.ctx, [[1], [0]], len(rows))
    cx = side.dev_ct(side.rand_ct(rng, ci, source, 2), ci, True)
    cy = side.dev_ct(side.rand_ct(rng, ci, 3, 2), ci, True)
    buf = S.DeviceBuffer(3 * K * n)
    outs = [[S.Ciphertext(side.ctx, batch=len(rows)) for _ in range(3)] for _ in range(2)]
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        pl = np.ascontiguousarray(side.rand_plain(rng, ci, 3, True))
        S._native.check(h2d(C.c_void_p(buf.ptr), pl.ctypes.data_as(C.c_void_p), C.c_uint64(pl.nbytes)))
        state["pl"] = pl
        for name, c, b in (("x", cx, source), ("y", cy, 3)):
            w = np.ascontiguousarray(side.rand_ct(rng, ci, b, 2))
            S._native.check(h2d(C.c_void_p(c.device_ptr()[0]), w.ctypes.data_as(C.c_void_p), C.c_uint64(w.nbytes)))
            state[name] = w

    def step(o=outs[0]):
        side.ev.dot_plain_mapped(cx, buf, 3, m, side.scale, o[0])
        side.ev.sum_items_mapped(o[0], gather, o[1])
        side.ev.dot_items_mapped(cx, cy, m, o[2])

    refresh()
    step()   # eager once
    graph = side.ev.capture(step)
    for trial in range(2):
        refresh()
        graph.launch()
        replay = [c.to_numpy() for c in outs[0]]
        step(outs[1])
        for k in range(3):
            assert np.array_equal(replay[k], outs[1][k].to_numpy()) and meta(outs[0][k]) == meta(outs[1][k]), ("graph replay", trial, k)
        assert np.array_equal(cx.to_numpy(), state["x"]) and np.array_equal(cy.to_numpy(), state["y"]), "the operands are only read"
    check_dot_plain(side, "replayed dot product", outs[0][0], state["x"], state["pl"], rows, second, ci)
    assert np.array_equal(outs[0][1].to_numpy(), outs[0][0].to_numpy()[:, [1, 0]]), "replayed gather"
    check_dot_items(side, "replayed ciphertext dot product", outs[0][2], state["x"], state["y"], rows, second, ci)


def case_destroy_after_call(scheme, n, bits, seed=53):
    """a map destroyed right after the call that used it, its block taken again at once: the queued call still reads its lists"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    x = side.rand_ct(rng, ci, SOURCE, 2)
    c = side.dev_ct(x, ci, True)
    outs = []
    for trial in range(3):
        m = S.ItemMap(side.ctx, ROWS if trial != 1 else ROWS[::-1], SOURCE)
        outs.append(side.ev.sum_items_mapped(c, m))
        m.destroy()
        assert m._h is None
    check_sum(side, "destroyed map", outs[0], x, ROWS, ci, True)
    check_sum(side, "destroyed map", outs[1], x, ROWS[::-1], ci, True)
    assert np.array_equal(outs[2].to_numpy(), outs[0].to_numpy())


# ---- errors
def case_create_errors(scheme, n, bits):
    """everything ItemMap_Create validates, and its NULL pointers"""
    side = Side(scheme, n, bits)
    lib = S._native.lib()
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER

    def create(rows, offsets, first, second, b1, b2, ctx=side.ctx._h, out=True):
        h = C.c_void_p()
        arr = lambda v: None if v is None else (C.c_uint64 * max(len(v), 1))(*v)
        hr = lib.ItemMap_Create(ctx, C.c_uint64(rows), arr(offsets), arr(first), arr(second), C.c_uint64(b1), C.c_uint64(b2),
                                C.byref(h) if out else None) & 0xFFFFFFFF
        if hr == 0:
            assert lib.ItemMap_Destroy(h) == 0
        return hr

    assert create(2, [0, 1, 3], [0, 1, 2], None, 3, 3) == 0 and create(2, [0, 1, 3], [0, 1, 2], [4, 4, 0], 3, 5) == 0, "valid maps"
    assert create(2, [0, 1, 1], [0, 1, 2], None, 3, 3) == INVALID, "an empty row"
    assert create(2, [0, 2, 1], [0, 1, 2], None, 3, 3) == INVALID, "decreasing offsets"
    assert create(2, [1, 2, 3], [0, 1, 2], None, 3, 3) == INVALID, "offsets[0] != 0"
    assert create(2, [0, 1, 3], [0, 3, 2], None, 3, 3) == INVALID, "index == batch"
    assert create(2, [0, 1, 3], [0, 1, 2], [0, 5, 0], 3, 5) == INVALID, "second index == second batch"
    assert create(0, [0], [0], None, 3, 3) == INVALID, "rows == 0"
    assert create(1 << 32, [0], [0], None, 3, 3) == INVALID, "rows == 2^32 (refused before the arrays are read)"
    assert create(2, [0, 1, 3], [0, 1, 2], None, 3, 4) == INVALID, "second_items == NULL with unequal batches"
    assert create(2, None, [0, 1, 2], None, 3, 3) == INVALID and create(2, [0, 1, 3], None, None, 3, 3) == INVALID, "NULL arrays"
    assert create(2, [0, 1, 3], [0, 1, 2], None, 3, 3, ctx=None) == POINTER and create(2, [0, 1, 3], [0, 1, 2], None, 3, 3, out=False) == POINTER
    assert lib.ItemMap_Destroy(None) & 0xFFFFFFFF == POINTER and lib.ItemMap_Info(None, None, None, None, None, None) & 0xFFFFFFFF == POINTER
    for bad in ([[0], []], [[3]], []):
        _expect(S.InvalidArgument, lambda: S.ItemMap(side.ctx, bad, 3), "the Python constructor passes the library's refusal on")
    _expect(ValueError, lambda: S.ItemMap(side.ctx, [[0, 1]], 3, second=[[0]]), "lists of different shapes")


def case_errors(scheme, n, bits):
    """every check of the three calls returns its HRESULT and leaves the destination untouched; valid calls afterwards work"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, lib, ev = side.first, S._native.lib(), side.ev._h
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    out = len(ROWS)
    x, y = side.rand_ct(rng, ci, SOURCE, 2), side.rand_ct(rng, ci, 3, 2)
    pl = side.rand_plain(rng, ci, 3, True)
    buf = S.DeviceBuffer.from_numpy(pl)
    cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
    m = S.ItemMap(side.ctx, ROWS, SOURCE, second=SECOND_OF_3, second_batch=3)
    one = S.ItemMap(side.ctx, ROWS, SOURCE)
    dest = side.dev_ct(side.rand_ct(rng, ci, out, 3), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)
    wrong_batch = S.Ciphertext(side.ctx, batch=out + 1)
    other_side = Side(scheme, n, bits)
    foreign = other_side.dev_ct(x, ci, True)
    foreign_map = S.ItemMap(other_side.ctx, ROWS, SOURCE, second=SECOND_OF_3, second_batch=3)
    invalid = side.dev_ct(x, ci, True)
    invalid.set_scale(0.0 if scheme == "ckks" else 2.0)   # is_metadata_valid_for fails
    fewer = side.dev_ct(x[:, :SOURCE - 1], ci, True)

    def rsum(ev_h, ct_h, m_h, dest_h):
        return lib.Evaluator_SumItemsMapped(ev_h, ct_h, m_h, dest_h) & 0xFFFFFFFF

    def rdot(ev_h, ct_h, ptr, count, m_h, scale, dest_h):
        return lib.Evaluator_DotPlainMapped(ev_h, ct_h, C.c_void_p(ptr), C.c_uint64(count), m_h, C.c_double(scale), dest_h) & 0xFFFFFFFF

    def ritems(ev_h, x_h, y_h, m_h, dest_h):
        return lib.Evaluator_DotItemsMapped(ev_h, x_h, y_h, m_h, dest_h) & 0xFFFFFFFF

    good = (ev, cx._h, buf.ptr, 3, m._h, side.scale, dest._h)
    for k in (0, 1, 2, 3):
        args = [ev, cx._h, m._h, dest._h]
        args[k] = None
        assert rsum(*args) == POINTER, ("NULL handle", k)
    for k in (0, 1, 4, 6):
        args = list(good)
        args[k] = None
        assert rdot(*args) == POINTER, ("NULL handle", k)
    assert rsum(ev, invalid._h, m._h, dest._h) == INVALID and rdot(ev, invalid._h, *good[2:]) == INVALID, "an invalid ciphertext"
    assert rsum(ev, foreign._h, m._h, dest._h) == INVALID and rdot(ev, foreign._h, *good[2:]) == INVALID, "a ciphertext of another context"
    assert rsum(ev, cx._h, foreign_map._h, dest._h) == INVALID and rdot(*good[:4], foreign_map._h, *good[5:]) == INVALID, "a map of another context"
    assert rsum(ev, fewer._h, m._h, dest._h) == INVALID and rdot(ev, fewer._h, *good[2:]) == INVALID, "the operand's batch != the map's"
    assert rsum(ev, cx._h, m._h, wrong_batch._h) == INVALID and rdot(*good[:6], wrong_batch._h) == INVALID, "destination's batch != rows"
    gather7 = S.ItemMap(side.ctx, [[i] for i in range(SOURCE)], SOURCE)
    assert rsum(ev, cx._h, gather7._h, cx._h) == INVALID and rdot(ev, cx._h, buf.ptr, SOURCE, gather7._h, side.scale, cx._h) == INVALID, "destination == encrypted"
    assert rdot(*good[:3], 4, *good[4:]) == INVALID and rdot(*good[:3], 0, *good[4:]) == INVALID, "plain_count != second_batch"
    assert rdot(ev, cx._h, None, *good[3:]) == INVALID, "NULL device_plain"
    assert rdot(ev, cx._h, buf.ptr + 8, *good[3:]) == INVALID, "misaligned device_plain"
    ptr, _ = cx.device_ptr()
    assert rdot(ev, cx._h, ptr + 16, *good[3:]) == INVALID, "device_plain inside encrypted"
    ptr, _ = dest.device_ptr()
    assert rdot(ev, cx._h, ptr + 16, *good[3:]) == INVALID, "device_plain inside destination"
    assert rdot(ev, side.dev_ct(x, ci, False)._h, *good[2:]) == INVALID, "a coefficient-form ciphertext"
    if scheme == "ckks":
        assert rdot(*good[:5], 0.0, dest._h) == INVALID, "CKKS plaintext scale"
        assert rdot(*good[:5], 2.0 ** 400, dest._h) == INVALID, "scale out of bounds"
    _expect(ValueError, lambda: side.ev.dot_plain_mapped(cx, S.DeviceBuffer(max(pl.size - n, 1)), 3, m, side.scale, dest), "too few plaintext words")
    if scheme == "bfv":
        assert ritems(ev, cx._h, cx._h, one._h, dest._h) == INVALID, "BFV is refused"
    else:
        for k in range(5):
            args = [ev, cx._h, cy._h, m._h, dest._h]
            args[k] = None
            assert ritems(*args) == POINTER, ("NULL handle", k)
        lower = side.dev_ct(side.rand_ct(rng, ci - 1, 3, 2), ci - 1, True)
        three = side.dev_ct(side.rand_ct(rng, ci, 3, 3), ci, True)
        for bad, what in ((invalid, "an invalid ciphertext"), (foreign, "a ciphertext of another context"), (fewer, "x's batch != first_batch")):
            assert ritems(ev, bad._h, cy._h, m._h, dest._h) == INVALID, what
        for bad, what in ((lower, "mismatched levels"), (side.dev_ct(y, ci, False), "coefficient form"), (three, "a size other than 2"),
                          (cx, "y's batch != second_batch")):
            assert ritems(ev, cx._h, bad._h, m._h, dest._h) == INVALID, what
        assert ritems(ev, cx._h, cy._h, foreign_map._h, dest._h) == INVALID, "a map of another context"
        assert ritems(ev, cx._h, cy._h, m._h, wrong_batch._h) == INVALID, "destination's batch != rows"
        three_rows = S.ItemMap(side.ctx, [[0], [1], [2]], SOURCE, second=[[0], [1], [2]], second_batch=3)
        assert ritems(ev, cx._h, cy._h, three_rows._h, cy._h) == INVALID and ritems(ev, cx._h, cx._h, gather7._h, cx._h) == INVALID, "destination == an operand"
        if scheme == "ckks":
            big = side.dev_ct(x, ci, True)
            big.set_scale(2.0 ** 100)   # valid by itself; the product's 2^200 is beyond the level's modulus
            assert ritems(ev, big._h, big._h, one._h, dest._h) == INVALID, "scale out of bounds"
    assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
    assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
    assert np.array_equal(cx.to_numpy(), x) and np.array_equal(cy.to_numpy(), y)
    # valid calls afterwards
    side.ev.dot_plain_mapped(cx, buf, 3, m, side.scale, dest)
    check_dot_plain(side, "after the failures", dest, x, pl, ROWS, SECOND_OF_3, ci)
    side.ev.sum_items_mapped(cx, m, dest)
    check_sum(side, "after the failures", dest, x, ROWS, ci, True)
    if scheme != "bfv":
        side.ev.dot_items_mapped(cx, cy, m, dest)
        check_dot_items(side, "after the failures", dest, x, y, ROWS, SECOND_OF_3, ci)


# ---- pipelines (the reference's keys and objects)
def case_pipeline_sparse_matrix(n, bits, seed=41):
    """a 4 x 6 sparse plaintext matrix with 9 non-zeros times 6 encrypted columns: encode_device -> encrypt_symmetric_device ->
    dot_plain_mapped (one plaintext per non-zero) -> rescale_to_next -> decrypt_batch -> decode_device.  The ciphertext words after
    both evaluator stages equal the reference doing multiply_plain + add_many row by row on the same fresh ciphertexts"""
    from plain_batch_cases import _client
    side = _client("ckks", n, bits)
    ref, ev = side.ref, side.d.ev
    enc = S.CKKSEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    pid, ci, slots = side.ctx.first_parms_id(), side.first, n // 2
    scale = 2.0 ** (bits[-2] if len(bits) > 2 else 12)
    columns = [[0, 3], [1], [2, 4, 5, 0], [5, 3]]    # row o of the matrix: the columns of its non-zeros - 9 in all
    nonzeros = sum(map(len, columns))
    assert (len(columns), nonzeros) == (4, 9)
    weight_of, k = [], 0
    for r in columns:
        weight_of.append(list(range(k, k + len(r))))
        k += len(r)
    v, w = rng.standard_normal((6, slots)), rng.standard_normal((nonzeros, slots))
    wv = enc.encode_device(S.DeviceBuffer.from_array(v), 6, pid, scale)
    ww = enc.encode_device(S.DeviceBuffer.from_array(w), nonzeros, pid, scale)
    ww_host = ww.to_numpy((nonzeros, side.K(ci), n))
    side.enc.set_seed(None)
    V = side.enc.encrypt_symmetric_device(wv, 6, pid, scale)
    fresh = [V.save_bytes(item=b) for b in range(6)]
    m = S.ItemMap(side.ctx, columns, 6, second=weight_of, second_batch=nonzeros)
    R = ev.dot_plain_mapped(V, ww, nonzeros, m, scale)
    assert (R.batch(), R.size(), R.scale()) == (4, 2, scale * scale)
    product = R.to_numpy()
    ev.rescale_to_next_inplace(R)
    rescaled = R.to_numpy()
    coeffs, _ = side.dec.decrypt_batch(R)
    got = enc.decode_device(coeffs, 4, R.parms_id(), R.scale()).to_array((4, slots))
    for o, (cols, ws) in enumerate(zip(columns, weight_of)):
        rs = []
        for c, k in zip(cols, ws):
            r, _ = ref.ct_load(fresh[c])
            rs.append(ref.multiply_plain_inplace(r, ref.pt(ww_host[k], ci, scale)))
        r = ref.add_many(rs)
        assert np.array_equal(product[:, o], r.data()) and scale * scale == r.info()["scale"], ("dot_plain_mapped", o)
        ref.rescale_to_next_inplace(r)
        assert np.array_equal(rescaled[:, o], r.data()) and R.scale() == r.info()["scale"], ("rescale", o)
        want = ref.ckks_decode(ref.decrypt(r), False)
        assert got[o].tobytes() == want.tobytes(), ("decode", o)
        assert np.max(np.abs(got[o] - sum(v[c] * w[k] for c, k in zip(cols, ws)))) < 1e-2 * len(cols), ("row of the product", o)


def case_pipeline_pairs(n, bits, seed=43):
    """sum of x_i (x) y_j over 5 pairs in two rows: encode_device -> encrypt_symmetric_device (two batches of different length) ->
    dot_items_mapped -> relinearize -> rescale_to_next; after every stage the words of output item o equal the reference's
    per-pair multiply -> add_many -> relinearize -> rescale on the same fresh ciphertexts"""
    import encrypt_batch_cases as EB
    side = EB.Side("ckks", n, bits, ref_seed=0x5EA1)
    ref, ev = side.ref, side.d.ev
    enc = S.CKKSEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    ref.keygen_relin()
    rlk = S.RelinKeys(side.ctx)
    rlk.load_bytes(ref.keys_save("relin", True))
    pid, slots = side.ctx.first_parms_id(), n // 2
    scale = 2.0 ** bits[-2]
    pairs = [[(0, 1), (2, 0)], [(1, 1), (3, 2), (0, 0)]]
    a, b = rng.standard_normal((4, slots)), rng.standard_normal((3, slots))
    wa = enc.encode_device(S.DeviceBuffer.from_array(a), 4, pid, scale)
    wb = enc.encode_device(S.DeviceBuffer.from_array(b), 3, pid, scale)
    side.enc.set_seed(None)
    A = side.enc.encrypt_symmetric_device(wa, 4, pid, scale)
    B = side.enc.encrypt_symmetric_device(wb, 3, pid, scale)
    fa, fb = [A.save_bytes(item=k) for k in range(4)], [B.save_bytes(item=k) for k in range(3)]
    R = ev.dot_items_mapped(A, B, S.ItemMap(side.ctx, pairs, 4, second_batch=3))
    assert (R.batch(), R.size(), R.scale()) == (2, 3, scale * scale)
    summed = R.to_numpy()
    ev.relinearize_inplace(R, rlk)
    relinearized = R.to_numpy()
    ev.rescale_to_next_inplace(R)
    rescaled = R.to_numpy()
    for o, row in enumerate(pairs):
        rs = []
        for i, j in row:
            rs.append(ref.multiply_inplace(ref.ct_load(fa[i])[0], ref.ct_load(fb[j])[0]))
        r = ref.add_many(rs)
        assert np.array_equal(summed[:, o], r.data()), ("dot_items_mapped", o)
        ref.relinearize_inplace(r)
        assert np.array_equal(relinearized[:, o], r.data()), ("relinearize", o)
        ref.rescale_to_next_inplace(r)
        assert np.array_equal(rescaled[:, o], r.data()) and R.scale() == r.info()["scale"], ("rescale", o)
