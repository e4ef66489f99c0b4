"""The ciphertext x ciphertext reduction over the items of two device-resident batches (Evaluator_DotItems), shared by the CPU
(emulated kernels) and `-m gpu` suites.  Byte equality, per output item, against: the library's own multiply on batches of one and
add_many over the products; the REAL reference (oracle/_ref) doing the same on its own objects, where it is built; and, around the
flush interval of the lazy accumulators, Python-integer arithmetic, which depends on neither library.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
from harness import two_pass_ring
from batch_reduce_cases import meta, rule_slices, SLICE_BELOW
from plain_batch_cases import Side, _expect

# batch_reduce_kernels.hip: 2^(128 - 2 * 60) products of words below 2^60 fit 128 bits, and the middle polynomial adds two per item
DOT_ITEMS_FLUSH = (1 << (128 - 2 * 60)) // 2


def library_flush_interval():
    v = C.c_uint64()
    S._native.check(S._native.lib().shl_dot_items_flush_interval(C.byref(v)))
    return v.value


def expect_group(side, x, y, ci):
    """x, y [2][g][K][N] (y None: the squares) through multiply on batches of one and add_many -> (words [3][K][N], metadata); the
    reference, where it is built, must say the same (multiply_inplace / square_inplace, then add_many)"""
    g = x.shape[1]
    keep, prods = [], []
    for b in range(g):
        cx = side.dev_ct(x[:, b:b + 1], ci, True)
        cy = cx if y is None else side.dev_ct(y[:, b:b + 1], ci, True)
        keep += [cx, cy]
        prods.append(side.ev.multiply(cx, cy, S.Ciphertext(side.ctx)))
    out = side.ev.add_many(prods, S.Ciphertext(side.ctx))
    words, m = out.to_numpy()[:, 0], meta(out)
    if side.ref is not None:
        rs = []
        for b in range(g):
            r = side.ref.ct(ci, x[:, b], True, side.scale, side.cf)
            if y is None:
                side.ref.square_inplace(r)
            else:
                side.ref.multiply_inplace(r, side.ref.ct(ci, y[:, b], True, side.scale, side.cf))
            rs.append(r)
        r = side.ref.add_many(rs)
        i = r.info()
        assert np.array_equal(words, r.data()), ("multiply + add_many and the reference disagree", y is None)
        assert m == (i["is_ntt_form"], i["scale"], i["correction_factor"])
    return words, m


def check(side, what, got_ct, x, y, ci, group):
    batch = x.shape[1]
    got = got_ct.to_numpy()
    assert got.shape == (3, batch // group) + x.shape[2:], (what, got.shape)
    assert got_ct.batch() == batch // group and got_ct.size() == 3 and got_ct.parms_id() == side.ctx.parms_id_at(ci), what
    for o in range(batch // group):
        sl = slice(o * group, (o + 1) * group)
        words, m = expect_group(side, x[:, sl], None if y is None else y[:, sl], ci)
        assert np.array_equal(got[:, o], words), (what, "output item", o)
        assert meta(got_ct) == m, (what, "metadata")


def case_parity(scheme, n, bits, batch, groups, ci=None, seed=5):
    """output item o equals multiply + add_many and the reference; g = 1 is multiply on the whole batch"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    for group in groups:
        assert batch % group == 0
        x, y = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)
        cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
        out = side.ev.dot_items(cx, cy, group)
        check(side, (scheme, n, group), out, x, y, ci, group)
        assert np.array_equal(cx.to_numpy(), x) and np.array_equal(cy.to_numpy(), y), "the operands are only read"
        if group == 1:
            m = side.ev.multiply(cx, cy, S.Ciphertext(side.ctx, batch=batch))
            assert np.array_equal(out.to_numpy(), m.to_numpy()) and meta(out) == meta(m), "group 1 is multiply"
    # group None = the whole batch, into a destination the caller made
    dest = S.Ciphertext(side.ctx, batch=1)
    assert side.ev.dot_items(cx, cy, destination=dest) is dest
    check(side, (scheme, n, "whole batch"), dest, x, y, ci, batch)


def raw_dot(side, ci, x, y, group, slices):
    """shl_dot_items on raw words with a given cut (0: the library's rule); y None: the same pointer twice (the square kernel)
    -> words [3][batch / group][K][N]"""
    _, batch, K, n = x.shape
    a = S.DeviceBuffer.from_numpy(x)
    b = a if y is None else S.DeviceBuffer.from_numpy(y)
    out_words = 3 * (batch // group) * K * n
    r = S.DeviceBuffer(out_words)
    used = C.c_uint64()
    lib = S._native.lib()

    def call(rp, scratch):
        S._native.check(lib.shl_dot_items(side.ctx._h, C.c_uint64(ci), C.c_void_p(a.ptr), C.c_void_p(b.ptr), C.c_void_p(rp), C.c_uint64(batch),
                                          C.c_uint64(group), C.c_uint64(slices), C.c_void_p(scratch), C.byref(used), None))
    call(None, None)   # the slices this will run in
    scratch = S.DeviceBuffer(max(used.value * out_words, 1))
    call(r.ptr, scratch.ptr)
    S.device_synchronize()
    if slices:
        per = -(-group // slices)
        assert used.value == -(-group // per), ("slices run", used.value, slices)
    return r.to_numpy((3, batch // group, K, n))


def case_square(scheme, n, bits, batch=4, group=2, seed=7):
    """the same handle twice: multiply(x, x) + add_many, the reference's square + add_many; through the raw seam the square kernel
    (one pointer twice) and the general kernel on a copy of x give the same words"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    x = side.rand_ct(rng, ci, batch, 2)
    cx = side.dev_ct(x, ci, True)
    out = side.ev.dot_items(cx, cx, group)
    check(side, (scheme, "square"), out, x, None, ci, group)
    assert np.array_equal(cx.to_numpy(), x), "the operand is only read"
    other = side.ev.dot_items(cx, side.dev_ct(x, ci, True), group)
    assert np.array_equal(other.to_numpy(), out.to_numpy()) and meta(other) == meta(out), "a copy of x as the second operand"
    sq, general = raw_dot(side, ci, x, None, group, 1), raw_dot(side, ci, x, x.copy(), group, 1)
    assert np.array_equal(sq, general) and np.array_equal(sq, out.to_numpy()), "square kernel and general kernel"


# ---- flush boundaries: Python-integer arithmetic
def _columns(side, ci, pattern, rng, batch):
    """[2][batch][K][2] words by pattern; the operands repeat these two columns along N"""
    q = side.q(ci)
    qk = np.broadcast_to(q[:, None], (2, batch, q.size, 2))
    if pattern == "max":
        return (qk - 1).astype(np.uint64)
    if pattern == "half":
        return (qk // 2 + np.indices(qk.shape)[-1].astype(np.uint64)).astype(np.uint64)   # q / 2 next to q / 2 + 1
    if pattern == "alternating":   # q - 1 and 0 in turn along the items and along N
        idx = np.indices(qk.shape)
        return np.where((idx[1] + idx[3]) % 2 == 0, qk - 1, 0).astype(np.uint64)
    return (rng.integers(0, 2 ** 63, qk.shape, dtype=np.uint64) % qk).astype(np.uint64)


def _want(xo, yo, q, group, out_items):
    """Python integers: [3][out_items][K][2]"""
    K = len(q)
    want = np.zeros((3, out_items, K, 2), dtype=np.uint64)
    for o in range(out_items):
        sl = slice(o * group, (o + 1) * group)
        for k in range(K):
            x0, x1, y0, y1 = xo[0, sl, k], xo[1, sl, k], yo[0, sl, k], yo[1, sl, k]
            want[0, o, k] = ((x0 * y0).sum(axis=0) % q[k]).astype(np.uint64)
            want[1, o, k] = ((x0 * y1 + x1 * y0).sum(axis=0) % q[k]).astype(np.uint64)
            want[2, o, k] = ((x1 * y1).sum(axis=0) % q[k]).astype(np.uint64)
    return want


def case_flush(n, bits, group, patterns=("max", "alternating", "half", "random"), out_items=1, seed=61):
    """operands whose words are all q - 1 (the middle sum of a run reaches 256 (q - 1)^2), the structured cases alternating / q / 2
    and random ones, in a group around the flush interval: every word equals the sum formed with Python integers - for the
    evaluator's own schedule, for the one-launch form whose threads add the whole group, and for the square kernel"""
    assert library_flush_interval() == DOT_ITEMS_FLUSH == 128, "the interval the derivation gives is the library's"
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, batch = side.first, group * out_items
    q = [int(v) for v in side.q(ci)]
    for pattern in patterns:
        xc = _columns(side, ci, pattern, rng, batch)
        yc = _columns(side, ci, pattern if pattern != "alternating" else "max", rng, batch)
        x, y = np.ascontiguousarray(np.tile(xc, n // 2)), np.ascontiguousarray(np.tile(yc, n // 2))
        assert np.array_equal(x[..., 2:4], xc) and x.shape == (2, batch, len(q), n)
        xo, yo = xc.astype(object), yc.astype(object)
        want, want_sq = np.tile(_want(xo, yo, q, group, out_items), n // 2), np.tile(_want(xo, xo, q, group, out_items), n // 2)
        cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
        assert np.array_equal(side.ev.dot_items(cx, cy, group).to_numpy(), want), (pattern, group, "evaluator")
        assert np.array_equal(side.ev.dot_items(cx, cx, group).to_numpy(), want_sq), (pattern, group, "evaluator, square")
        assert np.array_equal(raw_dot(side, ci, x, y, group, 1), want), (pattern, group, "one launch")
        assert np.array_equal(raw_dot(side, ci, x, None, group, 1), want_sq), (pattern, group, "one launch, square")


# ---- the sliced path
def case_sliced(scheme, n, bits, batch, group, slice_counts, seed=67):
    """the same inputs through the one-launch form and through forced cuts - slice counts that do not divide the group among them -
    give identical words, which are those of multiply + add_many; so does the Evaluator's own choice"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    assert any(group % s for s in slice_counts), "a slice count that does not divide the group"
    x, y = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)
    for other in (y, None):
        one = raw_dot(side, ci, x, other, group, 1)
        for s in slice_counts:
            assert np.array_equal(raw_dot(side, ci, x, other, group, s), one), ("sliced", other is None, s)
        cx = side.dev_ct(x, ci, True)
        out = side.ev.dot_items(cx, cx if other is None else side.dev_ct(y, ci, True), group)
        assert np.array_equal(out.to_numpy(), one), ("the evaluator's choice", other is None)
        check(side, (scheme, "sliced", other is None), out, x, other, ci, group)


def case_natural_slices(scheme, n, bits, group, seed=71):
    """no forcing: by the documented rule a batch of one group is cut (asserted from the rule and through slices_used, not
    assumed), several groups of the same size are not; the first group's words agree and are those of multiply + add_many"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    pairs = K * n // 2
    many = -(-SLICE_BELOW // pairs)
    assert rule_slices(pairs, group) > 1 and rule_slices(many * pairs, group) == 1, ("the rule does not separate these shapes", pairs, many)
    used = C.c_uint64()
    for batch, want in ((group, rule_slices(pairs, group)), (many * group, 1)):
        S._native.check(S._native.lib().shl_dot_items(side.ctx._h, C.c_uint64(ci), None, None, None, C.c_uint64(batch), C.c_uint64(group),
                                                      C.c_uint64(0), None, C.byref(used), None))
        assert used.value == want, ("the library's rule is the documented one", batch, used.value)
    x, y = side.rand_ct(rng, ci, many * group, 2), side.rand_ct(rng, ci, many * group, 2)
    big = side.ev.dot_items(side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), group)
    small = side.ev.dot_items(side.dev_ct(x[:, :group], ci, True), side.dev_ct(y[:, :group], ci, True), group)
    assert np.array_equal(big.to_numpy()[:, :1], small.to_numpy()), "one launch and the cut disagree"
    check(side, (scheme, "natural slices"), small, x[:, :group], y[:, :group], ci, group)


# ---- the destination
def case_out_of_place_and_reuse(scheme, n, bits, batch=6, group=3, seed=17):
    """the operands are unchanged; a destination that held another size, level or form is reshaped to size 3 at the operands' level"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, out = side.first, batch // group
    x, y = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)
    want = None
    for dest in (S.Ciphertext(side.ctx, batch=out), side.dev_ct(side.rand_ct(rng, 0, out, 2), 0, True),
                 side.dev_ct(side.rand_ct(rng, ci, out, 4), ci, False)):
        cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
        got = side.ev.dot_items(cx, cy, group, dest)
        assert got is dest and np.array_equal(cx.to_numpy(), x) and np.array_equal(cy.to_numpy(), y), "an operand changed"
        assert meta(cx) == meta(cy) == (True, side.scale, side.cf)
        assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), 3, out)
        if want is None:
            check(side, (scheme, "out of place"), dest, x, y, ci, group)
            want = dest.to_numpy(), meta(dest)
        assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], "reshaped destination"
    # the last destination, now of size 3, is used again with the operands swapped
    again = side.ev.dot_items(side.dev_ct(y, ci, True), side.dev_ct(x, ci, True), group, dest)
    assert again is dest
    check(side, (scheme, "reused destination, operands swapped"), dest, y, x, ci, group)


# ---- errors
def case_errors(scheme, n, bits, batch=6, group=3):
    """every refusal of the contract returns its HRESULT and leaves the destination untouched; a valid call afterwards works"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, lib = side.first, S._native.lib()
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    out = batch // group
    x, y = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)
    cx, cy = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
    dest = side.dev_ct(side.rand_ct(rng, ci, out, 2), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)

    def dot(ev_h, x_h, y_h, g, dest_h):
        return lib.Evaluator_DotItems(ev_h, x_h, y_h, C.c_uint64(g), dest_h) & 0xFFFFFFFF

    ev = side.ev._h
    assert dot(None, cx._h, cy._h, group, dest._h) == POINTER and dot(ev, None, cy._h, group, dest._h) == POINTER, "NULL handles"
    assert dot(ev, cx._h, None, group, dest._h) == POINTER and dot(ev, cx._h, cy._h, group, None) == POINTER, "NULL handles"
    invalid = side.dev_ct(x, ci, True)
    invalid.set_scale(0.0 if scheme == "ckks" else 2.0)   # is_metadata_valid_for fails
    foreign = Side(scheme, n, bits).dev_ct(x, ci, True)
    lower = side.dev_ct(side.rand_ct(rng, ci - 1, batch, 2), ci - 1, True)
    fewer = side.dev_ct(x[:, :group], ci, True)
    coeff = side.dev_ct(x, ci, False)
    three = side.dev_ct(side.rand_ct(rng, ci, batch, 3), ci, True)
    for bad, what in ((invalid, "an invalid ciphertext"), (foreign, "a ciphertext of another context"), (lower, "mismatched levels"),
                      (fewer, "mismatched batches"), (coeff, "coefficient form"), (three, "a size other than 2")):
        assert dot(ev, bad._h, cy._h, group, dest._h) == INVALID and dot(ev, cx._h, bad._h, group, dest._h) == INVALID, what
    assert dot(ev, three._h, three._h, group, dest._h) == INVALID, "a size other than 2, squared"
    for g in (0, 4, batch + 1):
        assert dot(ev, cx._h, cy._h, g, dest._h) == INVALID, ("group", g)
    assert dot(ev, cx._h, cy._h, group, S.Ciphertext(side.ctx, batch=out + 1)._h) == INVALID, "destination's batch"
    assert dot(ev, cx._h, cy._h, 1, cx._h) == INVALID and dot(ev, cx._h, cy._h, 1, cy._h) == INVALID, "destination == an operand"
    assert dot(ev, cx._h, cx._h, 1, cx._h) == INVALID, "destination == the squared operand"
    if scheme == "ckks":
        big = side.dev_ct(x, ci, True)
        big.set_scale(2.0 ** 100)   # valid by itself; the product's 2^200 is beyond the level's modulus
        assert dot(ev, big._h, big._h, group, dest._h) == INVALID, "scale out of bounds"
    _expect(ValueError, lambda: side.ev.dot_items(cx, cy, 4), "a group that does not divide the batch, no destination")
    assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
    assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
    assert np.array_equal(cx.to_numpy(), x) and np.array_equal(cy.to_numpy(), y)
    # a valid call afterwards
    side.ev.dot_items(cx, cy, group, dest)
    check(side, "after the failures", dest, x, y, ci, group)


def case_bfv_refused(n, bits, batch=2):
    """BFV's product rounds per item: the fused sum could not be the reference's words, so the scheme is refused as multiply refuses
    an unknown scheme - in either form of the operands, with the destination untouched"""
    side = Side("bfv", n, bits)
    rng = np.random.default_rng(37)
    ci = side.first
    x = side.rand_ct(rng, ci, batch, 2)
    dest = side.dev_ct(side.rand_ct(rng, ci, 1, 2), ci, False)
    snapshot = dest.to_numpy()
    for ntt in (False, True):
        c = side.dev_ct(x, ci, ntt)
        hr = S._native.lib().Evaluator_DotItems(side.ev._h, c._h, c._h, C.c_uint64(batch), dest._h) & 0xFFFFFFFF
        assert hr == S._native.E_INVALIDARG, ("BFV", ntt, hex(hr))
    _expect(S.InvalidArgument, lambda: side.ev.dot_items(c, c), "BFV")
    assert np.array_equal(dest.to_numpy(), snapshot) and dest.size() == 2 and not dest.is_ntt_form()


def case_transparent_check(scheme, n, bits, batch=4):
    """with the check on the RESULT batch is checked: an all-zero second and third polynomial is refused (and computed with the
    check off), a proper result passes"""
    side = Side(scheme, n, bits)
    ci = side.first
    x, y = side.rand_ct(np.random.default_rng(3), ci, batch, 2), side.rand_ct(np.random.default_rng(4), ci, batch, 2)
    x0, y0 = x.copy(), y.copy()
    x0[1] = 0
    y0[1] = 0
    zero = side.ev.dot_items(side.dev_ct(x0, ci, True), side.dev_ct(y0, ci, True)).to_numpy()
    assert not np.any(zero[1:]) and np.any(zero[0])
    side.ev.set_transparent_check(True)
    try:
        _expect(S.LogicError, lambda: side.ev.dot_items(side.dev_ct(x0, ci, True), side.dev_ct(y0, ci, True)), "transparent result")
        out = side.ev.dot_items(side.dev_ct(x, ci, True), side.dev_ct(y, ci, True), 2)
    finally:
        side.ev.set_transparent_check(False)
    check(side, (scheme, "transparent check on"), out, x, y, ci, 2)


# ---- pending state
def case_pending(n, bits, batch=4, group=2, seed=73):
    """operand x is the result of relinearize with its key-switch tail still deferred; operand y is an input of a deferred product
    that has not been formed, and y is overwritten after the call.  The words are those of the eager sequence
    (SEALHIP_LAZY_PRODUCT=0 SEALHIP_KS_EAGER_TAIL=1) and of multiply + add_many on the settled operands; the deferred product still
    gets y's words of before the overwrite"""
    from parity_cases import _Env
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    a, b, yw = (side.rand_ct(rng, ci, batch, 2) for _ in range(3))

    def run():
        ca, cb, y = side.dev_ct(a, ci, True), side.dev_ct(b, ci, True), side.dev_ct(yw, ci, True)
        x = side.ev.relinearize_inplace(side.ev.multiply(ca, cb, S.Ciphertext(side.ctx, batch=batch)), rlk)   # a deferred tail
        w = side.ev.multiply(y, cb, S.Ciphertext(side.ctx, batch=batch))                                      # a deferred product reading y
        out = side.ev.dot_items(x, y, group)
        lazy_result = (out.size(), out.batch(), meta(out))
        side.ev.add_inplace(y, cb)                                                                            # y is overwritten afterwards
        return [c.to_numpy() for c in (out, x, w, y)], lazy_result

    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT_MIN_WGS=0, SEALHIP_LAZY_PRODUCT=None, SEALHIP_KS_EAGER_TAIL=None):
        tails0, products0 = S.tail_stats(), S.product_stats()
        lazy, shape = run()
        tails1, products1 = S.tail_stats(), S.product_stats()
    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT=0, SEALHIP_KS_EAGER_TAIL=1):
        eager, shape_e = run()
    if two_pass_ring(n):   # the sizes at which the library defers
        assert tails1[1] - tails0[1] >= 1, "dot_items completed a deferred tail"
        assert products1[1] - products0[1] >= 1, "the product reading y was formed when y was overwritten"
    assert shape == shape_e == (3, batch // group, (True, side.scale ** 3, 1))
    for got, want, what in zip(lazy, eager, ("dot_items", "relinearized x", "the product reading y", "y overwritten")):
        assert np.array_equal(got, want), what
    # the settled composition on the words the operands had
    x_settled = lazy[1]
    q = side.q(ci)[None, :, None]
    assert np.array_equal(lazy[3], (yw + b) % q), "y after the overwrite"
    side.scale, saved = side.scale ** 2, side.scale   # x carries the product's scale
    try:
        cx = side.dev_ct(x_settled, ci, True)
    finally:
        side.scale = saved
    prod = side.ev.multiply(cx, side.dev_ct(yw, ci, True), S.Ciphertext(side.ctx, batch=batch))
    want = side.ev.sum_items(prod, group)
    assert np.array_equal(lazy[0], want.to_numpy()) and shape[2] == meta(want), "multiply + sum_items on the settled operands"


# ---- capture
def case_capture(n, bits, batch, group, seed=47):
    """CKKS: a sliced dot_items recorded in a graph; both operands' words are refreshed in place before each replay and the replay
    equals the eager result"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    cx, cy = side.dev_ct(side.rand_ct(rng, ci, batch, 2), ci, True), side.dev_ct(side.rand_ct(rng, ci, batch, 2), ci, True)
    out = batch // group
    dot, dot_e = S.Ciphertext(side.ctx, batch=out), S.Ciphertext(side.ctx, batch=out)
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        for name, c in (("x", cx), ("y", cy)):
            w = np.ascontiguousarray(side.rand_ct(rng, ci, batch, 2))
            S._native.check(h2d(C.c_void_p(c.device_ptr()[0]), w.ctypes.data_as(C.c_void_p), C.c_uint64(w.nbytes)))
            state[name] = w

    def step(d=dot):
        side.ev.dot_items(cx, cy, group, d)

    refresh()
    step()   # eager once
    graph = side.ev.capture(step)
    for trial in range(2):
        refresh()
        graph.launch()
        replay = dot.to_numpy()
        step(dot_e)
        assert np.array_equal(replay, dot_e.to_numpy()) and meta(dot) == meta(dot_e), ("graph replay", trial)
        assert np.array_equal(cx.to_numpy(), state["x"]) and np.array_equal(cy.to_numpy(), state["y"]), "the operands are only read"
    check(side, "replayed dot product", dot, state["x"], state["y"], ci, group)


# ---- pipeline (the reference's keys and objects)
def case_pipeline_ckks(n, bits, batch, group, seed=41):
    """encode_device -> encrypt_symmetric_device (two batches) -> dot_items -> relinearize -> rescale_to_next: after every stage the
    ciphertext words of output item o equal the reference's per-item multiply -> add_many -> relinearize -> rescale on the same
    fresh ciphertexts"""
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
    a, b = rng.standard_normal((batch, slots)), rng.standard_normal((batch, slots))
    wa = enc.encode_device(S.DeviceBuffer.from_array(a), batch, pid, scale)
    wb = enc.encode_device(S.DeviceBuffer.from_array(b), batch, pid, scale)
    side.enc.set_seed(None)
    A = side.enc.encrypt_symmetric_device(wa, batch, pid, scale)
    B = side.enc.encrypt_symmetric_device(wb, batch, pid, scale)
    fresh = [(A.save_bytes(item=k), B.save_bytes(item=k)) for k in range(batch)]
    R = ev.dot_items(A, B, group)
    assert (R.batch(), R.size(), R.scale()) == (batch // group, 3, scale * scale)
    summed = R.to_numpy()
    ev.relinearize_inplace(R, rlk)
    relinearized = R.to_numpy()
    ev.rescale_to_next_inplace(R)
    rescaled = R.to_numpy()
    for o in range(batch // group):
        rs = []
        for k in range(o * group, (o + 1) * group):
            ra, rb = ref.ct_load(fresh[k][0])[0], ref.ct_load(fresh[k][1])[0]
            rs.append(ref.multiply_inplace(ra, rb))
        r = ref.add_many(rs)
        assert np.array_equal(summed[:, o], r.data()), ("dot_items", o)
        ref.relinearize_inplace(r)
        assert np.array_equal(relinearized[:, o], r.data()), ("relinearize", o)
        ref.rescale_to_next_inplace(r)
        assert np.array_equal(rescaled[:, o], r.data()) and R.scale() == r.info()["scale"], ("rescale", o)
