"""Sums over the items of a device-resident batch (Evaluator_SumItems / Evaluator_DotPlainDevice), shared by the CPU (emulated
kernels) and `-m gpu` suites.  Byte equality, per output item, against two yardsticks: the library's unchanged per-object forms on
batches of one (multiply_plain_inplace, then add_many) and, where oracle/_ref is built, the REAL reference doing the same on its own
objects.  The flush-boundary cases compare with Python-integer arithmetic, which depends on neither library.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import sealref
from harness import two_pass_ring
from plain_batch_cases import Side, _client, _expect

# include/sealhip.h, batch_reduce_kernels.hip: with primes below 2^60, 2^(64 - 60) words fit 64 bits and 2^(128 - 120) products 128 bits
SUM_FLUSH, DOT_FLUSH = 1 << (64 - 60), 1 << (128 - 2 * 60)
# include/sealhip.h: a result of fewer than 2^17 output pairs whose groups have at least 8 items is computed in slices
SLICE_BELOW, SLICE_MIN_GROUP, MAX_SLICES = 1 << 17, 8, 64


def library_flush_intervals():
    a, b = C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_reduce_flush_intervals(C.byref(a), C.byref(b)))
    return a.value, b.value


def forms(scheme):
    """ciphertext forms sum_items takes: every form add accepts (the native one and the other)"""
    return (True, False) if scheme != "bfv" else (False, True)


def meta(ct):
    return ct.is_ntt_form(), ct.scale(), ct.correction_factor()


def expect_group(side, x, pl, ci, ct_ntt):
    """x [size][g][K][N] (and pl [g][K][N]: the dot product) through the per-object forms on batches of one -> (words [size][K][N],
    metadata); the reference, where it is built, must say the same"""
    g = x.shape[1]
    cts = [side.dev_ct(x[:, b:b + 1], ci, ct_ntt) for b in range(g)]
    if pl is not None:
        for b in range(g):
            side.ev.multiply_plain_inplace(cts[b], side.plaintext(pl[b], ci, True))
    out = side.ev.add_many(cts, S.Ciphertext(side.ctx))
    words, m = out.to_numpy()[:, 0], meta(out)
    if side.ref is not None:
        rs = [side.ref.ct(ci, x[:, b], ct_ntt, side.scale, side.cf) for b in range(g)]
        if pl is not None:
            for b in range(g):
                side.ref.multiply_plain_inplace(rs[b], side.ref.pt(pl[b], ci, side.scale))
        r = side.ref.add_many(rs)
        i = r.info()
        assert np.array_equal(words, r.data()), ("per-object forms and reference disagree", ct_ntt, pl is not None)
        assert m == (i["is_ntt_form"], i["scale"], i["correction_factor"])
    return words, m


def check(side, what, got_ct, x, pl, ci, ct_ntt, group):
    size, batch = x.shape[:2]
    got = got_ct.to_numpy()
    assert got.shape == (size, batch // group) + x.shape[2:], (what, got.shape)
    assert got_ct.batch() == batch // group and got_ct.size() == size and got_ct.parms_id() == side.ctx.parms_id_at(ci), what
    for o in range(batch // group):
        sl = slice(o * group, (o + 1) * group)
        words, m = expect_group(side, x[:, sl], None if pl is None else pl[sl], ci, ct_ntt)
        assert np.array_equal(got[:, o], words), (what, "output item", o)
        assert meta(got_ct) == m, (what, "metadata")


def case_parity(scheme, n, bits, batch, groups, sizes=(2, 3), ci=None, seed=5):
    """sum_items in every form add accepts and dot_plain_device NTT x NTT: output item o equals the per-object forms and the reference"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first if ci is None else ci
    for size in sizes:
        for group in groups:
            assert batch % group == 0
            for ct_ntt in forms(scheme):
                x = side.rand_ct(rng, ci, batch, size)
                c = side.dev_ct(x, ci, ct_ntt)
                out = side.ev.sum_items(c, group)
                check(side, (scheme, n, "sum", ct_ntt, size, group), out, x, None, ci, ct_ntt, group)
                if group == 1:
                    assert np.array_equal(out.to_numpy(), x), "group 1 is a copy"
            x = side.rand_ct(rng, ci, batch, size)
            pl = side.rand_plain(rng, ci, batch, True)
            c, buf = side.dev_ct(x, ci, True), S.DeviceBuffer.from_numpy(pl)
            out = side.ev.dot_plain_device(c, buf, side.scale, group)
            check(side, (scheme, n, "dot", size, group), out, x, pl, ci, True, group)
            if group == 1:
                m = side.ev.multiply_plain_device(side.dev_ct(x, ci, True), buf, True, side.scale)
                assert np.array_equal(out.to_numpy(), m.to_numpy()) and meta(out) == meta(m), "group 1 is multiply_plain_device"
    # group None = the whole batch, into a destination the caller made
    x = side.rand_ct(rng, ci, batch, 2)
    dest = S.Ciphertext(side.ctx, batch=1)
    assert side.ev.sum_items(side.dev_ct(x, ci, forms(scheme)[0]), destination=dest) is dest
    check(side, (scheme, n, "sum", "whole batch"), dest, x, None, ci, forms(scheme)[0], batch)


# ---- flush boundaries: Python-integer arithmetic
def _columns(side, ci, pattern, rng, shape):
    """[...][K][2] words by pattern; the operands repeat these two columns along N"""
    q = side.q(ci)
    qk = np.broadcast_to(q[:, None], shape + (q.size, 2))
    if pattern == "max":
        return (qk - 1).astype(np.uint64)
    if pattern == "half":
        return (qk // 2 + np.indices(qk.shape)[-1].astype(np.uint64)).astype(np.uint64)   # q / 2 next to q / 2 + 1
    if pattern == "alternating":   # q - 1 and 0 in turn along the items and along N
        idx = np.indices(qk.shape)
        return np.where((idx[-3] + idx[-1]) % 2 == 0, qk - 1, 0).astype(np.uint64)
    return (rng.integers(0, 2 ** 63, qk.shape, dtype=np.uint64) % qk).astype(np.uint64)


def flush_groups():
    out = []
    for f in (SUM_FLUSH, DOT_FLUSH):
        out += [f - 1, f, f + 1]
    return out + [2 * DOT_FLUSH + 3]


def case_flush(n, bits, group, patterns=("max", "alternating", "half", "random"), out_items=1, size=2, seed=61):
    """operands whose words are all q - 1 (and the structured worst cases alternating / q / 2, and random ones) in groups around
    the flush intervals: every word equals the sum formed with Python integers"""
    assert library_flush_intervals() == (SUM_FLUSH, DOT_FLUSH), "the intervals the derivation gives are the library's"
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, batch = side.first, group * out_items
    q = [int(v) for v in side.q(ci)]
    K = len(q)
    for pattern in patterns:
        xc = _columns(side, ci, pattern, rng, (size, batch))    # [size][batch][K][2]
        pc = _columns(side, ci, pattern if pattern != "alternating" else "max", rng, (batch,))
        x = np.ascontiguousarray(np.tile(xc, n // 2))
        pl = np.ascontiguousarray(np.tile(pc, n // 2))
        assert np.array_equal(x[..., 2:4], xc) and x.shape == (size, batch, K, n)
        xo, po = xc.astype(object), pc.astype(object)
        want_sum = np.zeros((size, out_items, K, 2), dtype=np.uint64)
        want_dot = np.zeros((size, out_items, K, 2), dtype=np.uint64)
        for o in range(out_items):
            sl = slice(o * group, (o + 1) * group)
            for k in range(K):
                want_sum[:, o, k] = (xo[:, sl, k].sum(axis=1) % q[k]).astype(np.uint64)
                want_dot[:, o, k] = ((xo[:, sl, k] * po[None, sl, k]).sum(axis=1) % q[k]).astype(np.uint64)
        c, buf = side.dev_ct(x, ci, True), S.DeviceBuffer.from_numpy(pl)
        # the evaluator's own schedule (a small result is cut into slices shorter than the intervals) and the one-launch form, whose
        # threads add the whole group and so cross every boundary
        for how in ("evaluator", "one launch"):
            if how == "evaluator":
                got_sum = side.ev.sum_items(c, group).to_numpy()
                got_dot = side.ev.dot_plain_device(c, buf, side.scale, group).to_numpy()
            else:
                got_sum = raw_reduce(side, ci, x, None, group, 1)
                got_dot = raw_reduce(side, ci, x, pl, group, 1)
            assert np.array_equal(got_sum, np.tile(want_sum, n // 2)), ("sum", pattern, group, how)
            assert np.array_equal(got_dot, np.tile(want_dot, n // 2)), ("dot", pattern, group, how)


# ---- the sliced path
def rule_slices(threads, group):
    """include/sealhip.h restated: slices the library runs a launch of `threads` output pairs in"""
    if threads >= SLICE_BELOW or group < SLICE_MIN_GROUP:
        return 1
    s = min(-(-(1 << 19) // threads), group // 4, MAX_SLICES)
    per = -(-group // s)
    return -(-group // per)


def raw_reduce(side, ci, x, pl, group, slices):
    """shl_reduce_items on raw words with a given cut (0: the library's rule) -> words [size][batch / group][K][N]"""
    size, batch, K, n = x.shape
    a = S.DeviceBuffer.from_numpy(x)
    p = S.DeviceBuffer.from_numpy(pl) if pl is not None else None
    out_words = size * (batch // group) * K * n
    r = S.DeviceBuffer(out_words)
    used = C.c_uint64()
    lib = S._native.lib()

    def call(rp, scratch):
        S._native.check(lib.shl_reduce_items(side.ctx._h, C.c_uint64(ci), C.c_void_p(a.ptr), C.c_void_p(p.ptr if p else None), C.c_void_p(rp),
                                             C.c_uint64(size), C.c_uint64(batch), C.c_uint64(group), C.c_uint64(slices),
                                             C.c_void_p(scratch), C.byref(used), None))
    call(None, None)   # the slices this will run in
    scratch = S.DeviceBuffer(max(used.value * out_words, 1))
    call(r.ptr, scratch.ptr)
    S.device_synchronize()
    if slices:
        per = -(-group // slices)
        assert used.value == -(-group // per), ("slices run", used.value, slices)
    return r.to_numpy((size, batch // group, K, n))


def case_sliced(scheme, n, bits, batch, group, slice_counts, size=3, seed=67):
    """the same inputs through the one-launch form and through forced cuts - slice counts that do not divide the group among them -
    give identical words, which are the per-object forms'; so does the Evaluator's own choice"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    assert any(group % s for s in slice_counts), "a slice count that does not divide the group"
    x = side.rand_ct(rng, ci, batch, size)
    pl = side.rand_plain(rng, ci, batch, True)
    for plain in (None, pl):
        one = raw_reduce(side, ci, x, plain, group, 1)
        for s in slice_counts:
            assert np.array_equal(raw_reduce(side, ci, x, plain, group, s), one), ("sliced", plain is not None, s)
        c = side.dev_ct(x, ci, True)
        out = side.ev.sum_items(c, group) if plain is None else side.ev.dot_plain_device(c, S.DeviceBuffer.from_numpy(pl), side.scale, group)
        assert np.array_equal(out.to_numpy(), one), ("the evaluator's choice", plain is not None)
        check(side, (scheme, "sliced", plain is not None), out, x, plain, ci, True, group)


def case_plane_counts(n, bits, sizes=(1, 4, 5), batch=6, group=3, patterns=("max", "random"), seed=79):
    """plane counts the Evaluator's cases do not reach, through the raw seam: one plane (the product's single-plane kernel), four and
    five (the product takes its planes three at a time, then one or two; the sum has all of them in its grid), in one launch and in
    two slices - which do not divide the group of three, so the second slice is short.  Every word equals the sum formed with
    Python integers"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, out_items = side.first, batch // group
    q = [int(v) for v in side.q(ci)]
    K = len(q)
    for size in sizes:
        for pattern in patterns:
            xc = _columns(side, ci, pattern, rng, (size, batch))    # [size][batch][K][2]
            pc = _columns(side, ci, pattern, rng, (batch,))
            x = np.ascontiguousarray(np.tile(xc, n // 2))
            pl = np.ascontiguousarray(np.tile(pc, n // 2))
            assert np.array_equal(x[..., -2:], xc) and x.shape == (size, batch, K, n)
            xo, po = xc.astype(object), pc.astype(object)
            want_sum = np.zeros((size, out_items, K, 2), dtype=np.uint64)
            want_dot = np.zeros((size, out_items, K, 2), dtype=np.uint64)
            for o in range(out_items):
                sl = slice(o * group, (o + 1) * group)
                for k in range(K):
                    want_sum[:, o, k] = (xo[:, sl, k].sum(axis=1) % q[k]).astype(np.uint64)
                    want_dot[:, o, k] = ((xo[:, sl, k] * po[None, sl, k]).sum(axis=1) % q[k]).astype(np.uint64)
            for slices in (1, 2):
                assert np.array_equal(raw_reduce(side, ci, x, None, group, slices), np.tile(want_sum, n // 2)), ("sum", size, pattern, slices)
                assert np.array_equal(raw_reduce(side, ci, x, pl, group, slices), np.tile(want_dot, n // 2)), ("dot", size, pattern, slices)


def case_natural_slices(scheme, n, bits, group, size=2, seed=71):
    """no forcing: by the documented rule a batch of one group is cut (asserted from the rule, not assumed), several groups of the
    same size are not (fewer items per launch than the rule asks for would be: checked too); the first group's words agree"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    pairs = K * n // 2
    many = -(-SLICE_BELOW // pairs)
    assert rule_slices(pairs, group) > 1 and rule_slices(many * pairs, group) == 1, ("the rule does not separate these shapes", pairs, many)
    x = side.rand_ct(rng, ci, many * group, size)
    pl = side.rand_plain(rng, ci, many * group, True)
    used = C.c_uint64()
    S._native.check(S._native.lib().shl_reduce_items(side.ctx._h, C.c_uint64(ci), None, C.c_void_p(1), None, C.c_uint64(size), C.c_uint64(group),
                                                     C.c_uint64(group), C.c_uint64(0), None, C.byref(used), None))
    assert used.value == rule_slices(pairs, group), ("the library's rule is the documented one", used.value)
    big = side.ev.dot_plain_device(side.dev_ct(x, ci, True), S.DeviceBuffer.from_numpy(pl), side.scale, group)
    small = side.ev.dot_plain_device(side.dev_ct(x[:, :group], ci, True), S.DeviceBuffer.from_numpy(pl[:group]), side.scale, group)
    assert np.array_equal(big.to_numpy()[:, :1], small.to_numpy()), "one launch and the cut disagree"
    check(side, (scheme, "natural slices"), small, x[:, :group], pl[:group], ci, True, group)
    big = side.ev.sum_items(side.dev_ct(x, ci, True), group)
    small = side.ev.sum_items(side.dev_ct(x[:, :group], ci, True), group)
    assert np.array_equal(big.to_numpy()[:, :1], small.to_numpy()), "one launch and the cut disagree (sum)"


# ---- out of place only
def case_out_of_place(scheme, n, bits, batch=6, group=3, seed=17):
    """the operand is unchanged; a destination of another level, size or context's worth of words is reshaped"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(seed)
    ci, ntt = side.first, True
    x = side.rand_ct(rng, ci, batch, 3)
    pl = side.rand_plain(rng, ci, batch, True)
    buf = S.DeviceBuffer.from_numpy(pl)
    out = batch // group
    for op in ("sum", "dot"):
        want = None
        for dest in (S.Ciphertext(side.ctx, batch=out), side.dev_ct(side.rand_ct(rng, 0, out, 2), 0, ntt),
                     side.dev_ct(side.rand_ct(rng, ci, out, 4), ci, not ntt)):
            src = side.dev_ct(x, ci, ntt)
            got = side.ev.sum_items(src, group, dest) if op == "sum" else side.ev.dot_plain_device(src, buf, side.scale, group, dest)
            assert got is dest and np.array_equal(src.to_numpy(), x), ("encrypted changed", op)
            assert meta(src) == (ntt, side.scale, side.cf)
            assert (dest.parms_id(), dest.size(), dest.batch()) == (side.ctx.parms_id_at(ci), 3, out)
            if want is None:
                check(side, (scheme, "out of place", op), dest, x, pl if op == "dot" else None, ci, ntt, group)
                want = dest.to_numpy(), meta(dest)
            assert np.array_equal(dest.to_numpy(), want[0]) and meta(dest) == want[1], ("reshaped destination", op)


# ---- errors
def case_errors(scheme, n, bits, batch=6, group=3):
    """every check returns its HRESULT and leaves the destination untouched; a valid call afterwards works"""
    side = Side(scheme, n, bits)
    rng = np.random.default_rng(31)
    ci, lib = side.first, S._native.lib()
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    out = batch // group
    x = side.rand_ct(rng, ci, batch, 2)
    pl = side.rand_plain(rng, ci, batch, True)
    buf = S.DeviceBuffer.from_numpy(pl)
    ct = side.dev_ct(x, ci, True)
    dest = side.dev_ct(side.rand_ct(rng, ci, out, 3), ci, True)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch()) + meta(dest)
    wrong_batch = S.Ciphertext(side.ctx, batch=out + 1)
    foreign = Side(scheme, n, bits).dev_ct(x, ci, True)
    invalid = side.dev_ct(x, ci, True)
    invalid.set_scale(0.0 if scheme == "ckks" else 2.0)   # is_metadata_valid_for fails

    def rsum(ct_h, g, dest_h):
        return lib.Evaluator_SumItems(side.ev._h, ct_h, C.c_uint64(g), dest_h) & 0xFFFFFFFF

    def rdot(ct_h, ptr, b, g, scale, dest_h):
        return lib.Evaluator_DotPlainDevice(side.ev._h, ct_h, C.c_void_p(ptr), C.c_uint64(b), C.c_uint64(g), C.c_double(scale), dest_h) & 0xFFFFFFFF

    good = (ct._h, buf.ptr, batch, group, side.scale, dest._h)
    assert rsum(None, group, dest._h) == POINTER and rsum(ct._h, group, None) == POINTER, "NULL handles"
    assert rdot(None, *good[1:]) == POINTER and rdot(*good[:5], None) == POINTER, "NULL handles"
    assert lib.Evaluator_SumItems(None, ct._h, C.c_uint64(group), dest._h) & 0xFFFFFFFF == POINTER
    assert rsum(invalid._h, group, dest._h) == INVALID and rdot(invalid._h, *good[1:]) == INVALID, "an invalid ciphertext"
    assert rsum(foreign._h, group, dest._h) == INVALID and rdot(foreign._h, *good[1:]) == INVALID, "a ciphertext of another context"
    for g in (0, 4, batch + 1):
        assert rsum(ct._h, g, dest._h) == INVALID and rdot(*good[:3], g, *good[4:]) == INVALID, ("group", g)
    assert rsum(ct._h, group, wrong_batch._h) == INVALID and rdot(*good[:5], wrong_batch._h) == INVALID, "destination's batch"
    assert rsum(ct._h, 1, ct._h) == INVALID and rdot(ct._h, buf.ptr, batch, 1, side.scale, ct._h) == INVALID, "destination == encrypted"
    assert rdot(*good[:2], batch + 1, *good[3:]) == INVALID and rdot(*good[:2], 0, *good[3:]) == INVALID, "batch != B"
    assert rdot(ct._h, None, *good[2:]) == INVALID, "NULL device_plain"
    assert rdot(ct._h, buf.ptr + 8, *good[2:]) == INVALID, "misaligned device_plain"
    ptr, _ = ct.device_ptr()
    assert rdot(ct._h, ptr + 16, *good[2:]) == INVALID, "device_plain inside encrypted"
    ptr, _ = dest.device_ptr()
    assert rdot(ct._h, ptr + 16, *good[2:]) == INVALID, "device_plain inside destination"
    assert rdot(side.dev_ct(x, ci, False)._h, *good[1:]) == INVALID, "a coefficient-form ciphertext"
    if scheme == "ckks":
        assert rdot(*good[:4], 0.0, dest._h) == INVALID, "CKKS plaintext scale"
        assert rdot(*good[:4], 2.0 ** 400, dest._h) == INVALID, "scale out of bounds"
    small = S.DeviceBuffer(max(pl.size - n, 1))
    _expect(ValueError, lambda: side.ev.dot_plain_device(ct, small, side.scale, group, dest), "too few plaintext words for the level")
    _expect(ValueError, lambda: side.ev.sum_items(ct, 4), "a group that does not divide the batch, no destination")
    assert np.array_equal(dest.to_numpy(), snapshot), "a failed check must leave the destination untouched"
    assert (dest.parms_id(), dest.size(), dest.batch()) + meta(dest) == before
    assert np.array_equal(ct.to_numpy(), x)
    # valid calls afterwards
    side.ev.dot_plain_device(ct, buf, side.scale, group, dest)
    check(side, "after the failures", dest, x, pl, ci, True, group)
    side.ev.sum_items(ct, group, dest)
    check(side, "after the failures", dest, x, None, ci, True, group)


def case_transparent_check(scheme, n, bits, batch=4):
    """an all-zero result is refused when the check is on (and computed when it is off)"""
    side = Side(scheme, n, bits)
    x = side.rand_ct(np.random.default_rng(3), side.first, batch, 2)
    x[1] = 0
    pl = side.rand_plain(np.random.default_rng(4), side.first, batch, True)
    ntt = True
    assert not np.any(side.ev.sum_items(side.dev_ct(x, side.first, ntt)).to_numpy()[1])
    side.ev.set_transparent_check(True)
    try:
        _expect(S.LogicError, lambda: side.ev.sum_items(side.dev_ct(x, side.first, ntt)), "transparent sum")
        _expect(S.LogicError, lambda: side.ev.dot_plain_device(side.dev_ct(x, side.first, ntt), S.DeviceBuffer.from_numpy(pl), side.scale),
                "transparent dot product")
    finally:
        side.ev.set_transparent_check(False)


# ---- pending state
def case_pending(n, bits, batch=4, group=2, seed=73):
    """sum_items of a ciphertext with a pending tensor product, of one with a deferred key-switch tail, and into a destination that
    has a pending product of its own: the words of the eager sequence (SEALHIP_LAZY_PRODUCT=0 SEALHIP_KS_EAGER_TAIL=1)"""
    from parity_cases import _Env
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci, out = side.first, batch // group
    rlk = S.KeyGenerator(side.ctx).create_relin_keys()
    x, y = side.rand_ct(rng, ci, batch, 2), side.rand_ct(rng, ci, batch, 2)

    def run():
        a, b = side.dev_ct(x, ci, True), side.dev_ct(y, ci, True)
        prod = side.ev.multiply(a, b, S.Ciphertext(side.ctx, batch=batch))
        of_product = side.ev.sum_items(prod, group)            # a pending product is formed first
        relin = side.ev.relinearize_inplace(side.ev.multiply(a, b, S.Ciphertext(side.ctx, batch=batch)), rlk)
        of_tail = side.ev.sum_items(relin, group)              # a deferred tail is completed first
        a1, b1 = side.dev_ct(x[:, :out], ci, True), side.dev_ct(y[:, :out], ci, True)   # (alive: a product is formed when an operand goes away)
        dest = side.ev.multiply(a1, b1, S.Ciphertext(side.ctx, batch=out))
        side.ev.sum_items(relin, group, dest)                  # pending state of the destination is discarded
        return [c.to_numpy() for c in (of_product, of_tail, dest, prod, relin)]

    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT_MIN_WGS=0, SEALHIP_LAZY_PRODUCT=None, SEALHIP_KS_EAGER_TAIL=None):
        tails0, products0 = S.tail_stats(), S.product_stats()
        lazy = run()
        tails1, products1 = S.tail_stats(), S.product_stats()
    with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT=0, SEALHIP_KS_EAGER_TAIL=1):
        eager = run()
    if two_pass_ring(n):   # the sizes at which the library defers
        assert tails1[1] - tails0[1] >= 1, "sum_items completed a deferred tail"
        assert products1[1] - products0[1] >= 1, "sum_items formed a pending product"
        assert products1[2] - products0[2] >= 1, "the destination's pending product was discarded"
    for got, want, what in zip(lazy, eager, ("sum of a product", "sum after relinearize", "into a pending destination", "product", "relinearized")):
        assert np.array_equal(got, want), what
    assert np.array_equal(lazy[1], lazy[2])
    q = side.q(ci)[None, :, None]
    for src, got in ((lazy[3], lazy[0]), (lazy[4], lazy[1])):
        for o in range(out):
            acc = np.zeros_like(src[:, 0])
            for b in range(o * group, (o + 1) * group):
                acc = (acc + src[:, b]) % q
            assert np.array_equal(got[:, o], acc), ("the sums are sums", o)


# ---- capture
def case_capture(n, bits, batch, group, seed=47):
    """CKKS: dot_plain_device + sum_items recorded in a graph; ciphertext and plaintext words are refreshed in place before each
    replay and the replay equals the eager result"""
    side = Side("ckks", n, bits)
    rng = np.random.default_rng(seed)
    ci = side.first
    K = len(side.ctx.coeff_modulus_at(ci))
    cx = side.dev_ct(side.rand_ct(rng, ci, batch, 2), ci, True)
    buf = S.DeviceBuffer(batch * K * n)
    out = batch // group
    dot, tot = S.Ciphertext(side.ctx, batch=out), S.Ciphertext(side.ctx, batch=1)
    dot_e, tot_e = S.Ciphertext(side.ctx, batch=out), S.Ciphertext(side.ctx, batch=1)
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        pl = np.ascontiguousarray(side.rand_plain(rng, ci, batch, True))
        x = np.ascontiguousarray(side.rand_ct(rng, ci, batch, 2))
        S._native.check(h2d(C.c_void_p(buf.ptr), pl.ctypes.data_as(C.c_void_p), C.c_uint64(pl.nbytes)))
        S._native.check(h2d(C.c_void_p(cx.device_ptr()[0]), x.ctypes.data_as(C.c_void_p), C.c_uint64(x.nbytes)))
        state["x"], state["pl"] = x, pl

    def step(d=dot, t=tot):
        side.ev.dot_plain_device(cx, buf, side.scale, group, d)
        side.ev.sum_items(d, None, t)

    refresh()
    step()   # eager once
    graph = side.ev.capture(step)
    for trial in range(3):
        refresh()
        graph.launch()
        replay_dot, replay_tot = dot.to_numpy(), tot.to_numpy()
        step(dot_e, tot_e)
        assert np.array_equal(replay_dot, dot_e.to_numpy()) and np.array_equal(replay_tot, tot_e.to_numpy()), ("graph replay", trial)
        assert np.array_equal(cx.to_numpy(), state["x"]), "the operand is only read"
        assert meta(tot) == meta(tot_e) and tot.size() == 2 and tot.batch() == 1
    check(side, "replayed dot product", dot, state["x"], state["pl"], ci, True, group)


# ---- pipelines (the reference's keys and objects)
def case_pipeline_ckks(n, bits, batch, seed=41):
    """encode_device -> encrypt_symmetric_device -> dot_plain_device over the whole batch -> decrypt_batch -> decode_device: the
    ciphertext words and the decoded values equal the reference's doing the same with its own objects"""
    side = _client("ckks", n, bits)
    ref, ev = side.ref, side.d.ev
    enc = S.CKKSEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    pid, ci, slots = side.ctx.first_parms_id(), side.first, n // 2
    scale = 2.0 ** (bits[-2] if len(bits) > 2 else 12)
    a, w = rng.standard_normal((batch, slots)), rng.standard_normal((batch, slots))
    wa = enc.encode_device(S.DeviceBuffer.from_array(a), batch, pid, scale)
    ww = enc.encode_device(S.DeviceBuffer.from_array(w), batch, pid, scale)
    ww_host = ww.to_numpy((batch, side.K(ci), n))
    side.enc.set_seed(None)
    A = side.enc.encrypt_symmetric_device(wa, batch, pid, scale)
    fresh = [A.save_bytes(item=b) for b in range(batch)]
    R = ev.dot_plain_device(A, ww, scale)
    assert R.batch() == 1 and R.scale() == scale * scale
    coeffs, _ = side.dec.decrypt_batch(R)
    got = enc.decode_device(coeffs, 1, R.parms_id(), R.scale()).to_array((1, slots))
    rs = []
    for b in range(batch):
        r, _ = ref.ct_load(fresh[b])
        rs.append(ref.multiply_plain_inplace(r, ref.pt(ww_host[b], ci, scale)))
    r = ref.add_many(rs)
    assert np.array_equal(R.to_numpy()[:, 0], r.data()) and R.scale() == r.info()["scale"], "dot_plain_device"
    want = ref.ckks_decode(ref.decrypt(r), False)
    assert got[0].tobytes() == want.tobytes(), "decode"
    assert np.max(np.abs(got[0] - (a * w).sum(axis=0))) < 1e-2 * batch, "sum_b a_b * w_b"


def case_pipeline_bfv(n, bits, batch, seed=43):
    """BatchEncoder.encode_device -> encrypt_device -> transform_to_ntt -> transform_plain_to_ntt_device -> dot_plain_device ->
    transform_from_ntt -> decrypt_batch -> decode_device: the words equal the reference's, the slots hold sum_b a_b * v_b modulo t"""
    side = _client("bfv", n, bits)
    ref, ev, t = side.ref, side.d.ev, side.t
    be = S.BatchEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    vals = [rng.integers(0, 50, (batch, n), dtype=np.uint64) for _ in range(2)]
    a, v = [be.encode_device(S.DeviceBuffer.from_numpy(x), batch) for x in vals]
    v_host = v.to_numpy((batch, n))
    side.enc.set_seed(None)
    A = side.enc.encrypt_device(a, batch)
    fresh = [A.save_bytes(item=b) for b in range(batch)]
    ev.transform_to_ntt_inplace(A)
    vn = ev.transform_plain_to_ntt_device(v, batch, A.parms_id())
    R = ev.dot_plain_device(A, vn)
    ev.transform_from_ntt_inplace(R)
    coeffs, _ = side.dec.decrypt_batch(R)
    got = be.decode_device(coeffs, 1).to_numpy((1, n))
    rs = []
    for b in range(batch):
        r, _ = ref.ct_load(fresh[b])
        ref.transform_to_ntt_inplace(r)
        rp = ref.pt_transform_to_ntt_inplace(ref.pt(v_host[b]), side.first)
        rs.append(ref.multiply_plain_inplace(r, rp))
    r = ref.transform_from_ntt_inplace(ref.add_many(rs))
    assert np.array_equal(R.to_numpy()[:, 0], r.data()), "dot_plain_device"
    want = np.zeros(n, dtype=np.uint64)
    rd = ref.decrypt(r).data()
    want[: rd.size] = rd
    assert np.array_equal(coeffs.to_numpy((1, n))[0], want), "decrypt"
    assert np.array_equal(got[0], (vals[0] * vals[1]).sum(axis=0) % t), "sum_b a_b * v_b"
