"""Galois sets (GaloisSet_Create / CreateFromSteps; Evaluator_ApplyGaloisSet), shared by the CPU (emulated kernels) and `-m gpu`
suites.  Byte equality, per result item, against two yardsticks: the library's unchanged per-object calls (Evaluator_ApplyGalois /
RotateVector / RotateRows / RotateColumns / ComplexConjugate) on a batch of one holding the source item and, where oracle/_ref is
built, the REAL reference's apply_galois_inplace / rotate_*_inplace with the same keys loaded into both sides.  The set call and the
per-object call share kernels on some routes, so agreement between those two proves less than the reference does; the routes are
asserted through SealHip_GaloisSetStats / GaloisStats / KsChunkStats.
TEST INFRASTRUCTURE: the reference is the checker."""
import ctypes as C

import numpy as np

import seal_amd as S
import sealref
from harness import DeviceSide, two_pass_ring
from oracle import coeff_modulus_create, plain_modulus_batching
from parity_cases import _Env, extreme_key, extreme_slab

KS_ENV = dict(SEALHIP_KS_SPLIT=None, SEALHIP_KS_CHUNK=None, SEALHIP_KS_LANES=None)


def _expect(exc, call, what):
    try:
        call()
    except exc:
        return
    raise AssertionError("%s: no %s" % (what, exc.__name__))


def worst_steps(n):
    """R = 5 from steps: step +1, an identity entry, step -(N/2 - 1), a repeat, and a second identity"""
    return [1, 0, -(n // 2 - 1), 1, 0]


def worst_elts(side):
    """R = 5 from elements, none the identity: step +1, the element 2N - 1 (conjugation / column rotation), step -(N/2 - 1), repeats"""
    return [side.elt(1), 2 * side.n - 1, side.elt(-(side.n // 2 - 1)), side.elt(1), 2 * side.n - 1]


class Side:
    """one scheme on one ring: the device context, the reference's (where built) and Galois keys for `elts` in both.  The keys are
    the reference KeyGenerator's, uniform words without it, or parity_cases.extreme_key words (key_pattern) set on both sides"""

    def __init__(self, scheme, n, bits, steps=(), elts=(), key_pattern=None, seed=7, tbits=20, cheap_keys=False):
        self.scheme, self.n, self.bits = scheme, n, bits
        self.primes = coeff_modulus_create(n, bits)
        self.t = plain_modulus_batching(n, tbits) if scheme != "ckks" else 0
        self.d = DeviceSide(scheme, n, self.primes, self.t)
        self.ctx, self.ev = self.d.ctx, self.d.ev
        self.L = len(self.primes)
        self.first = self.ctx.chain_index(self.ctx.first_parms_id())
        self.ntt = scheme != "bfv"
        self.cf = 3 if scheme == "bgv" else 1
        self.scale = 2.0 ** 20 if scheme == "ckks" else 1.0
        self.rng = np.random.default_rng(seed)
        self.ref = sealref.RefContext(scheme, n, self.primes, self.t) if sealref.available() and not cheap_keys else None
        self.key_elts = sorted(set(list(elts) + [self.elt(s) for s in steps if s]))
        self.glk = S.GaloisKeys(self.ctx)
        self.key_words = {}
        if self.ref is not None and self.key_elts:
            self.ref.keygen_galois_elts(self.key_elts)
        q = np.array(self.primes, dtype=np.uint64)[None, None, :, None]
        base = None
        for k, e in enumerate(self.key_elts):
            index = S.GaloisKeys.get_index(e)
            if key_pattern is not None:
                w = extreme_key(self.primes, self.L - 1, n, key_pattern, seed=seed + k)
                if self.ref is not None:
                    self.ref.set_key("galois", index, w)
            elif self.ref is not None:
                w = self.ref.key("galois", index)
            elif cheap_keys and base is not None:
                w = np.roll(base, k, axis=3)   # (a large ring: one draw, the other keys are its rotations)
            else:
                w = (self.rng.integers(0, 2 ** 63, (self.L - 1, 2, self.L, n), dtype=np.uint64) % q).astype(np.uint64)
                base = w
            self.glk.set_key(index, w)
            self.key_words[e] = w

    def elt(self, step):
        e = C.c_uint32()
        S._native.check(S._native.lib().GaloisTool_GetEltFromStep(self.ctx._h, C.c_int(step), C.byref(e)))
        return e.value

    def K(self, ci):
        return len(self.ctx.coeff_modulus_at(ci))

    def q(self, ci):
        return np.array(self.ctx.coeff_modulus_at(ci), dtype=np.uint64)

    def operand(self, ci, batch, structured=True):
        """[2][batch][K][N]: random items; with `structured` the first items are the suites' worst cases (all q - 1 with alternating,
        q/2 with q/2 + 1), the rest random"""
        q = self.q(ci)
        x = (self.rng.integers(0, 2 ** 63, (2, batch, q.size, self.n), dtype=np.uint64) % q[None, None, :, None]).astype(np.uint64)
        if structured:
            for b, (p0, p1) in enumerate([("qm1", "alt"), ("half", "half1")][: max(batch - 1, 0)]):
                x[0, b], x[1, b] = extreme_slab(q, self.n, p0, seed=3), extreme_slab(q, self.n, p1, seed=5)
        return x

    def dev_ct(self, words, ci, scale=None):
        return S.Ciphertext.from_numpy(self.ctx, words, self.ctx.parms_id_at(ci), self.ntt, self.scale if scale is None else scale, self.cf)

    # ---- the per-object calls
    def single(self, c, entry, dest=None):
        """entry = ("elt", e) | ("step", s): the per-object call on c (any batch) -> destination"""
        dest = S.Ciphertext(self.ctx, batch=c.batch()) if dest is None else dest
        kind, v = entry
        if kind == "elt":
            self.ev.apply_galois(c, v, self.glk, dest)
        elif self.scheme == "ckks":
            self.ev.rotate_vector(c, v, self.glk, dest)
        else:
            self.ev.rotate_rows(c, v, self.glk, dest)
        return dest

    def ref_single(self, words_b, ci, entry, scale=None):
        """the reference on item words_b [2][K][N] -> (words, info) or None where it refuses the result as transparent"""
        r = self.ref.ct(ci, words_b, self.ntt, self.scale if scale is None else scale, self.cf)
        kind, v = entry
        try:
            if kind == "elt":
                self.ref.apply_galois_inplace(r, v)
            elif self.scheme == "ckks":
                self.ref.rotate_vector_inplace(r, v)
            else:
                self.ref.rotate_rows_inplace(r, v)
        except sealref.RefError as e:
            assert e.code == 2, e
            return None
        return r

    def make_set(self, entries):
        if entries[0][0] == "elt":
            return S.GaloisSet(self.ctx, self.glk, galois_elts=[v for _, v in entries])
        return S.GaloisSet(self.ctx, self.glk, steps=[v for _, v in entries])

    def check(self, what, out, x, ci, entries, follow=None):
        """item b R + r of `out` == the per-object call (and the reference) on item b with entry r; follow: applied to both afterwards"""
        R, B = len(entries), x.shape[1]
        got = out.to_numpy()
        assert out.batch() == B * R and out.size() == 2, what
        cells = 0
        for b in range(B):
            for r, entry in enumerate(entries):
                one = self.single(self.dev_ct(x[:, b:b + 1], ci), entry)
                if follow:
                    follow(one)
                assert np.array_equal(one.to_numpy()[:, 0], got[:, b * R + r]), (what, "item", b, "entry", r, entry)
                assert (out.parms_id(), out.is_ntt_form(), out.scale(), out.correction_factor()) == \
                    (one.parms_id(), one.is_ntt_form(), one.scale(), one.correction_factor()), (what, "metadata")
                if self.ref is not None and follow is None:
                    ref = self.ref_single(x[:, b], ci, entry)
                    if ref is not None:
                        assert np.array_equal(ref.data(), got[:, b * R + r]), (what, "reference, item", b, "entry", r, entry)
                        i = ref.info()
                        assert (out.is_ntt_form(), out.scale(), out.correction_factor()) == (i["is_ntt_form"], i["scale"], i["correction_factor"])
                cells += 1
        return cells


def entries_of(side, which):
    if which == "steps":
        return [("step", s) for s in worst_steps(side.n)]
    if which == "elts":
        return [("elt", e) for e in worst_elts(side)]
    if which == "one":
        return [("elt", side.elt(1))]
    raise ValueError(which)


def make_side(scheme, n, bits, **kw):
    return Side(scheme, n, bits, steps=[1, -(n // 2 - 1)], elts=[2 * n - 1], **kw)


def expected_route(side, entries):
    """restates the route rule of include/sealhip.h: the one-batch route where every key is in register order (N >= 2^13) and the set
    has more than one entry; a set of one entry is the single-key call"""
    return "batched" if two_pass_ring(side.n) and len(entries) > 1 else "looped"


# ---- parity
def case_parity(scheme, n, bits, batches=(1, 3), sets=("one", "steps", "elts"), ci=None, env=None, sub_route=None, key_pattern=None, side=None):
    """every set x every batch: each result item equals the per-object call and the reference.  sub_route: "gathered" | "permuted" |
    None - what SealHip_GaloisStats must count for a call on the one-batch route"""
    side = side or make_side(scheme, n, bits, key_pattern=key_pattern)
    ci = side.first if ci is None else ci
    with _Env(**dict(KS_ENV, **(env or {}))):
        for which in sets:
            entries = entries_of(side, which)
            gs = side.make_set(entries)
            identities = sum(1 for e in entries if e == ("step", 0))
            assert gs.info()[:2] == (len(entries), identities)
            for B in batches:
                x = side.operand(ci, B)
                c = side.dev_ct(x, ci)
                s0, g0 = S.galois_set_stats(), S.galois_stats()
                out = side.ev.apply_galois_set(c, gs)
                s1, g1 = S.galois_set_stats(), S.galois_stats()
                route = expected_route(side, entries)
                assert (s1[0] - s0[0], s1[1] - s0[1]) == ((1, 0) if route == "batched" else (0, 1)), (scheme, n, which, B, s0, s1)
                if route == "batched" and sub_route:
                    assert (g1[0] - g0[0], g1[1] - g0[1]) == ((1, 0) if sub_route == "gathered" else (0, 1)), (scheme, n, which, B, sub_route)
                side.check((scheme, n, which, B, env), out, x, ci, entries)
                assert np.array_equal(c.to_numpy(), x), "the operand is only read"
    return side


def case_chunks(scheme, n, bits, lanes):
    """B R = 15 items that are key-switched, in chunks of 2 (the last one short; edges inside a run of one key and between keys)"""
    side = make_side(scheme, n, bits)
    ci = side.first
    entries = entries_of(side, "elts")
    gs = side.make_set(entries)
    x = side.operand(ci, 3)
    with _Env(**dict(KS_ENV, SEALHIP_KS_SPLIT=1, SEALHIP_KS_CHUNK=2, SEALHIP_KS_LANES=lanes)):
        k0, s0 = S.ks_chunk_stats(), S.galois_set_stats()
        out = side.ev.apply_galois_set(side.dev_ct(x, ci), gs)
        k1, s1 = S.ks_chunk_stats(), S.galois_set_stats()
        assert (k1[0] - k0[0], k1[1] - k0[1]) == (1, 8), ("the set's key switch did not run in 8 chunks", k0, k1)
        assert (s1[0] - s0[0], s1[2] - s0[2]) == (1, 8), (s0, s1)
        side.check((scheme, n, "chunked", lanes), out, x, ci, entries)


def case_launch_count(n, bits, small):
    """the fused launches of an unchunked set call do not grow with R; the loop route issues R single-key calls"""
    side = make_side("ckks", n, bits)
    ci = side.first
    counts = {}
    with _Env(**dict(KS_ENV, SEALHIP_KS_SPLIT=1)):
        for R in (2, 8):
            entries = [("elt", [side.elt(1), 2 * n - 1][r % 2]) for r in range(R)]
            x = side.operand(ci, 1, structured=False)
            s0 = S.galois_set_stats()
            out = side.ev.apply_galois_set(side.dev_ct(x, ci), side.make_set(entries))
            s1 = S.galois_set_stats()
            assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, 0)
            counts[R] = s1[2] - s0[2]
            side.check(("launch count", R), out, x, ci, entries)
    assert counts[2] == counts[8] == 1, counts
    low = make_side("ckks", *small)
    for R in (2, 8):
        entries = [("elt", [low.elt(1), 2 * low.n - 1][r % 2]) for r in range(R)]
        x = low.operand(low.first, 1, structured=False)
        s0, g0 = S.galois_set_stats(), S.galois_stats()
        out = low.ev.apply_galois_set(low.dev_ct(x, low.first), low.make_set(entries))
        s1, g1 = S.galois_set_stats(), S.galois_stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (0, 1, 0)
        assert sum(g1) - sum(g0) == R, "the loop route: one single-key call per entry"


# ---- life cycle
def _follow(side):
    return side.ev.rescale_to_next_inplace if side.scheme == "ckks" else side.ev.mod_switch_to_next_inplace


def case_pending_tail(scheme, n, bits):
    """a set call followed by rescale_to_next (CKKS) / mod_switch_to_next (BFV) on the destination equals the per-item sequence; where
    the route defers and the set has no identity entry the division folds the pending tail (SealHip_TailStats)"""
    side = make_side(scheme, n, bits)
    ci = side.first
    scale = float(side.primes[side.K(ci) - 1]) * 2.0 ** 10 if scheme == "ckks" else 1.0
    side.scale = scale
    defers = scheme in ("ckks", "bfv") and two_pass_ring(n) and side.K(ci) >= 2
    for which in ("elts", "steps"):
        entries = entries_of(side, which)
        x = side.operand(ci, 2, structured=False)
        with _Env(**KS_ENV):
            out = side.ev.apply_galois_set(side.dev_ct(x, ci), side.make_set(entries))
            f0 = S.tail_stats()
            _follow(side)(out)
            f1 = S.tail_stats()
            direct = which == "elts"
            assert f1[0] - f0[0] == (1 if defers and direct else 0), (which, "folded tails", f0, f1)
            side.check((scheme, n, which, "+ the division that follows"), out, x, ci, entries, follow=_follow(side))


def case_pending_operand(n, bits):
    """CKKS: an operand with a pending tail (a rotation's) or a pending product (multiply into a third object) is settled first"""
    side = make_side("ckks", n, bits)
    ci = side.first
    entries = entries_of(side, "elts")
    gs = side.make_set(entries)
    x = side.operand(ci, 2, structured=False)
    with _Env(**dict(KS_ENV, SEALHIP_KS_SPLIT=1)):
        rotated = side.single(side.dev_ct(x, ci), ("step", 1))           # tail pending at the two-pass sizes
        out = side.ev.apply_galois_set(rotated, gs)
        settled = rotated.to_numpy()
        side.check("operand with a pending tail", out, settled, ci, entries)
    # a pending product makes its destination a size-3 object: refused like every operand that is not of size 2, and left as it was
    with _Env(**dict(KS_ENV, SEALHIP_LAZY_PRODUCT_MIN_WGS=0)):
        a, b, w = side.dev_ct(x, ci), side.dev_ct(x, ci), S.Ciphertext(side.ctx, batch=2)
        side.ev.multiply(a, b, w)
        _expect(S.InvalidArgument, lambda: side.ev.apply_galois_set(w, gs), "a size-3 operand")
        product = w.to_numpy()
        w2 = S.Ciphertext(side.ctx, batch=2)
        side.ev.multiply(a, b, w2)
        assert np.array_equal(product, w2.to_numpy()), "the refused operand's product is what multiply promised"


def case_refusals(scheme, n, bits):
    """destination == encrypted, a wrong destination batch, a set of another context, a foreign operand: INVALIDARG, destination untouched"""
    side = make_side(scheme, n, bits)
    other = make_side(scheme, n, bits)
    ci, lib, ev = side.first, S._native.lib(), side.ev._h
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER
    entries = entries_of(side, "elts")
    R = len(entries)
    gs, foreign_set = side.make_set(entries), other.make_set(entries_of(other, "elts"))
    x = side.operand(ci, 2)
    c = side.dev_ct(x, ci)
    dest = side.dev_ct(side.operand(ci, 2 * R), ci)
    snapshot, before = dest.to_numpy(), (dest.parms_id(), dest.size(), dest.batch(), dest.scale())

    def call(ev_h, c_h, s_h, d_h):
        return lib.Evaluator_ApplyGaloisSet(ev_h, c_h, s_h, d_h) & 0xFFFFFFFF

    for k in range(4):
        args = [ev, c._h, gs._h, dest._h]
        args[k] = None
        assert call(*args) == POINTER, ("NULL handle", k)
    assert call(ev, c._h, gs._h, c._h) == INVALID, "destination == encrypted"
    same_batch = side.dev_ct(side.operand(ci, R), ci)
    one_set = side.make_set(entries_of(side, "one"))
    assert call(ev, same_batch._h, one_set._h, same_batch._h) == INVALID, "destination == encrypted, even where the batches agree"
    for wrong in (2 * R - 1, 2 * R + 1, 2):
        assert call(ev, c._h, gs._h, S.Ciphertext(side.ctx, batch=wrong)._h) == INVALID, ("destination batch", wrong)
    assert call(ev, c._h, foreign_set._h, dest._h) == INVALID, "a set of another context"
    assert call(ev, other.dev_ct(x, ci)._h, gs._h, dest._h) == INVALID, "an operand of another context"
    three = S.Ciphertext.from_numpy(side.ctx, np.concatenate([x, x[:1]]), side.ctx.parms_id_at(ci), side.ntt, side.scale, side.cf)
    assert call(ev, three._h, gs._h, dest._h) == INVALID, "a size other than 2"
    wrong_form = S.Ciphertext.from_numpy(side.ctx, x, side.ctx.parms_id_at(ci), not side.ntt, side.scale, side.cf)
    assert call(ev, wrong_form._h, gs._h, dest._h) == INVALID, "not the scheme's native form"
    assert np.array_equal(dest.to_numpy(), snapshot) and (dest.parms_id(), dest.size(), dest.batch(), dest.scale()) == before, \
        "a failed check must leave the destination untouched"
    side.ev.apply_galois_set(c, gs, dest)
    side.check("after the refusals", dest, x, ci, entries)


def case_transparent_check(scheme, n, bits):
    """with Evaluator_SetTransparentCheck on, a result batch with a transparent item is refused; an ordinary one passes"""
    side = make_side(scheme, n, bits)
    ci = side.first
    entries = entries_of(side, "elts")
    gs = side.make_set(entries)
    x = side.operand(ci, 2, structured=False)
    side.ev.set_transparent_check(True)
    try:
        out = side.ev.apply_galois_set(side.dev_ct(x, ci), gs)
        side.check("transparent check on", out, x, ci, entries)
        z = x.copy()
        z[1] = 0   # every item is (c0, 0): so is every rotation of it, and the check over the result batch finds no non-zero word
        _expect(S.LogicError, lambda: side.ev.apply_galois_set(side.dev_ct(z, ci), gs), "a transparent result batch")
        z[1, 1] = x[1, 1]   # one ordinary item: the batch passes, as it does for Evaluator_ApplyGalois
        mixed = side.ev.apply_galois_set(side.dev_ct(z, ci), gs)
    finally:
        side.ev.set_transparent_check(False)
    side.check("one item of the batch is not transparent", mixed, z, ci, entries)


def case_destroy_after_call(scheme, n, bits):
    """a set destroyed right after the call that used it, its block taken again at once: the queued call still reads its table"""
    side = make_side(scheme, n, bits)
    ci = side.first
    x = side.operand(ci, 2, structured=False)
    c = side.dev_ct(x, ci)
    runs = []
    for trial in range(3):
        entries = entries_of(side, "elts")
        if trial == 1:
            entries = entries[::-1]
        gs = side.make_set(entries)
        runs.append((side.ev.apply_galois_set(c, gs), entries))
        gs.destroy()
        assert gs._h is None
    for out, entries in runs:
        side.check("destroyed set", out, x, ci, entries)


def case_keys_changed(scheme, n, bits):
    """a set whose keys object had a key replaced after Create is refused at call time; a new set works"""
    side = make_side(scheme, n, bits)
    ci = side.first
    entries = entries_of(side, "elts")
    gs = side.make_set(entries)
    x = side.operand(ci, 1, structured=False)
    c = side.dev_ct(x, ci)
    side.check("before the key is replaced", side.ev.apply_galois_set(c, gs), x, ci, entries)
    e = side.elt(1)
    side.glk.set_key(S.GaloisKeys.get_index(e), np.ascontiguousarray(side.key_words[2 * n - 1]))
    if side.ref is not None:
        side.ref.set_key("galois", S.GaloisKeys.get_index(e), side.key_words[2 * n - 1])
    _expect(S.InvalidArgument, lambda: side.ev.apply_galois_set(c, gs), "a key replaced after Create")
    side.check("a new set after the key was replaced", side.ev.apply_galois_set(c, side.make_set(entries)), x, ci, entries)


def case_create_errors(scheme, n, bits):
    """everything the two constructors validate, and their NULL pointers"""
    side = make_side(scheme, n, bits)
    other = make_side(scheme, n, bits)
    lib = S._native.lib()
    INVALID, POINTER = S._native.E_INVALIDARG, S._native.E_POINTER

    def create(elts, count=None, ctx=side.ctx._h, glk=side.glk._h, out=True, steps=False):
        h = C.c_void_p()
        arr = None if elts is None else ((C.c_int if steps else C.c_uint32) * max(len(elts), 1))(*elts)
        fn = lib.GaloisSet_CreateFromSteps if steps else lib.GaloisSet_Create
        hr = fn(ctx, glk, C.c_uint64(len(elts) if count is None else count), arr, C.byref(h) if out else None) & 0xFFFFFFFF
        if hr == 0:
            assert lib.GaloisSet_Destroy(h) == 0
        return hr

    e1 = side.elt(1)
    assert create([e1, 2 * n - 1, e1]) == 0 and create([1, 0, 1, -(n // 2 - 1)], steps=True) == 0, "valid sets (repeats allowed)"
    assert create([e1, 2]) == INVALID and create([0]) == INVALID, "an even element"
    assert create([e1, 2 * n + 1]) == INVALID, "an element >= 2N"
    assert create([side.elt(2)]) == INVALID and create([2], steps=True) == INVALID, "a missing key (no NAF chain in a set)"
    assert create([n], steps=True) == INVALID and create([-n], steps=True) == INVALID, "a step too large"
    assert create([], count=0) == INVALID and create([], count=0, steps=True) == INVALID, "count 0"
    assert create([e1], count=1 << 32) == INVALID, "count 2^32 (refused before the array is read)"
    assert create(None, count=1) == INVALID and create(None, count=1, steps=True) == INVALID, "NULL arrays"
    assert create([e1], glk=other.glk._h) == INVALID and create([1], glk=other.glk._h, steps=True) == INVALID, "keys of another context"
    assert create([e1], ctx=None) == POINTER and create([e1], glk=None) == POINTER and create([e1], out=False) == POINTER
    assert create([1], ctx=None, steps=True) == POINTER and create([1], glk=None, steps=True) == POINTER and create([1], out=False, steps=True) == POINTER
    assert lib.GaloisSet_Destroy(None) & 0xFFFFFFFF == POINTER and lib.GaloisSet_Info(None, None, None, None, None) & 0xFFFFFFFF == POINTER
    gs = S.GaloisSet(side.ctx, side.glk, steps=[1, 0, 1])
    assert gs.info() == (3, 1, 1, two_pass_ring(n))
    assert lib.GaloisSet_Info(gs._h, None, None, None, None) == 0, "any output may be NULL"
    _expect(S.InvalidArgument, lambda: S.GaloisSet(side.ctx, side.glk, galois_elts=[4]), "the Python constructor passes the refusal on")
    _expect(ValueError, lambda: S.GaloisSet(side.ctx, side.glk), "neither elements nor steps")
    msg = None
    try:
        S.GaloisSet(side.ctx, side.glk, steps=[2])
    except S.InvalidArgument as ex:
        msg = ex.message
    assert msg == "Galois key not present", msg


def case_capture(n, bits, R=4, seed=61):
    """GPU only.  CKKS: a set call plus dot_plain_device(group = R) recorded in a graph; the operand's words are refreshed in place
    before each replay; the replay equals the eager result and the per-object calls"""
    side = Side("ckks", n, bits, steps=[1, 2, 3])
    ci = side.first
    K = side.K(ci)
    entries = [("step", s) for s in (1, 2, 3, 1)][:R]
    gs = side.make_set(entries)
    rng = np.random.default_rng(seed)
    q = side.q(ci)
    pl = (rng.integers(0, 2 ** 63, (R, K, n), dtype=np.uint64) % q[None, :, None]).astype(np.uint64)
    buf = S.DeviceBuffer.from_numpy(pl)
    c = side.dev_ct(side.operand(ci, 1, structured=False), ci)
    rot = [S.Ciphertext(side.ctx, batch=R) for _ in range(2)]
    dot = [S.Ciphertext(side.ctx, batch=1) for _ in range(2)]
    h2d = S._native.lib().shl_memcpy_h2d
    state = {}

    def refresh():
        w = np.ascontiguousarray(side.operand(ci, 1, structured=False))
        S._native.check(h2d(C.c_void_p(c.device_ptr()[0]), w.ctypes.data_as(C.c_void_p), C.c_uint64(w.nbytes)))
        state["x"] = w

    def step(k=0):
        side.ev.apply_galois_set(c, gs, rot[k])
        side.ev.dot_plain_device(rot[k], buf, side.scale, group=R, destination=dot[k])

    refresh()
    step()
    graph = side.ev.capture(step)
    for trial in range(2):
        refresh()
        graph.launch()
        replay = (rot[0].to_numpy(), dot[0].to_numpy())
        step(1)
        assert np.array_equal(replay[0], rot[1].to_numpy()) and np.array_equal(replay[1], dot[1].to_numpy()), ("graph replay", trial)
        assert np.array_equal(c.to_numpy(), state["x"]), "the operand is only read"
    side.check("replayed set call", rot[0], state["x"], ci, entries)


def case_c5(n, bits):
    """GPU only: the C5 chain once, B = 1 and R = 3 (three keys: one draw and two rotations of it), word for word against three single calls"""
    side = Side("ckks", n, bits, steps=[1, 2, 3], cheap_keys=True)
    ci = side.first
    entries = [("step", s) for s in (1, 2, 3)]
    x = side.operand(ci, 1, structured=False)
    with _Env(**KS_ENV):
        s0 = S.galois_set_stats()
        out = side.ev.apply_galois_set(side.dev_ct(x, ci), side.make_set(entries))
        s1 = S.galois_set_stats()
        assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, 0)
        side.check("C5", out, x, ci, entries)


# ---- pipeline (the reference's keys and objects)
def case_pipeline_diagonals(n, bits, dim=4, seed=67):
    """a dense dim x dim plaintext matrix times a slot vector by diagonals: encode_device (the dim diagonals) -> apply_galois_set
    (steps 0 .. dim - 1: an identity entry and dim - 1 rotations) -> dot_plain_device(group = dim).  The words equal the reference's loop
    rotate_vector -> multiply_plain -> add_many on the same fresh ciphertext, and the result decodes to the numpy product within the
    error the reference's own loop makes on the same inputs"""
    from plain_batch_cases import _client
    side = _client("ckks", n, bits)
    ref, ev = side.ref, side.d.ev
    enc = S.CKKSEncoder(side.ctx)
    rng = np.random.default_rng(seed)
    pid, ci, slots = side.ctx.first_parms_id(), side.first, n // 2
    scale = 2.0 ** bits[-2]
    steps = list(range(dim))
    ref.keygen_galois_steps(steps[1:])
    glk = S.GaloisKeys(side.ctx)
    for s in steps[1:]:
        e = ref.galois_elt_from_step(s)
        glk.set_key(S.GaloisKeys.get_index(e), ref.key("galois", (e - 1) >> 1))
    M, v = rng.standard_normal((dim, dim)), rng.standard_normal(dim)
    tiled = np.tile(v, slots // dim)
    diags = np.stack([np.tile(np.array([M[i][(i + r) % dim] for i in range(dim)]), slots // dim) for r in steps])
    wv = enc.encode_device(S.DeviceBuffer.from_array(tiled[None, :]), 1, pid, scale)
    wd = enc.encode_device(S.DeviceBuffer.from_array(diags), dim, pid, scale)
    wd_host = wd.to_numpy((dim, side.K(ci), n))
    side.enc.set_seed(None)
    V = side.enc.encrypt_symmetric_device(wv, 1, pid, scale)
    fresh = V.save_bytes(item=0)
    gs = S.GaloisSet(side.ctx, glk, steps=steps)
    assert gs.info()[:3] == (dim, 1, dim - 1)
    rotated = ev.apply_galois_set(V, gs)
    R = ev.dot_plain_device(rotated, wd, scale, group=dim)
    assert (R.batch(), R.size(), R.scale()) == (1, 2, scale * scale)
    terms = []
    for r in steps:
        c, _ = ref.ct_load(fresh)
        ref.rotate_vector_inplace(c, r)
        assert np.array_equal(rotated.to_numpy()[:, r], c.data()), ("rotation", r)
        terms.append(ref.multiply_plain_inplace(c, ref.pt(wd_host[r], ci, scale)))
    want = ref.add_many(terms)
    assert np.array_equal(R.to_numpy()[:, 0], want.data()) and R.scale() == want.info()["scale"], "the diagonal product"
    coeffs, _ = side.dec.decrypt_batch(R)
    got = enc.decode_device(coeffs, 1, R.parms_id(), R.scale()).to_array((1, slots))[0]
    theirs = ref.ckks_decode(ref.decrypt(want), False)
    exact = np.tile(M @ v, slots // dim)
    tolerance = np.max(np.abs(theirs - exact))   # what the reference's own loop achieves on these inputs
    assert np.max(np.abs(got - exact)) <= tolerance, (np.max(np.abs(got - exact)), tolerance)
    assert tolerance < 1e-3, ("the reference's own loop is far from the product", tolerance)
