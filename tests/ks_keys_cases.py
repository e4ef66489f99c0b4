"""The key switch with structured switching keys, every digit-group count and every route.

Every other case takes its keys from the reference's KeyGenerator (or uniform words in the port oracle), so a key word at 0, 1,
floor(q/2), floor(q/2)+1 or q-1 - the ends and the middle of the ranges that key_layout_kernel folds into balanced doubles (primes
below 2^50) or stores next to floor(w 2^64 / q) (51 to 60 bits), and that ks2_kernel multiplies into the raised digits with the lazy
accumulators of field.h - has probability about 2^-50.  Here both keys are parity_cases.extreme_key words, set on the oracle and on
the device, and the same key switch runs with SEALHIP_KS_SPLIT unset and at 1, 2, 3, 5 and 8 digit groups (counts that do not divide K,
2 or 3 at K >= 4, counts above 4, a count above K), chunked, from a deferred product, with the eager tail and digit-parallel.

What this does and does not show: the words at the edges of the key and digit ranges are right on every route.  The digits pass
through a transform before they meet the key, so no input here drives every lane of an accumulator to its bound; the magnitude
bounds of field.h are argued there, not proven here.

SEALHIP_KS_EAGER_TAIL is read once per process, and on the emulator (built with SEALHIP_CHECK_BOUNDS) a bound violation aborts, so
every case runs in a child process of its own: `python ks_keys_cases.py LIB CASE MODE [PATTERNS]` runs one case in one mode against
the library LIB, compares every result word for word (and scale, level, correction factor) with the oracle (the real reference
when oracle/_ref is built, tests/oracle.py) and prints one JSON line.  The parents (test_ks_keys.py on the emulator,
test_gpu_ks_keys.py on the device) start one child at a time; the emulator's parent also reads the traced group counts
(SEALHIP_KS_TRACE, development builds) from the child's stderr.
"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# name -> (scheme, N, bit sizes of the chain incl. the special prime)
CASES = {
    # unfused path: keyswitch_mac_kernel, the 128-bit Field<false>::Acc, barrett128
    "mac_4096": ("ckks", 4096, [50, 59, 57, 50, 60]),
    # ks1t / ks2 with both arithmetic classes as digit and as target; K = 4: ragged groups at 3
    "fused_8192": ("ckks", 8192, [50, 59, 57, 50, 60]),
    # one-launch transform sizes, K = 3
    "fused_16384": ("ckks", 16384, [59, 50, 57, 60]),
    "fused_32768": ("ckks", 32768, [50, 59, 50, 60]),
    # lean fix placement and kLeanEntry: a 60-bit digit into 49- and 50-bit targets
    "lean_65536": ("ckks", 65536, [60, 50, 49, 57, 50, 60]),
    # K = 17: the double-precision fix at terms 7 and 14, the tight integer fix (2^58 <= q < 2^60, every 3 terms) five times, the
    # roomy one (q < 2^58, every 15 terms) once; 8 groups -> 3, 2, 2, ...
    "sched_8192": ("ckks", 8192, [50] * 8 + [59, 57] * 4 + [50, 60]),
    # K = 9: the lean placement across one acc_fix; 8 groups at K = 9
    "sched_65536": ("ckks", 65536, [60] + [50] * 8 + [60]),
    # the target read in place, the folded mod_switch tail
    "bfv_8192": ("bfv", 8192, [50, 55, 59, 60]),
    # bgv_correct_and_combine
    "bgv_8192": ("bgv", 8192, [50, 55, 59, 60]),
}
T_BITS = 20
SPLITS = (None, 1, 2, 3, 5, 8)  # SEALHIP_KS_SPLIT unset / forced
# the reference rejects a transparent result (logic_error): a flat key on a flat ciphertext often gives one; these pairs it does
REJECTED = (("qm1", ("qm1", "one")), ("half", ("half", "half1")))
# case -> the key patterns of REJECTED that the reference must refuse there (at K = 17 it accepts the second pair: agreement either way)
REJECTION_CASES = {"fused_8192": ("qm1", "half"), "sched_8192": ("qm1",)}
# keys that are the constant polynomial 1 or -1 (every word 1 or q - 1 in transformed form): a rotation's second polynomial is then
# small enough for the division that follows to round it to zero whatever the item, which the reference refuses as transparent
UNIT_KEYS = ("qm1", "one")
ENV_KEYS = ("SEALHIP_KS_SPLIT", "SEALHIP_KS_CHUNK", "SEALHIP_KS_LANES", "SEALHIP_KS_EAGER_TAIL", "SEALHIP_KS_TRACE", "SEALHIP_KS_NO_FOLD",
            "SEALHIP_LAZY_PRODUCT", "SEALHIP_LAZY_PRODUCT_MIN_WGS", "SEALHIP_KS_SCRATCH_CAP_MIB")


def auto_split(name):
    """what the launcher's rule gives at batch 3 for the shapes above: min(4, K)"""
    return min(4, len(CASES[name][2]) - 1)


def _note(text):
    """a line on stderr between the library's trace lines (unbuffered, as the library's own)"""
    os.write(2, ("[case] %s\n" % text).encode())


class _Side:
    """oracle and device for one case; the three items; the expected results per key pattern"""

    def __init__(self, name):
        import numpy as np
        from harness import DeviceSide
        from oracle import Oracle, coeff_modulus_create, plain_modulus_batching, rand_ct
        from parity_cases import extreme_slab
        self.name = name
        self.scheme, self.n, bits = CASES[name]
        self.primes = coeff_modulus_create(self.n, bits)
        self.K = len(self.primes) - 1
        self.t = plain_modulus_batching(self.n, T_BITS) if self.scheme != "ckks" else 0
        probe = Oracle(self.scheme, self.n, self.primes, self.t)
        self.elt = probe.galois_elt_from_step(1)
        self.o = Oracle(self.scheme, self.n, self.primes, self.t, galois_elts=[self.elt])
        self.d = DeviceSide(self.scheme, self.n, self.primes, self.t)
        self.is_ntt = self.scheme != "bfv"
        self.eager = bool(os.environ.get("SEALHIP_KS_EAGER_TAIL"))
        # CKKS: the scale the rescale that follows divides down to 2^10
        self.scale = float(self.primes[self.K - 1]) * 2.0 ** 10 if self.scheme == "ckks" else 1.0
        rng = np.random.default_rng(113)
        dp = self.primes[:self.K]

        def item(p0, p1, p2, seed):
            return np.stack([extreme_slab(dp, self.n, p, seed=seed + i) for i, p in enumerate((p0, p1, p2))])

        # size-3 items for relinearize; their first two polynomials are the size-2 items for the rotation.  (A second polynomial of
        # all ones is the constant 1: with any flat key the reference refuses the division's result as transparent, so the first
        # item's is mix4 like its first, from another seed)
        self.items = [item("mix4", "mix4", "qm1", 41), item("alt", "mix4", "half1", 47), rand_ct(rng, self.primes, self.K, self.n, size=3)]
        self.extra = [rand_ct(rng, self.primes, self.K, self.n, size=3) for _ in range(2)]  # the chunked route's batch of 5
        self.flat = lambda p0, p1: np.stack([extreme_slab(dp, self.n, p0, seed=53), extreme_slab(dp, self.n, p1, seed=59)])
        self.cells = 0

    # ---- keys
    def set_keys(self, pattern, galois=True):
        from parity_cases import extreme_key
        self.o.set_key("relin", 0, extreme_key(self.primes, self.K, self.n, pattern, seed=3))
        if galois:
            assert pattern != "zero", "a zero Galois key makes every rotation transparent"
            self.o.set_key("galois", self.elt, extreme_key(self.primes, self.K, self.n, pattern, seed=5))
        self.d.upload_keys(self.o)

    # ---- the oracle: key switch, then the division that follows -> ((words, info), (words, info)); info None in the port oracle
    def expect(self, x, op, pattern):
        import numpy as np
        import sealref
        o = self.o
        if o.kind == "reference":
            a = o._ct(x, self.scale, 1)
            if op == "relin":
                o.ref.relinearize_inplace(a)
            else:
                o.ref.apply_galois_inplace(a, self.elt)
            first = (a.data(), a.info())
            try:
                self._ref_follow(a)
            except sealref.RefError as e:
                if not (e.code == 2 and op == "rot" and pattern in UNIT_KEYS):
                    raise
                # The reference refuses, so it gives no words to compare with.  What is expected instead is partly the test's own
                # reasoning and not the reference's output: the key is the constant 1 or -1, so the second polynomial of the key
                # switch is round(+-sum_j t_j / P) with |coefficients| <= K, and the division by q_last rounds that to zero
                # whatever the item - the second polynomial expected from the device is all zero.  The premise is checked here on
                # the reference's own key-switch result; the refusal itself says the same (every word of it is zero).  The first
                # polynomial's expected words are the reference's: its division of (c0, a uniform polynomial), which it accepts
                # (the division treats each polynomial on its own).
                c1 = first[0][1] if self.scheme == "bfv" else o.ntt(0, first[0][1], "inv")
                q = np.array(self.primes[:self.K], dtype=np.uint64)[:, None]
                assert int(np.minimum(c1, q - c1).max()) <= self.K, "%s: key %s: the rotation's second polynomial is not small" % (self.name, pattern)
                a = o._ct(np.stack([first[0][0], self.items[2][0]]), self.scale, 1)
                self._ref_follow(a)
                words = a.data()
                words[1] = 0
                return first, (words, a.info(), True)
            return first, (a.data(), a.info(), False)
        assert self.scheme != "bgv", "BGV parity needs the real reference (oracle/_ref)"
        r = o.relinearize(x) if op == "relin" else o.apply_galois(x, self.elt)
        return (r, None), (o.rescale(r) if self.scheme == "ckks" else o.mod_switch_to_next(r), None, False)

    def _ref_follow(self, a):
        if self.scheme == "ckks":
            self.o.ref.rescale_to_next_inplace(a)
        else:
            self.o.ref.mod_switch_to_next_inplace(a)

    # ---- the device
    def ct(self, slabs):
        return self.d.ct(slabs, scale=self.scale, is_ntt=self.is_ntt)

    def switch(self, c, op):
        if op == "relin":
            self.d.ev.relinearize_inplace(c, self.d.rlk)
        elif self.scheme == "ckks":
            self.d.ev.rotate_vector_inplace(c, 1, self.d.glk)
        else:
            self.d.ev.rotate_rows_inplace(c, 1, self.d.glk)

    def follow(self, c):
        if self.scheme == "ckks":
            self.d.ev.rescale_to_next_inplace(c)
        else:
            self.d.ev.mod_switch_to_next_inplace(c)

    def defers(self):
        # mirrors Evaluator::ks_route (evaluator_keyswitch.cpp: r.defer) - keep in step with it; ntt2_supports is harness.two_pass_ring
        from harness import two_pass_ring
        return self.scheme in ("ckks", "bfv") and two_pass_ring(self.n) and self.K >= 2 and not self.eager

    def same(self, c, expected, what):
        """every item of the device ciphertext c == the oracle's (words, info)"""
        from parity_cases import _eq
        got = self.d.out(c)
        assert len(got) == len(expected), what
        for b, (words, info) in enumerate(e[:2] for e in expected):
            _eq(got[b], words, "%s: %s, item %d" % (self.name, what, b))
            assert c.coeff_modulus_size() == words.shape[1], "%s: %s: level" % (self.name, what)
            if info is not None:
                mine = (c.size(), c.coeff_modulus_size(), c.is_ntt_form(), c.scale(), c.correction_factor(),
                        c.parms_id() == self.d.ctx.parms_id_at(info["chain_index"]))
                theirs = (info["size"], info["coeff_modulus_size"], info["is_ntt_form"], info["scale"], info["correction_factor"], True)
                assert mine == theirs, "%s: %s, item %d: size, level, form, scale, correction factor %r, the oracle's %r" % (
                    self.name, what, b, mine, theirs)
            self.cells += 1
        return got

    def run_pair(self, slabs, op, expected, what, alone=True):
        """key switch + the division that follows in one go (the folded tail where the route defers), then (alone) the key switch read
        on its own (its tail completed by the read) -> the words of both, per item"""
        import seal_amd as S
        f0, p0, _ = S.tail_stats()
        c = self.ct(slabs)
        self.switch(c, op)
        self.follow(c)
        f1, p1, _ = S.tail_stats()
        want = (1, 0) if self.defers() else (0, 0)
        assert (f1 - f0, p1 - p0) == want, "%s: %s: folded %d, plain %d, expected %r" % (self.name, what, f1 - f0, p1 - p0, want)
        after = self.same(c, [e[1] for e in expected], what + " + the division that follows")
        if not alone:
            return [], after
        c = self.ct(slabs)
        self.switch(c, op)
        return self.same(c, [e[0] for e in expected], what + " on its own"), after

    def refused(self, slabs, op, what):
        """where the reference refuses the division's result as transparent, so does the device when it is asked to check"""
        import seal_amd as S
        _note(what + " refused")
        self.d.ev.set_transparent_check(True)
        try:
            c = self.ct(slabs)
            self.switch(c, op)
            try:
                self.follow(c)
                raise AssertionError("%s: %s: the device accepts a result that the reference refuses as transparent" % (self.name, what))
            except S.LogicError:
                self.cells += 1
        finally:
            self.d.ev.set_transparent_check(False)


def _splits_env(split):
    from parity_cases import _Env
    return _Env(SEALHIP_KS_SPLIT=split)


def mode_splits(side, patterns, only=None):
    """every key pattern x the three items x every group count: relinearize and a rotation, each followed by rescale_to_next (CKKS) or
    mod_switch_to_next (BFV, BGV); a count above K once per case (equal to the K-group run).  only = "relin" | "rot": that half (mode
    `splits:relin` / `splits:rot`, for the sizes at which the emulator needs minutes for both)"""
    from parity_cases import _eq
    K = side.K
    size3, size2 = side.items, [it[:2] for it in side.items]
    clamp_pattern = "mix4"  # once per case: the parents give every case one child whose patterns include it
    for pattern in patterns:
        galois = pattern != "zero"
        side.set_keys(pattern, galois)
        ops = [("relin", size3)] + ([("rot", size2)] if galois else [])
        ops = [o for o in ops if only in (None, o[0])]
        expected = {op: [side.expect(x, op, pattern) for x in slabs] for op, slabs in ops}
        for split in SPLITS:
            if split is not None and split > K:
                continue
            _note("pattern %s split %s" % (pattern, "auto" if split is None else split))
            with _splits_env(split):
                for op, slabs in ops:
                    # (the key switch on its own: once per pattern, at the launcher's own count)
                    side.run_pair(slabs, op, expected[op], "key %s, %s, groups %s" % (pattern, op, split or "auto"), alone=split is None)
        for op, slabs in ops:
            if any(e[1][2] for e in expected[op]):
                side.refused(slabs, op, "key %s, %s" % (pattern, op))
        if pattern == clamp_pattern and K < 8:
            over = [s for s in SPLITS if s is not None and s > K][0]
            runs = {}
            for split in (over, K):
                _note("pattern %s split %d clamp" % (pattern, split))
                with _splits_env(split):
                    runs[split] = [side.run_pair(slabs, op, expected[op], "key %s, %s, groups %d (K = %d)" % (pattern, op, split, K), alone=False)
                                   for op, slabs in ops]
            for a, b in zip(runs[over], runs[K]):
                for x, y in zip(a[0] + a[1], b[0] + b[1]):
                    _eq(x, y, "%s: %d groups asked at K = %d == the %d-group run" % (side.name, over, K, K))
    if side.name in REJECTION_CASES:
        mode_rejections(side)


def mode_rejections(side):
    """a rotation whose result is transparent is refused by the device (transparent check on) as by the reference; where the
    reference accepts (REJECTION_CASES says where it must not), so does the device, with the reference's words"""
    import seal_amd as S
    import sealref
    from parity_cases import _eq
    _note("rejections")
    side.d.ev.set_transparent_check(True)
    try:
        for pattern, (p0, p1) in REJECTED:
            side.set_keys(pattern)
            x = side.flat(p0, p1)
            what = "%s: key %s on (%s, %s)" % (side.name, pattern, p0, p1)
            refuses, words = True, None
            if side.o.kind == "reference":
                a = side.o._ct(x, side.scale, 1)
                try:
                    side.o.ref.apply_galois_inplace(a, side.elt)
                    refuses, words = False, a.data()
                except sealref.RefError as e:
                    assert e.code == 2, "%s: the reference raises %s" % (what, e)
                assert refuses or pattern not in REJECTION_CASES[side.name], what + ": the reference accepts"
            c = side.ct([x])
            try:
                side.switch(c, "rot")
                assert not refuses, what + ": the device accepts a result that the reference refuses as transparent"
                _eq(side.d.out(c)[0], words, what)
            except S.LogicError:
                assert refuses, what + ": the device refuses a result that the reference accepts"
            side.cells += 1
    finally:
        side.d.ev.set_transparent_check(False)


def mode_chunked(side, patterns):
    """batch 5 cut into chunks of 2 on 2 lanes (ragged last chunk): relinearize + the division that follows, and a rotation"""
    import seal_amd as S
    from parity_cases import _Env
    size3 = side.items + side.extra
    size2 = [it[:2] for it in size3]
    batch, chunk = len(size3), 2
    nchunks = (batch + chunk - 1) // chunk
    for pattern in patterns:
        side.set_keys(pattern)
        _note("pattern %s chunked" % pattern)
        c0, k0, _ = S.ks_chunk_stats()
        with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_KS_CHUNK=chunk, SEALHIP_KS_LANES=2):
            for op, slabs in (("relin", size3), ("rot", size2)):
                side.run_pair(slabs, op, [side.expect(x, op, pattern) for x in slabs], "key %s, %s, chunked" % (pattern, op))
        c1, k1, _ = S.ks_chunk_stats()
        # four key switches (two per run_pair), each in ceil(5 / 2) chunks
        assert (c1 - c0, k1 - k0) == (4, 4 * nchunks), ("the key switch did not run in chunks", c1 - c0, k1 - k0, nchunks)


def mode_lazy(side, patterns):
    """multiply(x, y, w) then relinearize_inplace(w): the product formed inside the key switch (CKKS; SealHip_ProductStats)"""
    import seal_amd as S
    from parity_cases import _Env, _eq
    assert side.scheme == "ckks"
    o, d = side.o, side.d
    xs = [it[:2] for it in side.items]
    ys = [xs[1], xs[2], xs[0]]
    defers = side.defers()
    for pattern in patterns:
        side.set_keys(pattern)
        _note("pattern %s deferred product" % pattern)
        relin = [o.relinearize(o.multiply(x, y)) for x, y in zip(xs, ys)]
        resc = [o.rescale(r) for r in relin]
        with _Env(SEALHIP_KS_SPLIT=1, SEALHIP_LAZY_PRODUCT_MIN_WGS=0, SEALHIP_LAZY_PRODUCT=None):
            for follow in (True, False):
                f0, m0, _ = S.product_stats()
                cx, cy, w = d.ct(xs, scale=2.0 ** 10), d.ct(ys, scale=2.0 ** 10), S.Ciphertext(d.ctx, batch=len(xs))
                d.ev.multiply(cx, cy, w)
                d.ev.relinearize_inplace(w, d.rlk)
                f1, m1, _ = S.product_stats()
                assert (f1 - f0, m1 - m0) == ((1, 0) if defers else (0, 0)), "the fused relinearisation did not run where it should: %r" % (
                    (f1 - f0, m1 - m0),)
                if follow:
                    w.set_scale(side.scale)
                    d.ev.rescale_to_next_inplace(w)
                got = d.out(w)
                for b in range(len(xs)):
                    _eq(got[b], (resc if follow else relin)[b], "%s: key %s, deferred product + relinearize%s, item %d" % (
                        side.name, pattern, " + rescale" if follow else "", b))
                    side.cells += 1
                assert w.coeff_modulus_size() == side.K - (1 if follow else 0) and w.scale() == (2.0 ** 10 if follow else 2.0 ** 20)


def mode_dp(name, patterns, parts_list):
    """digit-parallel key switching over `parts` virtual ranks (parity_cases.case_digit_parallel, which builds its own two sides) with
    structured keys: counts that leave ranks without digits, and the *_finish entry points at up to 8 partial sums -> runs done"""
    from oracle import coeff_modulus_create, plain_modulus_batching
    from parity_cases import case_digit_parallel
    scheme, n, bits = CASES[name]
    primes = coeff_modulus_create(n, bits)
    t = plain_modulus_batching(n, T_BITS) if scheme != "ckks" else 0
    runs = 0
    for pattern in patterns:
        for parts in parts_list:
            _note("pattern %s digit-parallel %d" % (pattern, parts))
            case_digit_parallel(scheme, n, primes, t, parts=parts, batch=2, key_pattern=pattern)
            runs += 1
    return runs


def run_case(name, mode, patterns):
    t0 = time.time()
    if mode.startswith("dp"):
        cells = mode_dp(name, patterns, [int(p) for p in mode[2:].split("+")])
    else:
        side = _Side(name)
        if mode.startswith("splits:"):
            mode_splits(side, patterns, only=mode[7:])
        else:
            {"splits": mode_splits, "chunked": mode_chunked, "lazy": mode_lazy}[mode](side, patterns)
        cells = side.cells
    return {"case": name, "mode": mode, "patterns": list(patterns), "cells": cells, "seconds": round(time.time() - t0, 2)}


class ChildDied(Exception):
    """the child ended by a signal, an abort, at its time limit or after a device fault: nothing more may be started on the same device"""


# a fault that the runtime reports as an error (the child then ends with a Python exception and exit status 1)
DEVICE_FAULTS = ("illegal memory access", "memory access fault", "hsa_status_error", "unspecified launch failure", "hardware exception")


def run_in_child(lib, name, mode, patterns, env=None, timeout=600):
    """one case in a fresh process -> (result, stderr); AssertionError carrying the child's output when it fails, ChildDied when it was
    killed (signal, abort, time limit) or reported a device fault"""
    e = dict(os.environ)
    for k in ENV_KEYS:
        e.pop(k, None)
    e.update(env or {})
    cmd = [sys.executable, os.path.abspath(__file__), lib, name, mode, ",".join(patterns)]
    what = "%s %s %s with %r" % (name, mode, ",".join(patterns), env or {})
    try:
        out = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as ex:
        tail = ex.stderr[-3000:] if isinstance(ex.stderr, str) else (ex.stderr or b"")[-3000:].decode(errors="replace")
        raise ChildDied("%s: no result after %d s\n%s" % (what, timeout, tail))
    if out.returncode < 0 or out.returncode in (134, 137, 139):
        raise ChildDied("%s: exit %d\n%s\n%s" % (what, out.returncode, out.stdout[-2000:], out.stderr[-3000:]))
    if out.returncode != 0 and any(m in out.stderr.lower() for m in DEVICE_FAULTS):
        raise ChildDied("%s: exit %d after a device fault\n%s\n%s" % (what, out.returncode, out.stdout[-2000:], out.stderr[-3000:]))
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, "%s: exit %d\n%s\n%s" % (what, out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    return json.loads(lines[-1]), out.stderr


def traced_splits(stderr):
    """the child's stderr -> [(note, [group counts the library traced after it])]"""
    out = []
    for ln in stderr.splitlines():
        if ln.startswith("[case] "):
            out.append((ln[7:], []))
        elif ln.startswith("[ks] split ") and out:
            out[-1][1].append(int(ln.split()[2]))
    return out


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    import seal_amd
    if os.path.basename(sys.argv[1]).startswith("libsealhip_emu"):
        os.environ["SEALHIP_COMM_NO_RCCL"] = "1"
    seal_amd.load(sys.argv[1])
    print(json.dumps(run_case(sys.argv[2], sys.argv[3], sys.argv[4].split(","))))
