"""Pass 1 of the rounding tails in both orders (ntt2_kernels.hip: src_resident()): target-resident (ntt2_fwd_p1 / ntt2_tail2_p1, one
workgroup per target component) and source-resident (ntt2_src_p1t, the source tile in registers and the targets in the loop).

SEALHIP_TAIL_P1_ORDER is read once per process, so every setting runs in a child process of its own: `python tail_order_cases.py LIB
CASE` runs one case against the library LIB, compares every result word for word with the oracle (the real reference when
oracle/_ref is built, tests/oracle.py) and prints one JSON line with a digest per result; the parent (test_tail_order.py on the
emulator, test_gpu_tail_order.py on the device) compares the digests of the settings with each other.

What a case runs: relinearize + rescale and rotate + rescale (the folded tail, two sources; SealHip_TailStats says that it ran),
plain rescale (one source, epilogue 1), and with SEALHIP_KS_EAGER_TAIL=1 the key switch's own tail (one source, epilogue 2 / 3)
followed by the plain rescale; BFV: multiply + relinearize + mod_switch_to_next and a plain mod_switch_to_next.
"""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# name -> (scheme, N, bit sizes of the chain incl. the special prime, batch)
CASES = {
    # K = 2: after the division ONE target, a class run of one (forced source-resident: the loop of one)
    "ckks_k2_8192": ("ckks", 8192, [50, 40, 60], 3),
    # mixed chains: 60-bit and double-precision targets, q_last below and above 2^52, odd batches
    "ckks_mixed_8192": ("ckks", 8192, [60, 40, 50, 45, 60], 3),
    "ckks_mixed_last60_8192": ("ckks", 8192, [50, 40, 58, 60], 2),
    "ckks_mixed_32768": ("ckks", 32768, [60, 50, 40, 50, 60], 1),
    "ckks_mixed_65536": ("ckks", 65536, [60, 50, 50, 60], 1),
    # every target on the integer back end (all three modulus classes)
    "ckks_int_8192": ("ckks", 8192, [60, 58, 55, 52, 60], 3),
    "ckks_int_65536": ("ckks", 65536, [60, 59, 51, 60], 1),
    "bfv_8192": ("bfv", 8192, [50, 55, 56, 56], 2),
    "bfv_32768": ("bfv", 32768, [55, 55, 56], 1),
    # device only: 16 tiles x 2 x batch items against the threshold of 512 workgroups - batch 15 below it, 16 on it
    # (two double-precision targets after the division: a class run that has a tile to share)
    "ckks_threshold_below_65536": ("ckks", 65536, [60, 50, 50, 50, 60], 15),
    "ckks_threshold_at_65536": ("ckks", 65536, [60, 50, 50, 50, 60], 16),
    # emulator only (SEALHIP_TAIL_P1_MIN_WGS=8, a development switch): 2 tiles x 2 x batch items - batch 1 below, batch 2 on it
    "ckks_threshold_below_8192": ("ckks", 8192, [60, 40, 50, 45, 60], 1),
    "ckks_threshold_at_8192": ("ckks", 8192, [60, 40, 50, 45, 60], 2),
}


def run_case(name, check_items=None):
    """-> {stage: sha256 of the result words}; raises when a word differs from the oracle or the folded pass did not run"""
    import numpy as np
    import seal_amd as S
    from harness import DeviceSide
    from oracle import Oracle, coeff_modulus_create, plain_modulus_batching, rand_ct
    from parity_cases import _eq

    scheme, n, bits, batch = CASES[name]
    primes = coeff_modulus_create(n, bits)
    K = len(primes) - 1
    t = plain_modulus_batching(n, 20) if scheme == "bfv" else 0
    eager = bool(os.environ.get("SEALHIP_KS_EAGER_TAIL"))
    probe = Oracle(scheme, n, primes, t)
    elt = probe.galois_elt_from_step(1)
    o = Oracle(scheme, n, primes, t, galois_elts=[elt])
    d = DeviceSide(scheme, n, primes, t)
    d.upload_keys(o)
    rng = np.random.default_rng(97)
    # large batches: a few distinct items tiled (the oracle runs on the host), every item of the batch compared
    distinct = batch if check_items is None else min(batch, check_items)
    xs0 = [rand_ct(rng, primes, K, n) for _ in range(distinct)]
    ys0 = [rand_ct(rng, primes, K, n) for _ in range(distinct)]
    xs = [xs0[b % distinct] for b in range(batch)]
    ys = [ys0[b % distinct] for b in range(batch)]
    digests = {}

    def same(ct, expected, what):
        got = d.out(ct)
        h = hashlib.sha256()
        for b in range(batch):
            _eq(got[b], expected[b % distinct], "%s: %s, item %d" % (name, what, b))
            h.update(np.ascontiguousarray(got[b]).tobytes())
        digests[what] = h.hexdigest()

    def stats():
        return S.tail_stats()

    if scheme == "ckks":
        sc = float(primes[K - 1]) * 2.0 ** 10
        f0, p0, _ = stats()
        cz, cw = d.ct(xs, scale=2.0 ** 10), d.ct(ys, scale=2.0 ** 10)
        d.ev.multiply_inplace(cz, cw)
        d.ev.relinearize_inplace(cz, d.rlk)
        cz.set_scale(sc)
        d.ev.rescale_to_next_inplace(cz)
        f1, p1, _ = stats()
        assert (f1 - f0, p1 - p0) == ((0, 0) if eager else (1, 0)), "relinearize + rescale: folded %d, plain %d" % (f1 - f0, p1 - p0)
        same(cz, [o.rescale(o.relinearize(o.multiply(x, y))) for x, y in zip(xs0, ys0)], "relinearize + rescale")
        cr = d.ct(xs, scale=sc)
        d.ev.rotate_vector_inplace(cr, 1, d.glk)
        d.ev.rescale_to_next_inplace(cr)
        f2, p2, _ = stats()
        assert (f2 - f1, p2 - p1) == ((0, 0) if eager else (1, 0)), "rotate + rescale: folded %d, plain %d" % (f2 - f1, p2 - p1)
        same(cr, [o.rescale(o.apply_galois(x, elt)) for x in xs0], "rotate + rescale")
        cp = d.ct(xs, scale=sc)
        d.ev.rescale_to_next_inplace(cp)
        assert stats()[:2] == (f2, p2), "a plain rescale has no tail to fold"
        same(cp, [o.rescale(x) for x in xs0], "plain rescale")
        # the key switch's tail on its own (a reader between the key switch and the rescale completes it)
        ck = d.ct(xs, scale=sc)
        d.ev.rotate_vector_inplace(ck, 1, d.glk)
        same(ck, [o.apply_galois(x, elt) for x in xs0], "rotate, tail on its own")
        assert stats()[1] - p2 == (0 if eager else 1)
    else:
        f0, p0, _ = stats()
        cz, cw = d.ct(xs), d.ct(ys)
        d.ev.multiply_inplace(cz, cw)
        d.ev.relinearize_inplace(cz, d.rlk)
        d.ev.mod_switch_to_next_inplace(cz)
        f1, p1, _ = stats()
        assert (f1 - f0, p1 - p0) == ((0, 0) if eager else (1, 0)), "relinearize + mod_switch: folded %d, plain %d" % (f1 - f0, p1 - p0)
        same(cz, [o.mod_switch_to_next(o.relinearize(o.multiply(x, y))) for x, y in zip(xs0, ys0)], "relinearize + mod_switch_to_next")
        cp = d.ct(xs)
        d.ev.mod_switch_to_next_inplace(cp)
        same(cp, [o.mod_switch_to_next(x) for x in xs0], "plain mod_switch_to_next")
        cr = d.ct(xs)
        d.ev.rotate_rows_inplace(cr, 1, d.glk)
        same(cr, [o.apply_galois(x, elt) for x in xs0], "rotate_rows, tail on its own")
    return digests


def run_in_child(lib, name, env, check_items=None, timeout=1500):
    """one case in a fresh process with `env` added to the environment -> (digests, stderr)"""
    e = dict(os.environ)
    for k in ("SEALHIP_TAIL_P1_ORDER", "SEALHIP_KS_EAGER_TAIL", "SEALHIP_TAIL_P1_MIN_WGS", "SEALHIP_TAIL_P1_TRACE"):
        e.pop(k, None)
    e.update(env)
    cmd = [sys.executable, os.path.abspath(__file__), lib, name] + ([str(check_items)] if check_items else [])
    out = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, "%s with %r: exit %d\n%s\n%s" % (name, env, out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    return json.loads(lines[-1]), out.stderr


def both_orders(lib, name, extra_env=None, check_items=None, auto=True):
    """the case with the order forced either way and (auto) left to the library: every result equal to the oracle's (in the child)
    and to each other's (here)"""
    results = {}
    for order in ("0", "1", None) if auto else ("0", "1"):
        env = dict(extra_env or {})
        if order is not None:
            env["SEALHIP_TAIL_P1_ORDER"] = order
        results[order], _ = run_in_child(lib, name, env, check_items)
    assert results["0"] and all(r == results["0"] for r in results.values()), "%s: the orders disagree: %r" % (name, results)
    return results["0"]


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    import seal_amd
    if os.path.basename(sys.argv[1]).startswith("libsealhip_emu"):
        os.environ["SEALHIP_COMM_NO_RCCL"] = "1"
    seal_amd.load(sys.argv[1])
    print(json.dumps(run_case(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else None)))
