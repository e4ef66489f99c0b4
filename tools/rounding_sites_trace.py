"""The kernel-launch sequence of every host site that divides by a dropped prime, for the emulated build:

    HIPEMU_TRACE=1 python tools/rounding_sites_trace.py N [path/to/libsealhip_emu.so] 2> trace.txt

One fixed script per ring size N (K = 3 data primes): CKKS rescale, mod_switch_to_next for BGV and BFV, relinearize for CKKS, BGV
and BFV, one CKKS rotation, shl_rns_stage stage 5.  The operands and keys are uniform random words - no oracle is involved, the
script compares nothing itself: it exists so that the output of two builds can be diffed (profiles/rounding_sites.txt).  A
"[site] ..." line on stderr precedes each step; stdout gets a SHA-256 of each step's result words."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import seal_amd as S  # noqa: E402


def note(text):
    os.write(2, ("[site] %s\n" % text).encode())


def digest(what, array):
    print("%s %s" % (hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()[:16], what), flush=True)


def main():
    n = int(sys.argv[1])
    S.load(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "hipemu", "libsealhip_emu.so"))
    bits = [50, 40, 40, 50] if n >= 4096 else [30, 30, 30, 30]
    primes = S.CoeffModulus.Create(n, bits)
    L, K = len(primes), len(primes) - 1
    t = S.PlainModulus.Batching(n, 20 if n >= 4096 else 17)
    rng = np.random.default_rng(1)

    def words(*lead, count=K):
        return np.stack([rng.integers(0, primes[i], lead + (n,), dtype=np.uint64) for i in range(count)], axis=len(lead))

    for scheme in ("ckks", "bgv", "bfv"):
        p = S.EncryptionParameters(scheme)
        p.set_poly_modulus_degree(n)
        p.set_coeff_modulus(primes)
        if scheme != "ckks":
            p.set_plain_modulus(t)
        ctx = S.SEALContext(p, True, 0)
        ev = S.Evaluator(ctx)
        pid = ctx.parms_id_at(ctx.chain_index(ctx.key_parms_id()) - 1)
        rlk, glk = S.RelinKeys(ctx), S.GaloisKeys(ctx)
        rlk.set_key(0, words(K, 2, count=L))
        is_ntt = scheme != "bfv"
        scale = float(primes[K - 1]) * 2.0 ** 10

        def ct(size, batch=2):
            return S.Ciphertext.from_numpy(ctx, words(size, batch), pid, is_ntt, scale if scheme == "ckks" else 1.0)

        if scheme == "ckks":
            note("ckks rescale")
            c = ct(2)
            ev.rescale_to_next_inplace(c)
            digest("ckks rescale", c.to_numpy())
        else:
            note("%s mod_switch_to_next" % scheme)
            c = ct(2)
            ev.mod_switch_to_next_inplace(c)
            digest("%s mod_switch_to_next" % scheme, c.to_numpy())
        note("%s relinearize" % scheme)
        c = ct(3)
        ev.relinearize_inplace(c, rlk)
        digest("%s relinearize" % scheme, c.to_numpy())
        if scheme == "ckks":
            note("ckks rotation")
            glk.set_key(S.GaloisKeys.get_index(3), words(K, 2, count=L))
            c = ct(2)
            ev.apply_galois_inplace(c, 3, glk)
            digest("ckks rotation", c.to_numpy())
            note("stage 5")
            src, dst = S.DeviceBuffer.from_numpy(words(2)), S.DeviceBuffer(2 * (K - 1) * n)
            S.rns_stage(ctx, ctx.chain_index(pid), "divide_and_round_q_last_ntt", src, dst, 2)
            digest("stage 5", dst.to_numpy((2, K - 1, n)))
    note("done")


if __name__ == "__main__":
    main()
