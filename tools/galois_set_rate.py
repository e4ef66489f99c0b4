"""R rotations of a batch: Evaluator_ApplyGaloisSet against what the SAME build already had - R calls of Evaluator_ApplyGalois into
R destinations, eager and as one hipGraph replay.

  set          one Evaluator_ApplyGaloisSet into a destination of B R items
  loop eager   R x Evaluator_ApplyGalois of the batch of B, each into its own destination
  loop graph   the same R calls recorded once and replayed

Every route ends with its results complete: a key-switch tail that a route leaves pending is completed inside the timed region (the
destination's words are asked for), so the three routes are timed to the same point.  CKKS, distinct steps 1 .. R, every step with
its own key: the set streams R keys, as the loop does.  Keys and operands hold valid uniform words, the same for every key (timing does
not depend on the words; the tests own correctness).

Configurations: the C5 chain (65536, {60, 14 x 50, 60}) with B = 1 and R in {1, 2, 8, 32, 64} and with B = 8, R = 8; (8192,
{60, 40, 40, 60}) with R in {8, 64}.  Per configuration: the device memory held by the keys, the largest key-switch intermediate
(SealHip_KsChunkStats), the chunk plan (chunks issued per call) and which sub-route served the set call (SealHip_GaloisStats).

All routes are timed interleaved sample by sample between two HIP events on the evaluator's stream, one warm-up round first; median
[min .. max] per call.  A set call whose median is behind the better loop by more than that loop's own min .. max spread is marked.

  python tools/galois_set_rate.py [--reps 7] [--out FILE] [--small] [--lib PATH] [--no-headline] [--no-graph] [--max-r 64]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import seal_amd as S
from batch_reduce_rate import interleaved
from harness import DeviceSide
from oracle import coeff_modulus_create

C5 = (65536, [60] + [50] * 14 + [60])
MID = (8192, [60, 40, 40, 60])
CONFIGS = [(C5, 1, 1), (C5, 1, 2), (C5, 1, 8), (C5, 1, 32), (C5, 1, 64), (C5, 8, 8), (MID, 1, 8), (MID, 1, 64)]


class Ring:
    """one context with Galois keys for the steps 1 .. max_r, every key the same valid words uploaded once"""

    def __init__(self, n, bits, max_r):
        self.n, self.bits = n, bits
        self.primes = coeff_modulus_create(n, bits)
        self.d = DeviceSide("ckks", n, self.primes)
        self.L = len(self.primes)
        self.K = self.L - 1
        rng = np.random.default_rng(1)
        q = np.array(self.primes, dtype=np.uint64)[None, None, :, None]
        words = (rng.integers(0, 2 ** 63, (self.K, 2, self.L, n), dtype=np.uint64) % q).astype(np.uint64)
        staged = S.DeviceBuffer.from_numpy(words)
        self.glk = S.GaloisKeys(self.d.ctx)
        lib = S._native.lib()
        self.elts = []
        for step in range(1, max_r + 1):
            e = C.c_uint32()
            S._native.check(lib.GaloisTool_GetEltFromStep(self.d.ctx._h, C.c_int(step), C.byref(e)))
            S._native.check(lib.KSwitchKeys_SetKeyFromDevice(self.glk._h, self.d.ctx._h, C.c_uint64(S.GaloisKeys.get_index(e.value)),
                                                             C.c_uint64(self.K), C.c_void_p(staged.ptr)))
            self.elts.append(e.value)
        self.rng = rng

    def operand(self, B):
        q = np.array(self.primes[:self.K], dtype=np.uint64)[None, None, :, None]
        x = (self.rng.integers(0, 2 ** 63, (2, B, self.K, self.n), dtype=np.uint64) % q).astype(np.uint64)
        return S.Ciphertext.from_numpy(self.d.ctx, x, self.d.parms_id_for_K(self.K), True, 2.0 ** 20)


def config(ring, B, R, a, lines, table):
    d, ev = ring.d, ring.d.ev
    elts = ring.elts[:R]
    gs = S.GaloisSet(d.ctx, ring.glk, galois_elts=elts)
    c = ring.operand(B)
    dest = S.Ciphertext(d.ctx, batch=B * R)
    singles = [S.Ciphertext(d.ctx, batch=B) for _ in range(R)]

    def set_call():
        ev.apply_galois_set(c, gs, dest)
        dest.device_ptr()   # completes a pending tail

    def loop():
        for e, one in zip(elts, singles):
            ev.apply_galois(c, e, ring.glk, one)
            one.device_ptr()

    set_call()
    loop()
    S.ks_chunk_stats()
    g0, k0, s0 = S.galois_stats(), S.ks_chunk_stats(), S.galois_set_stats()
    set_call()
    g1, k1, s1 = S.galois_stats(), S.ks_chunk_stats(), S.galois_set_stats()
    sub = "operand read through the maps" if g1[0] > g0[0] else "permuted scratch"
    route = "one batch, %s, %d fused launch(es), %d chunk(s)" % (sub, s1[2] - s0[2], max(k1[1] - k0[1], 1)) if s1[0] > s0[0] else "loop over the entries"
    graph = None if a.no_graph else ev.capture(loop)
    routes = [("set", set_call), ("loop eager", loop)] + ([("loop graph", graph.launch)] if graph else [])
    ms = interleaved(routes, a.reps)
    S.device_synchronize()
    med = {k: max(float(np.median(v)), 1e-9) for k, v in ms.items()}
    best = min([k for k, _ in routes[1:]], key=lambda k: med[k])
    spread = max(ms[best]) - min(ms[best])
    behind = med["set"] - med[best] > spread
    lines.append("N = %d, K = %d, B = %d, R = %d: keys %.2f GB on the device, largest key-switch intermediate %.2f GB; set call: %s"
                 % (ring.n, ring.K, B, R, R * ring.glk.device_bytes() / len(ring.elts) / 1e9, k1[2] / 1e9, route))
    for k, _ in routes:
        v = ms[k]
        lines.append("  %-10s %9.4f [%9.4f .. %9.4f] ms  %8.4f ms per rotation  best loop / this %5.2f%s"
                     % (k, med[k], min(v), max(v), med[k] / (B * R), med[best] / med[k],
                        "   BEHIND THE BEST LOOP BY MORE THAN ITS SPREAD" if k == "set" and behind else ""))
    lines.append("")
    print("\n".join(lines[-5:]), file=sys.stderr, flush=True)   # progress
    table.append("| %d | %d | %d | %.4f | %.4f | %s | %.2f | %.4f |" % (ring.n, B, R, med["set"], med["loop eager"],
                                                                      "%.4f" % med["loop graph"] if graph else "-", med[best] / med["set"],
                                                                      med["set"] / (B * R)))
    del graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 8192 with R = 2 only: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    ap.add_argument("--no-headline", action="store_true", help="skip the N = 65536 ring")
    ap.add_argument("--no-graph", action="store_true", help="leave the replayed loop out (the emulated build does not replay graphs)")
    ap.add_argument("--max-r", type=int, default=64, help="skip configurations with more entries")
    a = ap.parse_args()
    S.load(a.lib)
    configs = [(MID, 1, 2)] if a.small else [c for c in CONFIGS if c[2] <= a.max_r and not (a.no_headline and c[0] is C5)]
    lines = ["R rotations of B ciphertexts, results complete; median [min .. max] of %d interleaved samples (HIP events), ms per call" % a.reps, ""]
    table = ["| N | B | R | set ms | loop eager ms | loop graph ms | best loop / set | set ms per rotation |", "|---|---|---|---|---|---|---|---|"]
    for shape in (C5, MID):
        mine = [c for c in configs if c[0] is shape]
        if not mine:
            continue
        ring = Ring(shape[0], shape[1], max(c[2] for c in mine))
        for _, B, R in mine:
            config(ring, B, R, a, lines, table)
        del ring
        S.release_pool()
    text = "\n".join(lines + table) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
