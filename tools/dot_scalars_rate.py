"""A dense rows x B matrix of scalar plaintexts times a batch of B ciphertexts: the scalar-weights kernel against the composed route
the SAME build already had, on raw words through the seams:

  scalars R=2 / 4 / 8   shl_dot_scalars_tile: [rows][B][K] words of weights, a tile of R output rows per thread
  dense map             shl_reduce_mapped (kind 1: Evaluator_DotPlainMapped's kernel) over the dense ItemMap - row o names the items
                        0 .. B - 1, term (o, b) names plaintext o B + b - with the scalars expanded to [rows B][K][N] plaintexts

Shapes: CKKS, size 2; N = 8192 with {60, 40, 40, 60} at rows in {1, 8, 64} x B in {16, 256}; N = 65536 with {60, 14 x 50, 60} at
B = 16 (at B = 256 and 64 rows the expanded plaintexts of the composed route are 129 GB: it does not fit), the same rows.

By bytes (P = one plane of the batch = B K N 8 bytes): the scalar kernel reads ceil(rows / R) size P and writes size rows 8 K N; the
dense map reads (size + 1) rows P and writes the same.  Both do size rows B K N multiply-accumulates of 64 x 64 bits; the table gives
the model's GB/s and the Gmac/s next to the time, so that what bounds the kernel can be read off: the one that stops growing with R.

All routes are timed interleaved sample by sample, a sample being --inner calls between two HIP events on the NULL stream, one
warm-up round first; median [min .. max] per call.  Timing does not depend on the words: the plaintexts and scalars are whatever the
allocation holds (the tests own correctness); every route cuts by the library's rule (the slices run are printed).

  python tools/dot_scalars_rate.py [--reps 7] [--inner 10] [--out FILE] [--small] [--lib PATH] [--no-headline]"""
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

SHAPES = [(8192, [60, 40, 40, 60], (16, 256)), (65536, [60] + [50] * 14 + [60], (16,))]
ROWS = (1, 8, 64)
TILES = (2, 4, 8)


def shape(d, n, rows, batch, a, lines, table):
    size = 2
    lib, ci = S._native.lib(), d.ctx.chain_index(d.ctx.first_parms_id())
    K = len(d.ctx.coeff_modulus_at(ci))
    words = K * n
    P = batch * words * 8
    x, r = S.DeviceBuffer(size * batch * words), S.DeviceBuffer(size * rows * words)
    scalars, plain = S.DeviceBuffer(rows * batch * K), S.DeviceBuffer(rows * batch * words)
    dense = S.ItemMap(d.ctx, [list(range(batch))] * rows, batch, second=[list(range(o * batch, (o + 1) * batch)) for o in range(rows)],
                      second_batch=rows * batch)
    used = C.c_uint64()

    def mapped(rp, scratch):
        S._native.check(lib.shl_reduce_mapped(d.ctx._h, C.c_uint64(ci), C.c_int(1), C.c_void_p(x.ptr), C.c_uint64(batch), C.c_void_p(plain.ptr),
                                              C.c_uint64(rows * batch), C.c_void_p(rp), C.c_uint64(size), dense._h, C.c_uint64(0),
                                              C.c_void_p(scratch), C.byref(used), None))
    mapped(None, None)
    scratch = S.DeviceBuffer(max(used.value * size * rows * words, 1))

    def tiled(R):
        S._native.check(lib.shl_dot_scalars_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p(x.ptr), C.c_void_p(scalars.ptr), C.c_void_p(r.ptr),
                                                 C.c_uint64(size), C.c_uint64(rows), C.c_uint64(batch), C.c_uint64(0), C.byref(used),
                                                 C.c_uint64(R), None))

    def many(fn):
        def run():
            for _ in range(a.inner):
                fn()
        return run

    fns = [("dense map", many(lambda: mapped(r.ptr, scratch.ptr)))] + [("scalars R=%d" % R, many(lambda R=R: tiled(R))) for R in TILES]
    ms = {name: [v / a.inner for v in vals] for name, vals in interleaved(fns, a.reps).items()}
    slices = {}
    mapped(r.ptr, scratch.ptr)
    slices["dense map"] = used.value
    for R in TILES:
        tiled(R)
        slices["scalars R=%d" % R] = used.value
    S.device_synchronize()
    out_bytes = size * rows * words * 8
    nbytes = {"dense map": (size + 1) * rows * P + out_bytes}
    for R in TILES:
        nbytes["scalars R=%d" % R] = -(-rows // R) * size * P + out_bytes
    macs = size * rows * batch * words
    med = {name: max(float(np.median(v)), 1e-9) for name, v in ms.items()}
    lines.append("N = %d, K = %d, size %d, %d rows x B = %d; median [min .. max] of %d interleaved samples of %d calls (HIP events), ms per call"
                 % (n, K, size, rows, batch, a.reps, a.inner))
    for name, _ in fns:
        v = ms[name]
        lines.append("  %-12s %9.4f [%9.4f .. %9.4f] ms  %7.1f GB/s by the model  %7.1f Gmac/s  slices %d  composed / this %6.2f%s"
                     % (name, med[name], min(v), max(v), nbytes[name] / med[name] / 1e6, macs / med[name] / 1e6, slices[name],
                        med["dense map"] / med[name], "   SLOWER THAN THE COMPOSED ROUTE" if med[name] > med["dense map"] else ""))
    lines.append("")
    print(lines[-len(fns) - 2], file=sys.stderr, flush=True)   # progress
    table.append("| %d | %d | %d x %d | %.4f | %s |" % (n, K, rows, batch, med["dense map"], " | ".join(
        "%.4f (%.2fx, %.0f Gmac/s)" % (med["scalars R=%d" % R], med["dense map"] / med["scalars R=%d" % R], macs / med["scalars R=%d" % R] / 1e6)
        for R in TILES)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, a short chain, B = 16: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    ap.add_argument("--no-headline", action="store_true", help="skip the N = 65536 shape")
    a = ap.parse_args()
    shapes = [(1024, [60, 40, 60], (16,))] if a.small else [s for s in SHAPES if not (a.no_headline and s[0] == 65536)]
    S.load(a.lib)
    row_tile, flush = C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_dot_scalars_info(C.byref(row_tile), C.byref(flush)))
    lines = ["the library's row tile: R = %d; items between two reductions: %d" % (row_tile.value, flush.value), ""]
    table = ["| N | K | rows x B | dense map ms | " + " | ".join("R = %d ms (composed / this, rate)" % R for R in TILES) + " |", "|---|---|---|---|---|---|---|"]
    for n, bits, batches in shapes:
        d = DeviceSide("ckks", n, coeff_modulus_create(n, bits))
        for batch in batches:
            for rows in ROWS:
                shape(d, n, rows, batch, a, lines, table)
    text = "\n".join(lines + table) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
