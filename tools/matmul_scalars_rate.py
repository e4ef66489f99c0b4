"""A rows x inner matrix of scalar weights times an inner x cols matrix of ciphertexts (one per entry): the scalar-weights matrix
kernel in both forms and every built row tile against the routes the SAME build already had, on raw words through the seams:

  wide R=4 / 8     shl_matmul_scalars_tile: [rows inner][K] 64-bit words of weights, a tile of R output rows of one column per thread
  narrow R=4 / 8   the same with [rows inner] signed 32-bit weights (flags bit 2): half the multiplies per product
  plain 4 x 4      shl_matmul_plain_items (the library's tile) with every weight expanded to a [K][N] plaintext, where the expanded
                   plaintexts fit --plain-limit-gb
  dot_scalars      at cols = 1 only: shl_dot_scalars (the library's tile), the existing scalar kernel, whose shape this then is

Shapes: CKKS, size 2; N = 8192 with {60, 40, 40, 60} at rows in {1, 8, 64} x inner in {16, 256} and N = 65536 with {60, 14 x 50, 60} at
inner = 16, the same rows; each with cols in {1, 4, 16}.

By bytes (P = one plane of one item = K N 8 bytes): the scalar kernel reads ceil(rows / R) size inner cols P and writes size rows cols
P, the weights being rows inner K 8 (wide) or rows inner 4 (narrow) bytes; the plaintext tile reads (4 + 4) P per 16 terms and plane
(edge tiles counted as they are) and writes the same.  All do size rows inner cols K N multiply-accumulates; the table gives the
model's GB/s and the Gmac/s next to the time, so that what bounds a form can be read off: the one that stops growing with R.

All routes are timed interleaved sample by sample, a sample being --inner calls between two HIP events on the NULL stream, one
warm-up round first; median [min .. max] per call.  Timing does not depend on the words: the ciphertexts and plaintexts are whatever
the allocation holds, the weights are written before the first call (the tests own correctness); every route cuts by the library's
rule (the slices run are printed).

  python tools/matmul_scalars_rate.py [--reps 7] [--inner 10] [--out FILE] [--small] [--lib PATH] [--no-headline]"""
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
COLS = (1, 4, 16)
TILES = (4, 8)
SIZE = 2
NARROW = 4


def shape(d, n, rows, inner, cols, a, lines, table):
    lib, ci = S._native.lib(), d.ctx.chain_index(d.ctx.first_parms_id())
    K = len(d.ctx.coeff_modulus_at(ci))
    words = K * n
    P = words * 8
    rng = np.random.default_rng(rows * 1000 + cols)
    x, r = S.DeviceBuffer(SIZE * inner * cols * words), S.DeviceBuffer(SIZE * rows * cols * words)
    wide = S.DeviceBuffer.from_numpy(rng.integers(0, 1 << 39, rows * inner * K, dtype=np.uint64))
    narrow = S.DeviceBuffer.from_int32(rng.integers(-2 ** 31, 2 ** 31, rows * inner).astype(np.int32))
    plain = S.DeviceBuffer(rows * inner * words) if rows * inner * P <= a.plain_limit_gb * 1e9 else None
    used = C.c_uint64()

    def scalars(R, form):
        S._native.check(lib.shl_matmul_scalars_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p((narrow if form else wide).ptr), C.c_void_p(x.ptr),
                                                    C.c_void_p(r.ptr), C.c_uint64(SIZE), C.c_uint64(rows), C.c_uint64(inner), C.c_uint64(cols),
                                                    C.c_uint64(form), C.c_uint64(0), C.byref(used), C.c_uint64(R), None))

    def expanded():
        S._native.check(lib.shl_matmul_plain_items_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p(plain.ptr), C.c_void_p(x.ptr), C.c_void_p(r.ptr),
                                                        C.c_uint64(SIZE), C.c_uint64(rows), C.c_uint64(inner), C.c_uint64(cols), C.c_uint64(0),
                                                        C.c_uint64(0), C.byref(used), C.c_uint64(0), None))

    def dot():
        S._native.check(lib.shl_dot_scalars_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p(x.ptr), C.c_void_p(wide.ptr), C.c_void_p(r.ptr),
                                                 C.c_uint64(SIZE), C.c_uint64(rows), C.c_uint64(inner), C.c_uint64(0), C.byref(used),
                                                 C.c_uint64(0), None))

    def many(fn):
        def run():
            for _ in range(a.inner):
                fn()
        return run

    once = [("%s R=%d" % (name, R), lambda R=R, form=form: scalars(R, form)) for name, form in (("wide", 0), ("narrow", NARROW)) for R in TILES]
    if plain is not None:
        once.append(("plain 4 x 4", expanded))
    if cols == 1:
        once.append(("dot_scalars", dot))
    ms = {name: [v / a.inner for v in vals] for name, vals in interleaved([(name, many(fn)) for name, fn in once], a.reps).items()}
    slices = {}
    for name, fn in once:
        fn()
        slices[name] = used.value
    S.device_synchronize()
    out_bytes = SIZE * rows * cols * P
    nbytes = {}
    for name, _ in once:
        if name.startswith("plain"):
            items = sum(min(4, rows - i) + min(4, cols - j) for i in range(0, rows, 4) for j in range(0, cols, 4))
            nbytes[name] = SIZE * items * inner * P + out_bytes
        else:
            R = int(name.split("=")[1]) if "=" in name else 4
            weights = rows * inner * (4 if name.startswith("narrow") else 8 * K)
            nbytes[name] = -(-rows // R) * SIZE * inner * cols * P + weights + out_bytes
    macs = SIZE * rows * inner * cols * words
    med = {name: max(float(np.median(v)), 1e-9) for name, v in ms.items()}
    lines.append("N = %d, K = %d, size %d, %d x %d x %d (rows x inner x cols); median [min .. max] of %d interleaved samples of %d calls (HIP events), ms per call"
                 % (n, K, SIZE, rows, inner, cols, a.reps, a.inner))
    if plain is None:
        lines.append("  (the expanded plaintexts would be %.1f GB: that route is not run)" % (rows * inner * P / 1e9))
    for name, _ in once:
        v = ms[name]
        lines.append("  %-12s %9.4f [%9.4f .. %9.4f] ms  %7.1f GB/s by the model  %7.1f Gmac/s  slices %2d  wide R=4 / this %6.2f"
                     % (name, med[name], min(v), max(v), nbytes[name] / med[name] / 1e6, macs / med[name] / 1e6, slices[name], med["wide R=4"] / med[name]))
    if cols == 1:
        best = min(("wide R=%d" % R for R in TILES), key=lambda k: med[k])
        gap, spread = med[best] - med["dot_scalars"], max(max(ms[k]) - min(ms[k]) for k in (best, "dot_scalars"))
        if gap > spread:
            lines.append("  THE WIDE FORM IS SLOWER THAN dot_scalars HERE BY MORE THAN THE SPREAD OF THE SAMPLES (best: %s, %.4f ms)" % (best, gap))
    lines.append("")
    print("\n".join(lines[-len(once) - 3:]), file=sys.stderr, flush=True)   # progress
    cell = lambda name: "%.4f (%.0f)" % (med[name], macs / med[name] / 1e6) if name in med else "-"
    table.append("| %d | %d | %d x %d x %d | %s |" % (n, K, rows, inner, cols, " | ".join(cell(k) for k in NAMES)))


NAMES = ["wide R=4", "wide R=8", "narrow R=4", "narrow R=8", "plain 4 x 4", "dot_scalars"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, a short chain, two shapes: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    ap.add_argument("--no-headline", action="store_true", help="skip the N = 65536 ring")
    ap.add_argument("--plain-limit-gb", type=float, default=40.0, help="largest expanded plaintext matrix the plaintext route is run with")
    a = ap.parse_args()
    S.load(a.lib)
    v = [C.c_uint64() for _ in range(4)]
    S._native.check(S._native.lib().shl_matmul_scalars_info(*[C.byref(x) for x in v]))
    lines = ["the library's row tile: wide %d, narrow %d; values of the inner index between two reductions: wide %d, narrow %d"
             % tuple(x.value for x in v), ""]
    table = ["| N | K | rows x inner x cols | " + " | ".join("%s ms (Gmac/s)" % k for k in NAMES) + " |", "|---|---|---|" + "---|" * len(NAMES)]
    if a.small:
        d = DeviceSide("ckks", 1024, coeff_modulus_create(1024, [60, 40, 60]))
        for rows, inner, cols in ((1, 16, 1), (9, 5, 3)):
            shape(d, 1024, rows, inner, cols, a, lines, table)
    else:
        for n, bits, inners in SHAPES:
            if a.no_headline and n == 65536:
                continue
            d = DeviceSide("ckks", n, coeff_modulus_create(n, bits))
            for inner in inners:
                for rows in ROWS:
                    for cols in COLS:
                        shape(d, n, rows, inner, cols, a, lines, table)
    text = "\n".join(lines + table) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
