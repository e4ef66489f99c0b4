"""A rows x inner matrix of ciphertexts times an inner x cols matrix of ciphertexts (size 2 x 2, one ciphertext per entry): the
tiled kernel against the composed route the SAME build already had, on raw words through the seams:

  TR x TC nt / cached   shl_matmul_items_tile: a tile of TR x TC outputs per thread, every built tile, the operand loads with and
                        without the non-temporal hint
  dense map             shl_reduce_mapped (kind 2: Evaluator_DotItemsMapped's kernel) over the dense pair map - row i cols + j names
                        the pairs (i inner + k, k cols + j); with rows = cols = 1 its terms are Evaluator_DotItems' with group = inner

Shapes: CKKS; N = 8192 with {60, 40, 40, 60} and N = 65536 with {60, 14 x 50, 60}, each at (rows, inner, cols) = (1, 16, 1),
(4, 16, 4), (8, 16, 8), (8, 64, 8), (16, 16, 16); at (8, 16, 8) also Y stored [cols][inner] and X X^T with one buffer for both.

By bytes (P = one plane of one item = K N 8 bytes, a term = one (i, j, k)): the dense map reads 4 P per term, a TR x TC tile
2 (TR + TC) P per TR TC terms (edge tiles counted as they are); both write 3 rows cols P.  A term is four 64 x 64 multiply-accumulates
per word; the table gives the model's GB/s and the Gmac/s next to the time, so that what bounds a tile can be read off.

All routes are timed interleaved sample by sample, a sample being --inner calls between two HIP events on the NULL stream, one
warm-up round first; median [min .. max] per call.  Timing does not depend on the words: the operands are whatever the allocation
holds (the tests own correctness); every route cuts by the library's rule (the slices run are printed).

  python tools/matmul_items_rate.py [--reps 7] [--inner 10] [--out FILE] [--small] [--lib PATH] [--no-headline]"""
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

RINGS = [(8192, [60, 40, 40, 60]), (65536, [60] + [50] * 14 + [60])]
SHAPES = [(1, 16, 1), (4, 16, 4), (8, 16, 8), (8, 64, 8), (16, 16, 16)]
EXTRA = (8, 16, 8)   # also with Y transposed and as X X^T
TILES = [(1, 1), (2, 2), (2, 4)]
HINTS = [("nt", 1 << 16), ("cached", 2 << 16)]


def shape(d, n, rows, inner, cols, form, a, lines, table):
    lib, ci = S._native.lib(), d.ctx.chain_index(d.ctx.first_parms_id())
    K = len(d.ctx.coeff_modulus_at(ci))
    words = K * n
    P = words * 8
    flag, same = form == "Y transposed", form == "X X^T"
    assert not same or rows == cols
    x = S.DeviceBuffer(2 * rows * inner * words)
    y = x if same else S.DeviceBuffer(2 * inner * cols * words)
    r = S.DeviceBuffer(3 * rows * cols * words)
    first = [[i * inner + k for k in range(inner)] for i in range(rows) for j in range(cols)]
    if flag or same:   # item (k, j) at j inner + k
        second = [[j * inner + k for k in range(inner)] for i in range(rows) for j in range(cols)]
    else:
        second = [[k * cols + j for k in range(inner)] for i in range(rows) for j in range(cols)]
    dense = S.ItemMap(d.ctx, first, rows * inner, second=second, second_batch=inner * cols)
    used = C.c_uint64()

    def mapped(rp, scratch):
        S._native.check(lib.shl_reduce_mapped(d.ctx._h, C.c_uint64(ci), C.c_int(2), C.c_void_p(x.ptr), C.c_uint64(rows * inner), C.c_void_p(y.ptr),
                                              C.c_uint64(inner * cols), C.c_void_p(rp), C.c_uint64(3), dense._h, C.c_uint64(0),
                                              C.c_void_p(scratch), C.byref(used), None))
    mapped(None, None)
    scratch = S.DeviceBuffer(max(used.value * 3 * rows * cols * words, 1))

    def tiled(tile):
        S._native.check(lib.shl_matmul_items_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p(x.ptr), C.c_void_p(y.ptr), C.c_void_p(r.ptr), C.c_uint64(rows),
                                                  C.c_uint64(inner), C.c_uint64(cols), C.c_int(1 if flag or same else 0), C.c_uint64(0),
                                                  C.byref(used), C.c_uint64(tile), None))

    def many(fn):
        def run():
            for _ in range(a.inner):
                fn()
        return run

    routes = [("%d x %d %s" % (tr, tc, hint), tr << 8 | tc | bits, (tr, tc)) for tr, tc in TILES for hint, bits in HINTS]
    fns = [("dense map", many(lambda: mapped(r.ptr, scratch.ptr)))] + [(name, many(lambda t=tile: tiled(t))) for name, tile, _ in routes]
    ms = {name: [v / a.inner for v in vals] for name, vals in interleaved(fns, a.reps).items()}
    slices = {}
    mapped(r.ptr, scratch.ptr)
    slices["dense map"] = used.value
    for name, tile, _ in routes:
        tiled(tile)
        slices[name] = used.value
    S.device_synchronize()
    terms, out_bytes = rows * inner * cols, 3 * rows * cols * P
    nbytes = {"dense map": 4 * terms * P + out_bytes}
    for name, _, (tr, tc) in routes:
        # per value of the inner index a tile reads both planes of its live rows of x and of its live columns of y
        items = sum(min(tr, rows - i) + min(tc, cols - j) for i in range(0, rows, tr) for j in range(0, cols, tc))
        nbytes[name] = 2 * items * inner * P + out_bytes
    macs = 4 * terms * words
    med = {name: max(float(np.median(v)), 1e-9) for name, v in ms.items()}
    spread = {name: max(v) - min(v) for name, v in ms.items()}
    lines.append("N = %d, K = %d, %d x %d x %d (rows x inner x cols)%s; median [min .. max] of %d interleaved samples of %d calls (HIP events), ms per call"
                 % (n, K, rows, inner, cols, "" if form == "plain" else ", " + form, a.reps, a.inner))
    for name, _ in fns:
        v = ms[name]
        lines.append("  %-14s %9.4f [%9.4f .. %9.4f] ms  %7.1f GB/s by the model  %7.1f Gmac/s  slices %2d  composed / this %6.2f%s"
                     % (name, med[name], min(v), max(v), nbytes[name] / med[name] / 1e6, macs / med[name] / 1e6, slices[name],
                        med["dense map"] / med[name], "   SLOWER THAN THE COMPOSED ROUTE" if med[name] > med["dense map"] else ""))
    best = min((name for name, _, _ in routes), key=lambda k: med[k])
    if med["dense map"] - med[best] <= max(spread[best], spread["dense map"]):
        lines.append("  NO TILE BEATS THE COMPOSED ROUTE BY MORE THAN THE SPREAD OF THE SAMPLES AT THIS SHAPE (best: %s)" % best)
    lines.append("")
    print("\n".join(lines[-len(fns) - 3:]), file=sys.stderr, flush=True)   # progress
    table.append("| %d | %d | %d x %d x %d%s | %.4f | %s |" % (n, K, rows, inner, cols, "" if form == "plain" else " " + form, med["dense map"], " | ".join(
        "%.4f (%.2fx, %.0f Gmac/s)" % (med[name], med["dense map"] / med[name], macs / med[name] / 1e6) for name, _, _ in routes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, a short chain, two shapes: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    ap.add_argument("--no-headline", action="store_true", help="skip the N = 65536 ring")
    a = ap.parse_args()
    rings = [(1024, [60, 40, 60])] if a.small else [r for r in RINGS if not (a.no_headline and r[0] == 65536)]
    shapes = [(1, 16, 1), (3, 4, 5)] if a.small else SHAPES
    extra = (3, 4, 3) if a.small else EXTRA
    S.load(a.lib)
    tr, tc, flush = C.c_uint64(), C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_matmul_items_info(C.byref(tr), C.byref(tc), C.byref(flush)))
    lines = ["the library's tile: %d x %d; values of the inner index between two reductions: %d" % (tr.value, tc.value, flush.value), ""]
    names = ["%d x %d %s" % (r, c, hint) for r, c in TILES for hint, _ in HINTS]
    table = ["| N | K | rows x inner x cols | dense map ms | " + " | ".join("%s ms (composed / this, rate)" % k for k in names) + " |",
             "|---|---|---|---|" + "---|" * len(names)]
    for n, bits in rings:
        d = DeviceSide("ckks", n, coeff_modulus_create(n, bits))
        for rows, inner, cols in shapes:
            shape(d, n, rows, inner, cols, "plain", a, lines, table)
        for form in ("Y transposed", "X X^T"):
            shape(d, n, *extra, form, a, lines, table)
    text = "\n".join(lines + table) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
