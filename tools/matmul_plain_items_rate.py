"""A rows x inner matrix of NTT-form plaintexts times an inner x cols matrix of ciphertexts (one per entry): the tiled kernel
against the composed route the SAME build already had, on raw words through the seams:

  TP x TC nt / cached   shl_matmul_plain_items_tile: a tile of TP x TC outputs of one plane per thread, every built tile, the operand
                        loads with and without the non-temporal hint
  dense map             shl_reduce_mapped (kind 1: Evaluator_DotPlainMapped's kernel) over the dense map - row i cols + j names
                        ciphertext item k cols + j and plaintext i inner + k; with rows = cols = 1 its terms are
                        Evaluator_DotPlainDevice's with group = inner

Shapes: CKKS, size 2; N = 8192 with {60, 40, 40, 60} and N = 65536 with {60, 14 x 50, 60}, each at (rows, inner, cols) =
(1, 16, 1), (4, 16, 4), (8, 16, 8), (8, 64, 8), (16, 16, 16); at N = 65536, (8, 16, 8) also with each flag (the ciphertexts stored
[cols][inner], the result stored [cols][rows], both).

By bytes (P = one plane of one item = K N 8 bytes, a term = one (i, j, k)): the dense map reads (size + 1) P per term, a TP x TC
tile (TP + TC) P per TP TC terms and plane (edge tiles counted as they are); both write size rows cols P.  A term is `size` 64 x 64
multiply-accumulates per word; the table gives the model's GB/s and the Gmac/s next to the time, so that what bounds a tile can be
read off.

All routes are timed interleaved sample by sample, a sample being --inner calls between two HIP events on the NULL stream, one
warm-up round first; median [min .. max] per call.  The operands are random words (one item's worth, copied to every item); the
tests own correctness; every route cuts by the library's rule (the slices run are printed).

  python tools/matmul_plain_items_rate.py [--reps 7] [--inner 10] [--out FILE] [--small] [--lib PATH] [--no-headline]"""
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
EXTRA = (8, 16, 8)   # at the headline ring also with each flag
FORMS = [("X stored [cols][inner]", 1), ("result stored [cols][rows]", 2), ("both", 3)]
SIZE = 2
TILES = [(1, 1), (2, 4), (4, 4), (4, 8)]
HINTS = [("nt", 1 << 16), ("cached", 2 << 16)]


def filled(items, item_words, rng):
    """a buffer of `items` items that all hold the same random words"""
    buf = S.DeviceBuffer(items * item_words)
    w = rng.integers(0, 1 << 59, item_words, dtype=np.uint64)
    for i in range(items):
        S._native.check(S._native.lib().shl_memcpy_h2d(C.c_void_p(buf.ptr + 8 * i * item_words), w.ctypes.data_as(C.c_void_p), C.c_uint64(w.nbytes)))
    return buf


def shape(d, n, rows, inner, cols, form, flags, a, lines, table):
    lib, ci = S._native.lib(), d.ctx.chain_index(d.ctx.first_parms_id())
    K = len(d.ctx.coeff_modulus_at(ci))
    words = K * n
    P = words * 8
    rng = np.random.default_rng(rows * 1000 + cols)
    pl = filled(rows * inner, words, rng)
    x = filled(SIZE * inner * cols, words, rng)
    r = S.DeviceBuffer(SIZE * rows * cols * words)
    out = [[(j, i) for j in range(cols) for i in range(rows)], [(i, j) for i in range(rows) for j in range(cols)]][0 if flags & 2 else 1]
    if flags & 1:   # item (k, j) at j inner + k
        first = [[j * inner + k for k in range(inner)] for i, j in out]
    else:
        first = [[k * cols + j for k in range(inner)] for i, j in out]
    second = [[i * inner + k for k in range(inner)] for i, j in out]
    dense = S.ItemMap(d.ctx, first, inner * cols, second=second, second_batch=rows * inner)
    used = C.c_uint64()

    def mapped(rp, scratch):
        S._native.check(lib.shl_reduce_mapped(d.ctx._h, C.c_uint64(ci), C.c_int(1), C.c_void_p(x.ptr), C.c_uint64(inner * cols), C.c_void_p(pl.ptr),
                                              C.c_uint64(rows * inner), C.c_void_p(rp), C.c_uint64(SIZE), dense._h, C.c_uint64(0),
                                              C.c_void_p(scratch), C.byref(used), None))
    mapped(None, None)
    scratch = S.DeviceBuffer(max(used.value * SIZE * rows * cols * words, 1))

    def tiled(tile):
        S._native.check(lib.shl_matmul_plain_items_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p(pl.ptr), C.c_void_p(x.ptr), C.c_void_p(r.ptr),
                                                        C.c_uint64(SIZE), C.c_uint64(rows), C.c_uint64(inner), C.c_uint64(cols), C.c_uint64(flags),
                                                        C.c_uint64(0), C.byref(used), C.c_uint64(tile), None))

    def many(fn):
        def run():
            for _ in range(a.inner):
                fn()
        return run

    routes = [("%d x %d %s" % (tp, tc, hint), tp << 8 | tc | bits, (tp, tc)) for tp, tc in TILES for hint, bits in HINTS]
    fns = [("dense map", many(lambda: mapped(r.ptr, scratch.ptr)))] + [(name, many(lambda t=tile: tiled(t))) for name, tile, _ in routes]
    ms = {name: [v / a.inner for v in vals] for name, vals in interleaved(fns, a.reps).items()}
    slices = {}
    mapped(r.ptr, scratch.ptr)
    slices["dense map"] = used.value
    for name, tile, _ in routes:
        tiled(tile)
        slices[name] = used.value
    S.device_synchronize()
    terms, out_bytes = rows * inner * cols, SIZE * rows * cols * P
    nbytes = {"dense map": (SIZE + 1) * terms * P + out_bytes}
    for name, _, (tp, tc) in routes:
        # per value of the inner index and plane a tile reads its live rows of plaintexts and its live columns of ciphertexts
        items = sum(min(tp, rows - i) + min(tc, cols - j) for i in range(0, rows, tp) for j in range(0, cols, tc))
        nbytes[name] = SIZE * items * inner * P + out_bytes
    macs = SIZE * terms * words
    med = {name: max(float(np.median(v)), 1e-9) for name, v in ms.items()}
    spread = {name: max(v) - min(v) for name, v in ms.items()}
    lines.append("N = %d, K = %d, size %d, %d x %d x %d (rows x inner x cols)%s; median [min .. max] of %d interleaved samples of %d calls (HIP events), ms per call"
                 % (n, K, SIZE, rows, inner, cols, "" if not flags else ", " + form, a.reps, a.inner))
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
    table.append("| %d | %d | %d x %d x %d%s | %.4f | %s |" % (n, K, rows, inner, cols, "" if not flags else " " + form, med["dense map"], " | ".join(
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
    tp, tc, flush = C.c_uint64(), C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_matmul_plain_items_info(C.byref(tp), C.byref(tc), C.byref(flush)))
    lines = ["the library's tile: %d x %d; values of the inner index between two reductions: %d" % (tp.value, tc.value, flush.value), ""]
    names = ["%d x %d %s" % (r, c, hint) for r, c in TILES for hint, _ in HINTS]
    table = ["| N | K | rows x inner x cols | dense map ms | " + " | ".join("%s ms (composed / this, rate)" % k for k in names) + " |",
             "|---|---|---|---|" + "---|" * len(names)]
    for n, bits in rings:
        d = DeviceSide("ckks", n, coeff_modulus_create(n, bits))
        for rows, inner, cols in shapes:
            shape(d, n, rows, inner, cols, "", 0, a, lines, table)
        if a.small or n == 65536:
            for form, flags in FORMS:
                shape(d, n, *extra, form, flags, a, lines, table)
    text = "\n".join(lines + table) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
