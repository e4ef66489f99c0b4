"""A sparse matrix of scalar weights times a batch over an item map: the scalar term of the mapped kernel against the route the SAME
build already had, on raw words through the seams:

  scalars wide / narrow  shl_dot_scalars_mapped: [count][K] words or [count] 32-bit integers of weights
  plain map              shl_reduce_mapped (kind 1: Evaluator_DotPlainMapped's kernel) over the same map with the weights expanded
                         to [count][K][N] plaintexts
  tile (dense map only)  shl_dot_scalars_tile at the library's row tile: it reads the operand once per tile of rows

Shapes: CKKS, size 2, at N = 8192 with {60, 40, 40, 60} and at N = 65536 with {60, 14 x 50, 60}:
  pruned     64 rows x 8 random terms over 64 items, one weight per term
  pooling    2 x 2 average pooling over 8 channels of 8 x 8: 128 rows of 4 terms, one weight
  depthwise  3 x 3, pad 1, over 8 channels of 8 x 8: 512 rows of 4, 6 or 9 terms, 72 weights
  dense      16 rows x 64 items, 1024 weights

By bytes (W = K N 8, the bytes of one plane of one item): the scalar term reads size terms W and writes size rows W; the plain map
reads (size + 1) terms W and writes the same - 1.5 x the reads at size 2.  Both do size terms K N multiply-accumulates; the table gives
the model's GB/s and the Gmac/s next to the time, so that what bounds the kernel can be read off.

All routes are timed interleaved sample by sample, a sample being --inner calls between two HIP events on the NULL stream, one
warm-up round first; median [min .. max] per call.  Timing does not depend on the words: operands and weights are whatever the
allocation holds (the tests own correctness); every route cuts by the library's rule (the slices run are printed).  A scalar route
whose median is behind the plain map's by more than the plain map's own min .. max spread is marked.

  python tools/dot_scalars_mapped_rate.py [--reps 7] [--inner 10] [--out FILE] [--small] [--lib PATH] [--no-headline]"""
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


def pruned(rng, rows=64, terms=8, items=64):
    first = [[int(v) for v in rng.integers(0, items, terms)] for _ in range(rows)]
    return first, [list(range(o * terms, (o + 1) * terms)) for o in range(rows)], items, rows * terms


def pooling(channels=8, height=8, width=8, k=2):
    first = [[(c * height + y + dy) * width + x + dx for dy in range(k) for dx in range(k)]
             for c in range(channels) for y in range(0, height, k) for x in range(0, width, k)]
    return first, [[0] * len(r) for r in first], channels * height * width, 1


def depthwise(channels=8, height=8, width=8, k=3, pad=1):
    first, second = [], []
    for c in range(channels):
        for y in range(height):
            for x in range(width):
                taps = [(dy, dx) for dy in range(k) for dx in range(k) if 0 <= y + dy - pad < height and 0 <= x + dx - pad < width]
                first.append([(c * height + y + dy - pad) * width + x + dx - pad for dy, dx in taps])
                second.append([(c * k + dy) * k + dx for dy, dx in taps])
    return first, second, channels * height * width, channels * k * k


def dense(rows=16, items=64):
    return [list(range(items))] * rows, [list(range(o * items, (o + 1) * items)) for o in range(rows)], items, rows * items


def shape(d, n, name, lists, a, lines, table):
    size = 2
    first, second, items, count = lists
    rows, terms = len(first), sum(map(len, first))
    lib, ci = S._native.lib(), d.ctx.chain_index(d.ctx.first_parms_id())
    K = len(d.ctx.coeff_modulus_at(ci))
    words = K * n
    W = words * 8
    x, r = S.DeviceBuffer(size * items * words), S.DeviceBuffer(size * rows * words)
    wide, narrow, plain = S.DeviceBuffer(count * K), S.DeviceBuffer(max(-(-count // 2), 1)), S.DeviceBuffer(count * words)
    m = S.ItemMap(d.ctx, first, items, second=second, second_batch=count)
    used = C.c_uint64()

    def mapped(rp, scratch):
        S._native.check(lib.shl_reduce_mapped(d.ctx._h, C.c_uint64(ci), C.c_int(1), C.c_void_p(x.ptr), C.c_uint64(items), C.c_void_p(plain.ptr),
                                              C.c_uint64(count), C.c_void_p(rp), C.c_uint64(size), m._h, C.c_uint64(0), C.c_void_p(scratch),
                                              C.byref(used), None))

    def scalars(form, rp, scratch):
        S._native.check(lib.shl_dot_scalars_mapped(d.ctx._h, C.c_uint64(ci), C.c_void_p((narrow if form else wide).ptr), C.c_uint64(count),
                                                   C.c_int(form), C.c_void_p(x.ptr), C.c_uint64(items), C.c_void_p(rp), C.c_uint64(size), m._h,
                                                   C.c_uint64(0), C.c_void_p(scratch), C.byref(used), None))

    def tiled():
        S._native.check(lib.shl_dot_scalars_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p(x.ptr), C.c_void_p(wide.ptr), C.c_void_p(r.ptr),
                                                 C.c_uint64(size), C.c_uint64(rows), C.c_uint64(items), C.c_uint64(0), C.byref(used),
                                                 C.c_uint64(0), None))
    most = 1
    for query in (lambda: mapped(None, None), lambda: scalars(0, None, None), lambda: scalars(1, None, None)):
        query()
        most = max(most, used.value)
    scratch = S.DeviceBuffer(most * size * rows * words)

    def many(fn):
        def run():
            for _ in range(a.inner):
                fn()
        return run

    calls = [("plain map", lambda: mapped(r.ptr, scratch.ptr)), ("scalars wide", lambda: scalars(0, r.ptr, scratch.ptr)),
             ("scalars narrow", lambda: scalars(1, r.ptr, scratch.ptr))] + ([("tile", tiled)] if name == "dense" else [])
    ms = {k: [v / a.inner for v in vals] for k, vals in interleaved([(k, many(fn)) for k, fn in calls], a.reps).items()}
    slices = {}
    for k, fn in calls:
        fn()
        slices[k] = used.value
    S.device_synchronize()
    out_bytes = size * rows * W
    nbytes = {"plain map": (size + 1) * terms * W + out_bytes, "scalars wide": size * terms * W + out_bytes,
              "scalars narrow": size * terms * W + out_bytes, "tile": -(-rows // 4) * size * items * W + out_bytes}
    macs = size * terms * words
    med = {k: max(float(np.median(v)), 1e-9) for k, v in ms.items()}
    spread = max(ms["plain map"]) - min(ms["plain map"])
    lines.append("%s: N = %d, K = %d, size %d, %d rows, %d terms, %d items, %d weights; weights %.3f MB wide, %.3f MB narrow, %.1f MB expanded; "
                 "median [min .. max] of %d interleaved samples of %d calls (HIP events), ms per call"
                 % (name, n, K, size, rows, terms, items, count, count * K * 8 / 1e6, count * 4 / 1e6, count * W / 1e6, a.reps, a.inner))
    for k, _ in calls:
        v = ms[k]
        late = k.startswith("scalars") and med[k] - med["plain map"] > spread
        lines.append("  %-14s %9.4f [%9.4f .. %9.4f] ms  %7.1f GB/s by the model  %7.1f Gmac/s  slices %d  plain map / this %6.2f%s"
                     % (k, med[k], min(v), max(v), nbytes[k] / med[k] / 1e6, macs / med[k] / 1e6, slices[k], med["plain map"] / med[k],
                        "   BEHIND THE PLAIN MAP BY MORE THAN ITS SPREAD" if late else ""))
    lines.append("")
    print("\n".join(lines[-len(calls) - 2:]), file=sys.stderr, flush=True)   # progress
    table.append("| %s | %d | %d | %d x %.1f | %.4f | %s | %s |" % (name, n, K, rows, terms / rows, med["plain map"], " | ".join(
        "%.4f (%.2fx, %.0f GB/s, %.0f Gmac/s)" % (med[k], med["plain map"] / med[k], nbytes[k] / med[k] / 1e6, macs / med[k] / 1e6)
        for k in ("scalars wide", "scalars narrow")), "%.4f (%.2fx)" % (med["tile"], med["plain map"] / med["tile"]) if "tile" in med else "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, a short chain: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    ap.add_argument("--no-headline", action="store_true", help="skip the N = 65536 ring")
    a = ap.parse_args()
    rings = [(1024, [60, 40, 60])] if a.small else [s for s in RINGS if not (a.no_headline and s[0] == 65536)]
    S.load(a.lib)
    flush, narrow_flush = C.c_uint64(), C.c_uint64()
    S._native.check(S._native.lib().shl_dot_scalars_mapped_info(C.byref(flush), C.byref(narrow_flush)))
    lines = ["terms between two reductions: wide %d, narrow %d; by bytes the plain map reads 1.5 x what the scalar term reads at size 2"
             % (flush.value, narrow_flush.value), ""]
    table = ["| shape | N | K | rows x mean terms | plain map ms | wide ms (plain map / this, model GB/s, rate) | narrow ms (...) | tile ms |",
             "|---|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    shapes = [("pruned", pruned(rng)), ("pooling", pooling()), ("depthwise", depthwise()), ("dense", dense())]
    for n, bits in rings:
        d = DeviceSide("ckks", n, coeff_modulus_create(n, bits))
        for name, lists in shapes:
            shape(d, n, name, lists, a, lines, table)
    text = "\n".join(lines + table) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
