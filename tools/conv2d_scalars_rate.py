"""A 2-D convolution of scalar weights over a grid of ciphertexts, one per (channel, pixel): the convolution kernel in both weight
forms and with both hint choices against the route the SAME build already had, on raw words through the seams:

  conv wide / narrow                shl_conv2d_scalars_tile with the library's row tile and hint (0): what the evaluator runs
  conv wide / narrow, nt / cached   the same with operand loads with (hint 1) and without (hint 2) the non-temporal hint
  gather                            shl_reduce_mapped, kind 0, over the one-term rows of the im2col map: the gathered batch of
                                    C kh kw x OH OW items (pad 0 only: a gather cannot make a zero item)
  matmul wide / narrow              shl_matmul_scalars_tile on the gathered batch, OC x C kh kw x OH OW: the CONTROL - the same
                                    multiplies with no reuse between neighbouring outputs to exploit
  two calls                         gather + matmul, the sum of the two medians: the route without the convolution

Shapes: CKKS, size 2, at N = 65536 with {60, 14 x 50, 60} and N = 8192 with {60, 40, 40, 60}: C = 8, 8 x 8, 3 x 3, stride 1, pad 0
with OC = 8 and 16; the same with pad 1 and OC = 8 (no gathered route exists); C = 1, 28 x 28, 5 x 5, stride 2, pad 0 with OC = 5.

All do size OC (live taps) K N multiply-accumulates; the table gives Tmac/s next to the time and the device memory of the operands
of each route (input + result, plus the gathered batch).  The acceptance line compares the convolution with the two calls and
with the control, against the control's own spread in the same process.

All routes are timed interleaved sample by sample, a sample being --inner calls between two HIP events on the NULL stream, one
warm-up round first; median [min .. max] per call.  Timing does not depend on the words: the ciphertexts are whatever the
allocation holds, the weights are written before the first call (the tests own correctness); every route cuts by the library's
rule (the slices run are printed).

  python tools/conv2d_scalars_rate.py [--reps 7] [--inner 3] [--out FILE] [--small] [--lib PATH] [--no-headline] [--only INDEX]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import seal_amd as S
from seal_amd.api import Conv2dShape
from batch_reduce_rate import interleaved
from harness import DeviceSide
from oracle import coeff_modulus_create

RINGS = [(65536, [60] + [50] * 14 + [60]), (8192, [60, 40, 40, 60])]
# (C, H, W, OC, kh, kw, sh, sw, ph, pw)
SHAPES = [(8, 8, 8, 8, 3, 3, 1, 1, 0, 0), (8, 8, 8, 16, 3, 3, 1, 1, 0, 0), (8, 8, 8, 8, 3, 3, 1, 1, 1, 1), (1, 28, 28, 5, 5, 5, 2, 2, 0, 0)]
SIZE = 2
NARROW = 4


def live_taps(s):
    """taps inside the image, summed over the output positions of one channel pair"""
    oh, ow = s.out_size()
    ys = sum(1 for y in range(oh) for dy in range(s.kernel_h) if 0 <= y * s.stride_h + dy - s.pad_h < s.height)
    xs = sum(1 for x in range(ow) for dx in range(s.kernel_w) if 0 <= x * s.stride_w + dx - s.pad_w < s.width)
    return ys * xs


def im2col(d, s):
    """row t * cols + pos of the gathered batch = the input item of term t at output position pos (pad 0: every tap is live)"""
    oh, ow = s.out_size()
    rows = []
    for c in range(s.in_channels):
        for dy in range(s.kernel_h):
            for dx in range(s.kernel_w):
                for y in range(oh):
                    for x in range(ow):
                        rows.append([(c * s.height + y * s.stride_h + dy) * s.width + x * s.stride_w + dx])
    return S.ItemMap(d.ctx, rows, s.in_channels * s.height * s.width)


def shape(d, n, s, a, lines, table):
    lib, ci = S._native.lib(), d.ctx.chain_index(d.ctx.first_parms_id())
    K = len(d.ctx.coeff_modulus_at(ci))
    words = K * n
    P = words * 8
    oh, ow = s.out_size()
    oc, inner, cols, items = s.out_channels, s.in_channels * s.kernel_h * s.kernel_w, oh * ow, s.in_channels * s.height * s.width
    padded = bool(s.pad_h or s.pad_w)
    rng = np.random.default_rng(oc * 1000 + cols)
    x, r = S.DeviceBuffer(SIZE * items * words), S.DeviceBuffer(SIZE * oc * cols * words)
    wide = S.DeviceBuffer.from_numpy(rng.integers(0, 1 << 39, oc * inner * K, dtype=np.uint64))
    narrow = S.DeviceBuffer.from_int32(rng.integers(-2 ** 31, 2 ** 31, oc * inner).astype(np.int32))
    used = C.c_uint64()

    def conv(form, hint):
        S._native.check(lib.shl_conv2d_scalars_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p((narrow if form else wide).ptr), C.c_void_p(x.ptr),
                                                    C.c_void_p(r.ptr), C.c_uint64(SIZE), C.byref(s), C.c_uint64(form), C.c_uint64(0), C.byref(used),
                                                    C.c_uint64(0), C.c_uint64(hint), None))

    once = [(("conv %s %s" % (name, how)).strip(), lambda form=form, hint=hint: conv(form, hint))
            for name, form in (("wide", 0), ("narrow", NARROW)) for how, hint in (("", 0), ("nt", 1), ("cached", 2))]
    if not padded:
        gathered, r2 = S.DeviceBuffer(SIZE * inner * cols * words), S.DeviceBuffer(SIZE * oc * cols * words)
        m = im2col(d, s)

        def gather():
            S._native.check(lib.shl_reduce_mapped(d.ctx._h, C.c_uint64(ci), C.c_int(0), C.c_void_p(x.ptr), C.c_uint64(items), None, C.c_uint64(0),
                                                  C.c_void_p(gathered.ptr), C.c_uint64(SIZE), m._h, C.c_uint64(1), None, C.byref(used), None))

        def matmul(form):
            S._native.check(lib.shl_matmul_scalars_tile(d.ctx._h, C.c_uint64(ci), C.c_void_p((narrow if form else wide).ptr), C.c_void_p(gathered.ptr),
                                                        C.c_void_p(r2.ptr), C.c_uint64(SIZE), C.c_uint64(oc), C.c_uint64(inner), C.c_uint64(cols),
                                                        C.c_uint64(form), C.c_uint64(0), C.byref(used), C.c_uint64(0), None))

        once += [("gather", gather), ("matmul wide", lambda: matmul(0)), ("matmul narrow", lambda: matmul(NARROW))]

    def many(fn):
        def run():
            for _ in range(a.inner):
                fn()
        return run

    ms = {name: [v / a.inner for v in vals] for name, vals in interleaved([(name, many(fn)) for name, fn in once], a.reps).items()}
    slices = {}
    for name, fn in once:
        fn()
        slices[name] = used.value
    S.device_synchronize()
    macs = SIZE * oc * s.in_channels * live_taps(s) * words
    med = {name: max(float(np.median(v)), 1e-9) for name, v in ms.items()}
    geometry = "C = %d, %d x %d, OC = %d, %d x %d, stride (%d, %d), pad (%d, %d)" % tuple(getattr(s, f) for f, _ in s._fields_)
    lines.append("N = %d, K = %d, size %d, %s -> %d x %d; median [min .. max] of %d interleaved samples of %d calls (HIP events), ms per call"
                 % (n, K, SIZE, geometry, oh, ow, a.reps, a.inner))
    for name, _ in once:
        v = ms[name]
        rate = "" if name == "gather" else "  %6.3f Tmac/s" % (macs / med[name] / 1e9)
        lines.append("  %-18s %9.4f [%9.4f .. %9.4f] ms%s  slices %2d" % (name, med[name], min(v), max(v), rate, slices[name]))
    conv_gb = SIZE * (items + oc * cols) * P / 1e9
    lines.append("  device memory of the operands: convolution %.2f GB (input + result)" % conv_gb
                 + ("" if padded else "; two calls %.2f GB (+ the gathered batch of %d items, %.2f GB)"
                    % (conv_gb + SIZE * inner * cols * P / 1e9, inner * cols, SIZE * inner * cols * P / 1e9)))
    row = [n, K, geometry]
    for form in ("wide", "narrow"):
        best = min(("conv %s nt" % form, "conv %s cached" % form), key=lambda k: med[k])
        lib_choice = "conv %s" % form   # hint 0: the library's choice
        if padded:
            lines.append("  %-6s nt / cached %.3f; no gathered route exists for a padded shape" % (form, med["conv %s nt" % form] / med["conv %s cached" % form]))
            row += ["%.4f (%.3f)" % (med[lib_choice], macs / med[lib_choice] / 1e9), "-", "-", "-"]
            continue
        control = "matmul %s" % form
        two = med["gather"] + med[control]
        spread = max(ms[control]) - min(ms[control])
        verdict = "not slower" if med[lib_choice] - two <= spread else "SLOWER THAN THE TWO CALLS BY MORE THAN THE CONTROL'S SPREAD"
        behind = med[lib_choice] - med[control]
        lines.append("  %-6s nt / cached %.3f (best: %s); two calls %.4f ms = gather %.4f + control %.4f; two calls / conv %.2f: %s; "
                     "conv - control %+.4f ms (control's spread %.4f ms)%s"
                     % (form, med["conv %s nt" % form] / med["conv %s cached" % form], best, two, med["gather"], med[control], two / med[lib_choice],
                        verdict, behind, spread, ": BELOW THE CONTROL'S RATE BY MORE THAN ITS SPREAD" if behind > spread else ""))
        row += ["%.4f (%.3f)" % (med[lib_choice], macs / med[lib_choice] / 1e9), "%.4f" % med["gather"],
                "%.4f (%.3f)" % (med[control], macs / med[control] / 1e9), "%.2f" % (two / med[lib_choice])]
    lines.append("")
    print("\n".join(lines[-len(once) - 5:]), file=sys.stderr, flush=True)   # progress
    table.append("| " + " | ".join(str(v) for v in row) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="calls per timed sample")
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, a short chain, two small shapes: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    ap.add_argument("--no-headline", action="store_true", help="skip the N = 65536 ring")
    ap.add_argument("--only", type=int, help="index of the one shape to run, at N = 65536 alone (a short run for a profiler)")
    a = ap.parse_args()
    S.load(a.lib)
    v = [C.c_uint64() for _ in range(4)]
    S._native.check(S._native.lib().shl_matmul_scalars_info(*[C.byref(x) for x in v]))
    lines = ["the library's row tile: wide %d, narrow %d; executed taps between two reductions: wide %d, narrow %d" % tuple(x.value for x in v), ""]
    heads = ["conv ms (Tmac/s)", "gather ms", "control ms (Tmac/s)", "two calls / conv"]
    table = ["| N | K | shape | " + " | ".join("%s %s" % (form, h) for form in ("wide", "narrow") for h in heads) + " |", "|---|---|---|" + "---|" * 8]
    if a.small:
        d = DeviceSide("ckks", 1024, coeff_modulus_create(1024, [60, 40, 60]))
        for g in ((2, 3, 3, 3, 2, 2, 1, 1, 0, 0), (2, 3, 3, 9, 3, 3, 1, 1, 1, 1)):
            shape(d, 1024, Conv2dShape(*g), a, lines, table)
    else:
        for n, bits in RINGS:
            if a.no_headline and n == 65536:
                continue
            if a.only is not None and n != 65536:
                continue
            d = DeviceSide("ckks", n, coeff_modulus_create(n, bits))
            for g in (SHAPES if a.only is None else SHAPES[a.only:a.only + 1]):
                shape(d, n, Conv2dShape(*g), a, lines, table)
    text = "\n".join(lines + table) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
