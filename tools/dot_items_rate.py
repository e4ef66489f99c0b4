"""The ciphertext x ciphertext reduction over the items of two batches (Evaluator.dot_items) against its composition from forms of
the SAME build that it does not share code with, at the headline parameters (CKKS, N = 65536, {60, 14x50, 60}, batch 256) and at
the mid chain (N = 8192, {60, 40, 40, 60}, batch 256), both operands of size 2:

  fused g        Evaluator.dot_items(x, y, g), g = batch and g = 8
  composed g     Evaluator.multiply(x, y, w) into a third batch, then Evaluator.sum_items(w, g)
  square ...     the same with y = x (the sum of squares)

By bytes (P = one plane of the batch, g = group): the fused form reads 4 P (2 P for a square) and writes 3 P / g; the composed one
reads 4 P (2 P) and writes 3 P for the product, then reads 3 P and writes 3 P / g for the sum.  GB/s are these bytes over the median
time.  The composed form also holds the product batch w of 3 P words, which the fused form never allocates.

The calls are interleaved repetition by repetition, HIP events on the evaluator's (NULL) stream around each call, one warm-up round
first; median and range per cell, the measured time ratio next to the byte ratio, and the spread of a form against itself.

  python tools/dot_items_rate.py [--batch 256] [--reps 10] [--out FILE] [--small] [--lib PATH] [--no-headline]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import seal_amd as S
from harness import DeviceSide
from oracle import coeff_modulus_create

SHAPES = [(65536, [60] + [50] * 14 + [60]), (8192, [60, 40, 40, 60])]


def interleaved(fns, reps):
    """{name: [ms]}: every repetition times each call once, in turn"""
    for _, fn in fns:
        fn()
    S.device_synchronize()
    tm, out = S.HipTimer(), {name: [] for name, _ in fns}
    for _ in range(reps):
        for name, fn in fns:
            tm.start()
            fn()
            out[name].append(tm.stop())
    return out


def cell(ms, nbytes):
    med = float(np.median(ms))
    return "%8.3f [%8.3f .. %8.3f] ms  %7.1f GB/s" % (med, min(ms), max(ms), nbytes / max(med, 1e-9) / 1e6)


def composition(n, bits, a, lines):
    d = DeviceSide("ckks", n, coeff_modulus_create(n, bits))
    ev = d.ev
    enc = S.Encryptor(d.ctx, S.KeyGenerator(d.ctx).secret_key())
    coder = S.CKKSEncoder(d.ctx)
    pid, scale, batch = d.ctx.first_parms_id(), 2.0 ** 30, a.batch
    K = len(d.ctx.coeff_modulus_at(d.ctx.chain_index(pid)))
    rng = np.random.default_rng(1)
    x, y = (enc.encrypt_symmetric_device(coder.encode_device(S.DeviceBuffer.from_array(rng.standard_normal((batch, n // 2))), batch, pid, scale),
                                         batch, pid, scale) for _ in range(2))
    w = S.Ciphertext(d.ctx, batch=batch)
    P = batch * K * n * 8
    groups = [batch] + ([8] if batch % 8 == 0 and batch > 8 else [])
    fused = {g: S.Ciphertext(d.ctx, batch=batch // g) for g in groups}
    summed = {g: S.Ciphertext(d.ctx, batch=batch // g) for g in groups}

    def composed(g, other):
        ev.multiply(x, other, w)
        ev.sum_items(w, g, summed[g])

    fns, nbytes, pairs = [], {}, []
    for g in groups:
        fns += [("fused g=%d" % g, (lambda g=g: ev.dot_items(x, y, g, fused[g]))), ("composed g=%d" % g, (lambda g=g: composed(g, y)))]
        nbytes["fused g=%d" % g], nbytes["composed g=%d" % g] = 4 * P + 3 * P // g, 4 * P + 3 * P + 3 * P + 3 * P // g
        pairs.append(("fused g=%d" % g, "composed g=%d" % g))
    fns += [("square fused g=%d" % batch, lambda: ev.dot_items(x, x, batch, fused[batch])), ("square composed g=%d" % batch, lambda: composed(batch, x))]
    nbytes["square fused g=%d" % batch], nbytes["square composed g=%d" % batch] = 2 * P + 3 * P // batch, 2 * P + 3 * P + 3 * P + 3 * P // batch
    pairs.append(("square fused g=%d" % batch, "square composed g=%d" % batch))
    ms = interleaved(fns, a.reps)
    for g in groups:   # the two forms give the same words (for g = batch the last calls were the squares)
        assert np.array_equal(fused[g].to_numpy(), summed[g].to_numpy()), "fused and composed forms disagree"
    lines.append("CKKS N = %d, K = %d, batch %d, size 2 x 2; median [min .. max] of %d interleaved repetitions (HIP events)" % (n, K, batch, a.reps))
    for name, _ in fns:
        lines.append("  %-24s %s" % (name, cell(ms[name], nbytes[name])))
    for f_name, c_name in pairs:
        f, c = ms[f_name], ms[c_name]
        lines.append("  %-22s / %-24s: composed / fused time %.3f, by bytes %.3f; the composed form against itself: max / min = %.3f"
                     % (c_name, f_name, np.median(c) / max(np.median(f), 1e-9), nbytes[c_name] / nbytes[f_name], max(c) / max(min(c), 1e-9)))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, a short chain, batch 16: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    ap.add_argument("--no-headline", action="store_true", help="skip the N = 65536 shape")
    a = ap.parse_args()
    global SHAPES
    if a.small:
        SHAPES = [(1024, [60, 40, 60])]
        a.batch = min(a.batch, 16)
    S.load(a.lib)
    lines = []
    for n, bits in SHAPES:
        if not (a.no_headline and n == 65536):
            composition(n, bits, a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
