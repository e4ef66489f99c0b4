"""Sums over the items of a device-resident batch against their composition from the per-item and per-object forms of the SAME
build, at the headline parameters (CKKS, N = 65536, {60, 14x50, 60}, batch 256, size 2) and at one small-destination shape
(N = 8192, {60, 40, 40, 60}, batch 256):

  dot fused      Evaluator.dot_plain_device, group = batch and group = 16
  dot composed   Evaluator.multiply_plain_device into a second batch, then Evaluator.add_many over per-item handles (the items
                 are copied into the handles before the clock starts: the composition is not charged for having no other route)
  sum fused      Evaluator.sum_items, group = batch
  sum composed   Evaluator.add_many over the per-item handles

By bytes (P = one plane of the batch, size = polynomials per ciphertext, g = group): the fused dot product reads (size + 1) P and
writes size P / g; the composed one moves (2 size + 1) P for the product and about 3 size P for the chain of adds; the fused sum
reads size P and writes size P / g against the chain's 3 size P.  GB/s are these bytes over the median time.

The calls are interleaved repetition by repetition, HIP events on the evaluator's (NULL) stream around each call, one warm-up round
first; median and range per cell, the measured time ratio next to the byte ratio, and the spread of a form against itself.

Sweep: the kernels on raw words (shl_reduce_items) at N = 8192, K = 3, size 2, groups of 64, for 1 .. 64 output items, in one
launch and cut into 2 .. 64 slices: where the one-launch form catches up sets the threshold, the fastest cut the slice count.

Item maps (--mapped): the kernels on raw words through the seams, by the library's rule, at the sweep's shapes (N = 8192, K = 3,
groups of 64, 1 .. 64 output items) and at the headline level (N = 65536, K = 15, batch 256 in groups of 16), for the sum, the
plaintext dot product and the ciphertext dot product, interleaved sample by sample:
  (a) the contiguous form (shl_reduce_items / shl_dot_items) of this build - and, with --parent-lib, of the library built from the
      parent commit, timed TWICE in every round (its A/A spread) next to this build's;
  (b) shl_reduce_mapped with the identity map (rows of g consecutive items): (b) / (a) is the cost of the walk;
  (c) a random permutation of the same items in the same rows;
  (d) a ragged map with the same number of terms (row lengths drawn at random, every item once).
A sample is the time of --inner calls between two HIP events; GB/s are the bytes the reduction needs over the median sample.

  python tools/batch_reduce_rate.py [--batch 256] [--reps 10] [--out FILE] [--small] [--lib PATH] [--no-headline] [--no-sweep]
                                    [--mapped [--parent-lib PATH] [--inner 20] [--mapped-out FILE]] [--no-composition]"""
import argparse
import ctypes as C
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
SWEEP_N, SWEEP_BITS, SWEEP_GROUP = 8192, [60, 40, 40, 60], 64


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
    pid, scale, batch, size = d.ctx.first_parms_id(), 2.0 ** 30, a.batch, 2
    K = len(d.ctx.coeff_modulus_at(d.ctx.chain_index(pid)))
    rng = np.random.default_rng(1)
    words = coder.encode_device(S.DeviceBuffer.from_array(rng.standard_normal((batch, n // 2))), batch, pid, scale)
    ct = enc.encrypt_symmetric_device(words, batch, pid, scale)
    product = S.Ciphertext(d.ctx, batch=batch)
    items = [S.Ciphertext(d.ctx) for _ in range(batch)]   # per-item handles, filled off the clock
    for b in range(batch):
        items[b].load_bytes(ct.save_bytes(item=b))
    total = S.Ciphertext(d.ctx)
    P = batch * K * n * 8
    groups = [batch] + ([16] if batch % 16 == 0 and batch > 16 else [])
    dests = {g: S.Ciphertext(d.ctx, batch=batch // g) for g in groups}

    def composed_dot():
        ev.multiply_plain_device(ct, words, True, scale, destination=product)
        ev.add_many(items, total)

    fns = [("dot fused g=%d" % g, (lambda g=g: ev.dot_plain_device(ct, words, scale, g, dests[g]))) for g in groups]
    fns += [("dot composed", composed_dot),
            ("sum fused g=%d" % batch, lambda: ev.sum_items(ct, batch, dests[batch])),
            ("sum composed", lambda: ev.add_many(items, total))]
    ms = interleaved(fns, a.reps)
    nbytes = {"dot composed": (2 * size + 1) * P + 3 * size * P, "sum composed": 3 * size * P, "sum fused g=%d" % batch: size * P + size * P // batch}
    for g in groups:
        nbytes["dot fused g=%d" % g] = (size + 1) * P + size * P // g
    lines.append("CKKS N = %d, K = %d, batch %d, size %d; median [min .. max] of %d interleaved repetitions (HIP events)" % (n, K, batch, size, a.reps))
    for name, _ in fns:
        lines.append("  %-20s %s" % (name, cell(ms[name], nbytes[name])))
    for fused, comp in [("dot fused g=%d" % g, "dot composed") for g in groups] + [("sum fused g=%d" % batch, "sum composed")]:
        f, c = ms[fused], ms[comp]
        lines.append("  %-18s / %-12s: measured %.3f, by bytes %.3f; the composed form against itself: max / min = %.3f"
                     % (fused, comp, np.median(f) / max(np.median(c), 1e-9), nbytes[fused] / nbytes[comp], max(c) / max(min(c), 1e-9)))
    lines.append("")


def sweep(a, lines):
    n, group, size = SWEEP_N, SWEEP_GROUP, 2
    d = DeviceSide("ckks", n, coeff_modulus_create(n, SWEEP_BITS))
    ci = d.ctx.chain_index(d.ctx.first_parms_id())
    q = np.array(d.ctx.coeff_modulus_at(ci), dtype=np.uint64)
    K = q.size
    lib, rng = S._native.lib(), np.random.default_rng(2)
    cuts = [1, 2, 4, 8, 16, 32, 64]
    lines.append("kernels on raw words, N = %d, K = %d, size %d, groups of %d; median ms of %d interleaved repetitions; columns = slices"
                 % (n, K, size, group, a.reps))
    lines.append("  %-22s %s   library's rule" % ("", " ".join("%8d" % s for s in cuts)))
    sizes = (1, 2, 4, 8, 16, 32, 64)
    # one set of words for every row: each [K][N] block holds words below its primes, whatever batch the buffer is read as
    top = max(sizes) * group
    x = S.DeviceBuffer.from_numpy((rng.integers(0, 2 ** 63, (size, top, K, n), dtype=np.uint64) % q[None, None, :, None]).astype(np.uint64))
    pl = S.DeviceBuffer.from_numpy((rng.integers(0, 2 ** 63, (top, K, n), dtype=np.uint64) % q[None, :, None]).astype(np.uint64))
    r, scratch = S.DeviceBuffer(size * max(sizes) * K * n), S.DeviceBuffer(max(cuts) * size * max(sizes) * K * n)
    for out_items in sizes:
        batch = out_items * group
        for what, plain in (("sum", None), ("dot", pl)):
            used = C.c_uint64()

            def run(slices, rp=r.ptr):
                S._native.check(lib.shl_reduce_items(d.ctx._h, C.c_uint64(ci), C.c_void_p(x.ptr), C.c_void_p(plain.ptr if plain else None),
                                                     C.c_void_p(rp), C.c_uint64(size), C.c_uint64(batch), C.c_uint64(group), C.c_uint64(slices),
                                                     C.c_void_p(scratch.ptr), C.byref(used), None))
            run(0, None)
            rule = used.value
            ms = interleaved([(s, (lambda s=s: run(s))) for s in cuts], a.reps)
            threads = (1 if plain else size) * out_items * K * n // 2
            lines.append("  %s %3d items %7d thr %s   %d" % (what, out_items, threads, " ".join("%8.4f" % np.median(ms[s]) for s in cuts), rule))
    lines.append("")


def parent_context(path, n, primes):
    """the library built from the parent commit, with a CKKS context of its own (handles of one library never reach the other; the
    context lives until the process ends)"""
    lib = C.CDLL(os.path.abspath(path))
    for name in ("EncParams_Create1", "EncParams_SetPolyModulusDegree", "EncParams_SetCoeffModulus", "SEALContext_Create", "shl_reduce_items",
                 "shl_dot_items"):
        getattr(lib, name).restype = C.c_long
    parms, ctx = C.c_void_p(), C.c_void_p()
    for hr in (lib.EncParams_Create1(C.c_uint8(2), C.byref(parms)), lib.EncParams_SetPolyModulusDegree(parms, C.c_uint64(n)),
               lib.EncParams_SetCoeffModulus(parms, C.c_uint64(len(primes)), (C.c_uint64 * len(primes))(*primes)),
               lib.SEALContext_Create(parms, C.c_bool(True), C.c_int(0), C.byref(ctx))):
        if hr & 0xFFFFFFFF:
            raise RuntimeError("parent library: HRESULT 0x%08X" % (hr & 0xFFFFFFFF))
    return lib, ctx


def ragged_lengths(rng, rows, terms):
    """`rows` lengths >= 1 that add up to `terms`"""
    if rows == 1:
        return [terms]
    cuts = np.sort(rng.choice(np.arange(1, terms), rows - 1, replace=False))
    return [int(v) for v in np.diff(np.concatenate(([0], cuts, [terms])))]


def mapped(a, lines, table):
    size = 2
    shapes = [(SWEEP_N, SWEEP_BITS, out_items * SWEEP_GROUP, SWEEP_GROUP) for out_items in (1, 2, 4, 8, 16, 32, 64)]
    if not a.no_headline:
        shapes.append((SHAPES[0][0], SHAPES[0][1], a.batch, 16 if a.batch % 16 == 0 and a.batch > 16 else a.batch))
    rng = np.random.default_rng(3)
    held = {}
    for n, bits, batch, group in shapes:
        primes = coeff_modulus_create(n, bits)
        if (n, tuple(bits)) not in held:
            d = DeviceSide("ckks", n, primes)
            held[(n, tuple(bits))] = (d, parent_context(a.parent_lib, n, primes) if a.parent_lib else None)
        d, parent = held[(n, tuple(bits))]
        lib, ci = S._native.lib(), d.ctx.chain_index(d.ctx.first_parms_id())
        K, rows = len(d.ctx.coeff_modulus_at(ci)), batch // group
        words = K * n
        P = batch * words * 8
        # timing does not depend on the words: the operands are whatever the allocation holds (the tests own correctness)
        x, y, pl = S.DeviceBuffer(size * batch * words), S.DeviceBuffer(size * batch * words), S.DeviceBuffer(batch * words)
        r = S.DeviceBuffer(3 * rows * words)
        identity = [list(range(o * group, (o + 1) * group)) for o in range(rows)]
        perm = [int(v) for v in rng.permutation(batch)]
        permuted = [perm[o * group:(o + 1) * group] for o in range(rows)]
        lengths, at, ragged = ragged_lengths(rng, rows, batch), 0, []
        for ln in lengths:
            ragged.append(perm[at:at + ln])
            at += ln
        maps = {"identity map": S.ItemMap(d.ctx, identity, batch), "permuted map": S.ItemMap(d.ctx, permuted, batch),
                "ragged map": S.ItemMap(d.ctx, ragged, batch)}
        lines.append("N = %d, K = %d, size %d, batch %d in %d rows (contiguous: groups of %d; ragged rows: %d .. %d terms); median "
                     "[min .. max] of %d interleaved samples of %d calls each (HIP events), ms per call"
                     % (n, K, size, batch, rows, group, min(lengths), max(lengths), a.reps, a.inner))
        used = C.c_uint64()
        # scratch for the widest cut the rule makes of these maps (the contiguous forms cut like the identity map)
        most = 1
        for m in maps.values():
            for kind in (0, 1, 2):
                S._native.check(lib.shl_reduce_mapped(d.ctx._h, C.c_uint64(ci), C.c_int(kind), None, C.c_uint64(batch), None,
                                                      C.c_uint64(batch if kind else 0), None, C.c_uint64(size), m._h, C.c_uint64(0), None,
                                                      C.byref(used), None))
                most = max(most, used.value)
        scratch = S.DeviceBuffer(most * 3 * rows * words)
        for kind, what, nbytes in ((0, "sum", size * P + size * P // group), (1, "dot plain", (size + 1) * P + size * P // group),
                                   (2, "dot items", 4 * P + 3 * P // group)):
            b = None if kind == 0 else (pl if kind == 1 else y)

            def contiguous(l, ctx_h):
                if kind == 2:
                    hr = l.shl_dot_items(ctx_h, C.c_uint64(ci), C.c_void_p(x.ptr), C.c_void_p(y.ptr), C.c_void_p(r.ptr), C.c_uint64(batch),
                                         C.c_uint64(group), C.c_uint64(0), C.c_void_p(scratch.ptr), C.byref(used), None)
                else:
                    hr = l.shl_reduce_items(ctx_h, C.c_uint64(ci), C.c_void_p(x.ptr), C.c_void_p(b.ptr if b else None), C.c_void_p(r.ptr),
                                            C.c_uint64(size), C.c_uint64(batch), C.c_uint64(group), C.c_uint64(0), C.c_void_p(scratch.ptr),
                                            C.byref(used), None)
                S._native.check(hr)

            def through_map(m):
                S._native.check(lib.shl_reduce_mapped(d.ctx._h, C.c_uint64(ci), C.c_int(kind), C.c_void_p(x.ptr), C.c_uint64(batch),
                                                      C.c_void_p(b.ptr if b else None), C.c_uint64(batch if b else 0), C.c_void_p(r.ptr),
                                                      C.c_uint64(size), m._h, C.c_uint64(0), C.c_void_p(scratch.ptr), C.byref(used), None))

            def many(fn):
                def run():
                    for _ in range(a.inner):
                        fn()
                return run

            fns = [("contiguous", many(lambda: contiguous(lib, d.ctx._h)))]
            if parent:
                fns += [("parent A", many(lambda: contiguous(*parent))), ("parent B", many(lambda: contiguous(*parent)))]
            fns += [(name, many(lambda m=m: through_map(m))) for name, m in maps.items()]
            ms = {name: [v / a.inner for v in vals] for name, vals in interleaved(fns, a.reps).items()}
            slices = {}
            for name, m in maps.items():
                through_map(m)
                slices[name] = used.value
            contiguous(lib, d.ctx._h)
            slices["contiguous"] = used.value
            S.device_synchronize()
            med = {name: max(float(np.median(v)), 1e-9) for name, v in ms.items()}
            for name, _ in fns:
                lines.append("  %-10s %-13s %s%s" % (what, name, cell(ms[name], nbytes), "  slices %d" % slices[name] if name in slices else ""))
            ratios = "identity / contiguous %.3f, permuted / contiguous %.3f, ragged / contiguous %.3f" % tuple(
                med[k] / med["contiguous"] for k in ("identity map", "permuted map", "ragged map"))
            if parent:
                ratios += "; this build / parent %.3f, parent A / parent B %.3f" % (
                    med["contiguous"] / (0.5 * (med["parent A"] + med["parent B"])), med["parent A"] / med["parent B"])
            lines.append("  %-10s %s" % (what, ratios))
            print("N = %d, %d rows: %s %s" % (n, rows, what, ratios), file=sys.stderr, flush=True)   # progress
            gbs = lambda k: nbytes / max(med[k], 1e-9) / 1e6
            table.append("| %d | %d | %d x %d | %s | %s | %.0f | %.0f | %.3f | %.0f | %.0f | %s |" % (
                n, K, rows, group, what, "%.0f (A / B %.3f)" % (gbs("parent A"), med["parent A"] / med["parent B"]) if parent else "-",
                gbs("contiguous"), gbs("identity map"), med["identity map"] / med["contiguous"], gbs("permuted map"), gbs("ragged map"),
                "%.3f" % (med["contiguous"] / (0.5 * (med["parent A"] + med["parent B"]))) if parent else "-"))
        lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="N = 1024, short chains, batch 32: a dry run of this script")
    ap.add_argument("--lib", help="library to load instead of the gfx950 build (the emulated one, for a dry run)")
    ap.add_argument("--no-headline", action="store_true", help="skip the N = 65536 shape")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-composition", action="store_true", help="skip the fused forms against their composition")
    ap.add_argument("--mapped", action="store_true", help="item maps next to the contiguous forms (see above)")
    ap.add_argument("--parent-lib", help="libsealhip.so built from the parent commit: timed next to this build, twice per round")
    ap.add_argument("--inner", type=int, default=20, help="calls per timed sample of --mapped")
    ap.add_argument("--mapped-out", help="file for the --mapped section (default: --out)")
    a = ap.parse_args()
    global SHAPES, SWEEP_N, SWEEP_BITS, SWEEP_GROUP
    if a.small:
        SHAPES, SWEEP_N, SWEEP_BITS, SWEEP_GROUP = [(1024, [60, 40, 60])], 64, [60, 40, 60], 64
        a.batch = min(a.batch, 32)
    S.load(a.lib)
    lines = []
    for n, bits in SHAPES:
        if not (a.no_headline and n == 65536) and not a.no_composition:
            composition(n, bits, a, lines)
    if not a.no_sweep:
        sweep(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if a.mapped:
        lines, table = [], ["| N | K | rows x group | term | parent GB/s | this build GB/s | identity map GB/s | identity / contiguous | permuted GB/s | ragged GB/s | this build / parent |",
                            "|---|---|---|---|---|---|---|---|---|---|---|"]
        mapped(a, lines, table)
        text = "\n".join(lines + table) + "\n"
        print(text)
        if a.mapped_out or a.out:
            path = a.mapped_out or a.out
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
