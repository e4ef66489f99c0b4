"""BEHZ base conversions of BFV multiplication (behz_kernels.hip) at every dispatch class and at their bounds: one body for the CPU
(fiber emulator, test_behz.py) and the device (test_gpu_behz.py).

Three things are held against each other, word for word:
  * Model - the reference's integer formulas (util/rns.cpp:903-1131, the x t of evaluator.cpp:549-566) restated in Python integers
    from nothing but the level's primes, the base Bsk, t and m~ = 2^32.  It also returns what the cases steer: the vectors y that
    enter each dot product, the m~-residue r, alpha and its sign.
  * the oracle's stages (Oracle.rns_stage), which hold the model to the reference;
  * the library: the fused kernels (shl_rns_stage "lift" / "floor_sk") and the staged kernels 0-3.

The steered patterns solve input words in the model so that r, alpha and the dot products' vectors sit on the kernels' own edges;
each asserts from the model that the edge was reached before anything runs on the library."""
import functools
from math import prod

import numpy as np

import seal_amd as S
from harness import DeviceSide
from oracle import Oracle, coeff_modulus_create, plain_modulus_batching, rand_ct

MT = 1 << 32
POLYS = 5                                   # 320 coefficients at N = 64: one full block of 256, one partial, items end inside a block
MIXED = (45, 50, 55, 58, 60, 30)            # component 0 above 2^32 (the r steering needs y_0 to range over all of [0, 2^32))

# name -> (N, bit sizes of the data primes, bits of t or None = the smallest that adds a prime to B, expected |B| - K)
CONFIGS = {}


def _cfg(name, n, bits, t_bits, extra):
    CONFIGS[name] = (n, list(bits), t_bits, extra)


def _mixed(K):
    return [MIXED[i % len(MIXED)] for i in range(K)]


_cfg("K01", 64, [60], 20, 0)
_cfg("K01_nB02", 64, [60], None, 1)
_cfg("K04", 64, [60] * 4, 20, 0)
_cfg("K04_nB05", 64, [60] * 4, None, 1)      # lift class <4>, tail class <8>
_cfg("K05_mixed", 64, _mixed(5), 20, 0)
_cfg("K08", 64, [60] * 8, 20, 0)
_cfg("K08_nB09", 64, [60] * 8, None, 1)
_cfg("K09_mixed", 64, _mixed(9), 20, 0)
_cfg("K16", 64, [60] * 16, 20, 0)
_cfg("K16_nB17", 64, [60] * 16, None, 1)
_cfg("K17_mixed", 64, _mixed(17), 20, 0)
_cfg("K32_mixed", 64, _mixed(32), 20, 0)     # |Bsk| = 33: the first dynamic LDS request above 64 KiB
_cfg("K33_mixed", 64, _mixed(33), 20, 0)
_cfg("K63_mixed", 16, _mixed(63), 20, 0)     # L = 64, the longest chain
ORDER = list(CONFIGS)                         # ascending K: a refused launch names its size
THRESHOLD = [c for c in ORDER if CONFIGS[c][2] is None]
# one per dispatch class of either kernel, and the two where the classes of the two kernels differ or B has its extra prime
EVALUATOR = ["K04", "K04_nB05", "K08", "K16", "K16_nB17", "K32_mixed", "K63_mixed"]
STRIDE = ("K03_stride", 64, [45, 50, 60], 20)
STRIDE_POLYS = 8200                           # 8200 * 64 = 524800 coefficients > 2048 blocks * 256: the grid-stride loop's second trip


def _eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, "%s: shape %s vs %s" % (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError("%s: %d of %d words differ, first at %s: got %d expected %d" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])]))


def _col(v):
    return np.array([int(x) for x in v], dtype=object)[:, None]


def _obj(a):
    return np.asarray(a).astype(object)


def _u64(a):
    return np.array(a, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the model
class Model:
    """every array is [components][coefficients] of Python integers"""

    def __init__(self, q, bsk, t):
        self.q, self.bsk, self.t = [int(x) for x in q], [int(x) for x in bsk], int(t)
        self.B, self.msk = self.bsk[:-1], self.bsk[-1]
        self.K, self.nB, self.nBsk = len(self.q), len(self.B), len(self.bsk)
        q, B, bsk, msk = self.q, self.B, self.bsk, self.msk
        self.Q, self.PB = prod(q), prod(B)
        self.punct_q = [self.Q // x for x in q]
        self.punct_b = [self.PB // x for x in B]
        self.inv_punct_q = _col([pow(p % x, -1, x) for p, x in zip(self.punct_q, q)])
        self.inv_punct_b = _col([pow(p % x, -1, x) for p, x in zip(self.punct_b, B)])
        self.qc, self.Bc, self.bskc = _col(q), _col(B), _col(bsk)
        # BaseConverter matrices (rns.cpp:418-463): [output modulus][input component]
        self.q_to_bsk = np.array([[p % m for p in self.punct_q] for m in bsk], dtype=object).reshape(self.nBsk, self.K)
        self.q_to_mt = np.array([[p % MT for p in self.punct_q]], dtype=object).reshape(1, self.K)
        self.b_to_q = np.array([[p % m for p in self.punct_b] for m in q], dtype=object).reshape(self.K, self.nB)
        self.b_to_msk = np.array([[p % msk for p in self.punct_b]], dtype=object).reshape(1, self.nB)
        self.neg_inv_q_mt = (MT - pow(self.Q % MT, -1, MT)) % MT
        self.inv_mt_bsk = _col([pow(MT % m, -1, m) for m in bsk])
        self.inv_q_bsk = _col([pow(self.Q % m, -1, m) for m in bsk])
        self.inv_b_msk = pow(self.PB % msk, -1, msk)

    # rns.cpp:1086-1131
    def fastbconv_m_tilde(self, x):
        temp = (x * (MT % self.qc)) % self.qc
        y = (temp * self.inv_punct_q) % self.qc
        out = np.concatenate([self.q_to_bsk.dot(y) % self.bskc, self.q_to_mt.dot(y) % MT])
        return out, dict(y=y)

    # rns.cpp:979-1039
    def sm_mrq(self, x):
        r = (x[self.nBsk] * self.neg_inv_q_mt) % MT
        upper = np.array(r >= (MT >> 1), dtype=bool)
        out = np.empty((self.nBsk, x.shape[1]), dtype=object)
        for j, m in enumerate(self.bsk):
            temp = np.where(upper, r + (m - MT), r)
            out[j] = (((temp * (self.Q % m) + x[j]) % m) * int(self.inv_mt_bsk[j, 0])) % m
        return out, dict(r=r)

    # rns.cpp:1041-1084
    def fast_floor(self, x):
        y = (x[:self.K] * self.inv_punct_q) % self.qc
        conv = self.q_to_bsk.dot(y) % self.bskc
        out = ((x[self.K:] + (self.bskc - conv)) * self.inv_q_bsk) % self.bskc
        return out, dict(yq=y)

    # rns.cpp:903-977
    def fastbconv_sk(self, x):
        y = (x[:self.nB] * self.inv_punct_b) % self.Bc
        g = self.b_to_q.dot(y) % self.qc
        temp = (self.b_to_msk.dot(y) % self.msk)[0]
        alpha = ((temp + (self.msk - x[self.nB])) * self.inv_b_msk) % self.msk
        negative = np.array(alpha > (self.msk >> 1), dtype=bool)
        out = np.empty((self.K, x.shape[1]), dtype=object)
        for i, m in enumerate(self.q):
            pb = self.PB % m
            out[i] = np.where(negative, ((self.msk - alpha) * pb + g[i]) % m, (alpha * (m - pb) + g[i]) % m)
        return out, dict(yb=y, alpha=alpha, negative=negative)

    def times_t(self, x):
        """evaluator.cpp:554-556 on [K + |Bsk|] components"""
        mods = np.concatenate([self.qc, self.bskc])
        return (x * self.t) % mods

    def lift(self, x):
        a, ia = self.fastbconv_m_tilde(x)
        b, ib = self.sm_mrq(a)
        return b, dict(ia, **ib)

    def tail(self, x):
        a, ia = self.fast_floor(self.times_t(x))
        b, ib = self.fastbconv_sk(a)
        return b, dict(ia, **ib)

    # ---- inverses, for steering
    def lift_input_for_y(self, y):
        """x with fastbconv_m_tilde's y equal to the argument (y_i < q_i)"""
        return (y * _col([pow((MT % m) * int(c) % m, -1, m) for m, c in zip(self.q, self.inv_punct_q[:, 0])])) % self.qc

    def r_coefficients(self):
        """r = sum_i y_i c_i mod 2^32, every c_i odd"""
        return [(p % MT) * self.neg_inv_q_mt % MT for p in self.punct_q]

    def tail_q_input_for_y(self, y):
        inv_t = _col([pow(self.t % m, -1, m) for m in self.q])
        return ((y * _col(self.punct_q)) % self.qc * inv_t) % self.qc

    def tail_b_input_for(self, xq, yb, alpha):
        """the Bsk part of the tail's input for which fastbconv_sk sees the vector yb (yb_i < b_i) and the given alpha, next to the
        q part xq: f_i = yb_i (B/b_i), f_sk = conv_sk - alpha B, and input = (f Q + conv) t^-1 componentwise"""
        zq = (xq * self.t) % self.qc
        conv = self.q_to_bsk.dot((zq * self.inv_punct_q) % self.qc) % self.bskc
        f = np.empty((self.nBsk, xq.shape[1]), dtype=object)
        f[:self.nB] = (yb * _col(self.punct_b)) % self.Bc
        f[self.nB] = ((self.b_to_msk.dot(yb) % self.msk)[0] - alpha * self.PB) % self.msk
        inv_t = _col([pow(self.t % m, -1, m) for m in self.bsk])
        return (((f * _col([self.Q % m for m in self.bsk]) + conv) % self.bskc) * inv_t) % self.bskc


# ---------------------------------------------------------------------------------------------------------------- parameters
def _t_bits_threshold(primes, K):
    """smallest bit count of t at which RNSTool::initialize (rns.cpp:605-632) gives B one prime more than q has, from the level's
    actual total_coeff_modulus_bit_count: 32 + bits(t) + total >= 61 K + 61"""
    total = prod(primes[:K]).bit_length()
    return 61 * K + 61 - 32 - total, total


class Setup:
    def __init__(self, name, n, bits, t_bits):
        self.name, self.n, self.K = name, n, len(bits)
        K = self.K
        chain = list(bits) if K == 1 else list(bits) + [60]   # K = 1: the single-prime chain; otherwise one special prime on top
        self.primes = coeff_modulus_create(n, chain)
        self.t_bits_threshold, self.total_bits = _t_bits_threshold(self.primes, K)
        if t_bits is None:
            t_bits = self.t_bits_threshold
            assert t_bits <= 60, "%s: no plain modulus is large enough for |B| = K + 1" % name
        self.t_bits = t_bits
        self.t = plain_modulus_batching(n, t_bits)
        self.o = Oracle("bfv", n, self.primes, self.t)
        self.bsk = self.o.base_bsk(K)
        self.model = Model(self.primes[:K], self.bsk, self.t)
        self.nBsk = len(self.bsk)

    def device(self):
        d = DeviceSide("bfv", self.n, self.primes, self.t)
        return d, d.chain_index_for_K(self.K)


@functools.lru_cache(maxsize=None)
def setup(name):
    if name == STRIDE[0]:
        return Setup(*STRIDE)
    n, bits, t_bits, _ = CONFIGS[name]
    return Setup(name, n, bits, t_bits)


# ---------------------------------------------------------------------------------------------------------------- patterns
R_TARGETS = (0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1)


def alpha_targets(msk):
    return (0, 1, (msk - 1) // 2, (msk + 1) // 2, msk - 1)


def _rand(rng, mods, cols):
    return np.stack([rng.integers(0, m, cols, dtype=np.uint64) for m in mods]).astype(object)


def _steer_slots(cols):
    """coefficient -> index of the target it is steered to, or -1: every target in the first and in the last five coefficients of
    the slab and on either side of the block boundary at 256 (where there is one)"""
    slot = np.full(cols, -1)
    for base in (0, 254, cols - 5):
        if 0 <= base and base + 5 <= cols:
            slot[base:base + 5] = np.arange(5)
    return slot


def lift_patterns(s, rng):
    """name -> [K][POLYS * N] inputs of the lift; the steered ones assert their own success in the model"""
    m, cols = s.model, POLYS * s.n
    pats = {"random": _rand(rng, m.q, cols), "zero": np.zeros((m.K, cols), dtype=object), "words_max": np.tile(m.qc - 1, (1, cols))}
    x = m.lift_input_for_y(np.tile(m.qc - 1, (1, cols)))
    _, im = m.fastbconv_m_tilde(x)
    assert (im["y"] == m.qc - 1).all(), "maximal vector not reached"
    pats["y_max"] = x
    assert m.q[0] > MT, "the r steering needs component 0 above 2^32"
    # r is linear in y_0 mod 2^32 with an odd coefficient: solve y_0 in the model, then x_0
    x = _rand(rng, m.q, cols)
    _, im = m.fastbconv_m_tilde(x)
    y, c = im["y"], m.r_coefficients()
    slot = _steer_slots(cols)
    rest = sum(y[i] * c[i] for i in range(1, m.K)) if m.K > 1 else np.zeros(cols, dtype=object)
    inv_c0 = pow(c[0], -1, MT)
    for col in np.nonzero(slot >= 0)[0]:
        y[0, col] = (R_TARGETS[slot[col]] - int(rest[col])) * inv_c0 % MT
    x = m.lift_input_for_y(y)
    _, im = m.lift(x)
    for k, target in enumerate(R_TARGETS):
        hit = im["r"][slot == k]
        assert len(hit) >= 1 and (hit == target).all(), "r = %d not reached" % target
    pats["r_steered"] = x
    return pats


def tail_patterns(s, rng):
    """name -> [K + |Bsk|][POLYS * N] inputs of the tail (before x t)"""
    m, cols = s.model, POLYS * s.n
    mods = m.q + m.bsk
    allc = np.concatenate([m.qc, m.bskc])
    pats = {"random": _rand(rng, mods, cols), "zero": np.zeros((len(mods), cols), dtype=object), "words_max": np.tile(allc - 1, (1, cols))}
    targets = alpha_targets(m.msk)
    slot = _steer_slots(cols)

    def steered(name, xq, yb, every):
        # alpha is an affine bijection of the m_sk word of the B-side input: solve that word (and, for maximal vectors, all of them)
        _, base = m.tail(np.concatenate([xq, _rand(rng, m.bsk, cols)]))
        alpha = base["alpha"].copy()
        which = np.arange(cols) % 5 if every else slot
        for col in np.nonzero(which >= 0)[0]:
            alpha[col] = targets[which[col]]
        x = np.concatenate([xq, m.tail_b_input_for(xq, yb, alpha)])
        _, im = m.tail(x)
        assert (im["yb"] == yb).all(), "%s: B-side vector not reached" % name
        for k, target in enumerate(targets):
            hit = im["alpha"][which == k]
            assert len(hit) >= 1 and (hit == target).all(), "%s: alpha = %d not reached" % (name, target)
            assert (im["negative"][which == k] == (target > m.msk >> 1)).all()
        pats[name] = x

    # every y entering the three dot products at p - 1; alpha cycles through its targets along the way
    yq_max = np.tile(m.qc - 1, (1, cols))
    xq_max = m.tail_q_input_for_y(yq_max)
    _, im = m.fast_floor(m.times_t(np.concatenate([xq_max, _rand(rng, m.bsk, cols)])))
    assert (im["yq"] == yq_max).all(), "maximal q-side vector not reached"
    steered("y_max", xq_max, np.tile(m.Bc - 1, (1, cols)), True)
    xq = _rand(rng, m.q, cols)
    steered("alpha_steered", xq, _rand(rng, m.B, cols), False)
    steered("alpha_steered_yb_max", xq, np.tile(m.Bc - 1, (1, cols)), False)
    return pats


def _polys(a, n):
    """[comps][POLYS * n] integers -> uint64 [POLYS][comps][n]"""
    a = _u64(a)
    return np.ascontiguousarray(a.reshape(a.shape[0], -1, n).transpose(1, 0, 2))


def _flat(a):
    """uint64 [polys][comps][n] -> [comps][polys * n] integers"""
    return _obj(a.transpose(1, 0, 2).reshape(a.shape[1], -1))


class Expected:
    """inputs and expected outputs of every pattern of one configuration, as uint64 [POLYS][comps][N]; computed once per process.
    The constructor holds the model to the oracle on every pattern, stage by stage and fused."""

    def __init__(self, s, seed):
        o, m, n, K, nBsk = s.o, s.model, s.n, s.K, s.nBsk
        rng = np.random.default_rng(seed)
        stage = lambda which, x, oc: np.stack([o.rns_stage(K, which, p, oc) for p in x])
        self.lift, self.tail, self.sm_mrq, self.sk = {}, {}, {}, {}
        for name, x in lift_patterns(s, rng).items():
            xin = _polys(x, n)
            e0 = stage("fastbconv_m_tilde", xin, nBsk + 1)
            e1 = stage("sm_mrq", e0, nBsk)
            _eq(_polys(m.fastbconv_m_tilde(x)[0], n), e0, "%s: model fastbconv_m_tilde vs oracle, %s" % (s.name, name))
            _eq(_polys(m.lift(x)[0], n), e1, "%s: model lift vs oracle stages 0, 1, %s" % (s.name, name))
            self.lift[name] = (xin, e0, e1)
        for name, x in tail_patterns(s, rng).items():
            xin, zin = _polys(x, n), _polys(m.times_t(x), n)
            e2 = stage("fast_floor", zin, nBsk)
            e3 = stage("fastbconv_sk", e2, K)
            _eq(_polys(m.fast_floor(m.times_t(x))[0], n), e2, "%s: model x t, fast_floor vs oracle, %s" % (s.name, name))
            _eq(_polys(m.tail(x)[0], n), e3, "%s: model tail vs x t, oracle stages 2, 3, %s" % (s.name, name))
            self.tail[name] = (xin, zin, e2, e3)
        # the staged kernels 1 and 3 on words of their own as well (above they see what stages 0 and 2 produce); the m~ word of
        # stage 1 cycles through the preimages of the r targets
        cols = POLYS * n
        pre = [tg * pow(m.neg_inv_q_mt, -1, MT) % MT for tg in R_TARGETS]
        mtw = np.array([pre[c % 5] for c in range(cols)], dtype=object)[None, :]
        direct1 = {"random": _rand(rng, m.bsk, cols), "zero": np.zeros((nBsk, cols), dtype=object), "words_max": np.tile(m.bskc - 1, (1, cols))}
        for name, x in direct1.items():
            x = np.concatenate([x, mtw if name != "zero" else np.zeros((1, cols), dtype=object)])
            e = stage("sm_mrq", _polys(x, n), nBsk)
            out, im = m.sm_mrq(x)
            if name != "zero":
                assert all((im["r"][np.arange(cols) % 5 == k] == tg).all() for k, tg in enumerate(R_TARGETS))
            _eq(_polys(out, n), e, "%s: model sm_mrq vs oracle, %s" % (s.name, name))
            self.sm_mrq[name] = (_polys(x, n), e)
        for name, x in direct1.items():
            e = stage("fastbconv_sk", _polys(x, n), K)
            _eq(_polys(m.fastbconv_sk(x)[0], n), e, "%s: model fastbconv_sk vs oracle, %s" % (s.name, name))
            self.sk[name] = (_polys(x, n), e)


@functools.lru_cache(maxsize=None)
def expected(name, seed=0xBE42):
    return Expected(setup(name), seed)


# ---------------------------------------------------------------------------------------------------------------- the library
def run_stage(d, ci, which, x, out_comps):
    """x uint64 [polys][in_comps][N] -> [polys][out_comps][N]; the input must come back untouched"""
    polys, n = x.shape[0], x.shape[2]
    src, dst = S.DeviceBuffer.from_numpy(x), S.DeviceBuffer(polys * out_comps * n)
    S.rns_stage(d.ctx, ci, which, src, dst, polys)
    got = dst.to_numpy((polys, out_comps, n))
    assert np.array_equal(src.to_numpy(x.shape), x), "%s wrote to its input" % which
    return got


def case_model_vs_oracle(name):
    """the model against the oracle's stages on every pattern, and every steering target reached (CPU work only)"""
    expected(name)


def case_stages(name):
    """every pattern through the fused kernels and the staged ones"""
    s, e = setup(name), expected(name)
    K, nBsk = s.K, s.nBsk
    d, ci = s.device()
    assert d.ctx.base_bsk(ci) == s.bsk, "base Bsk"
    for pat, (x, e0, e1) in e.lift.items():
        what = "%s, %s: " % (name, pat)
        _eq(run_stage(d, ci, "lift", x, nBsk), e1, what + "lift")
        _eq(run_stage(d, ci, "fastbconv_m_tilde", x, nBsk + 1), e0, what + "fastbconv_m_tilde")
        _eq(run_stage(d, ci, "sm_mrq", e0, nBsk), e1, what + "sm_mrq")
    for pat, (x, z, e2, e3) in e.tail.items():
        what = "%s, %s: " % (name, pat)
        _eq(run_stage(d, ci, "floor_sk", x, K), e3, what + "floor_sk")
        _eq(run_stage(d, ci, "fast_floor", z, nBsk), e2, what + "fast_floor")
        _eq(run_stage(d, ci, "fastbconv_sk", e2, K), e3, what + "fastbconv_sk")
    for pat, (x, exp) in e.sm_mrq.items():
        _eq(run_stage(d, ci, "sm_mrq", x, nBsk), exp, "%s, %s: sm_mrq on its own words" % (name, pat))
    for pat, (x, exp) in e.sk.items():
        _eq(run_stage(d, ci, "fastbconv_sk", x, K), exp, "%s, %s: fastbconv_sk on its own words" % (name, pat))


def case_threshold(name):
    """the rule that gives B its extra prime (rns.cpp:605-632), on either side of its threshold: t one bit below the smallest bit
    count that adds the prime, and exactly at it"""
    n, bits, _, _ = CONFIGS[name]
    s = setup(name)
    K = s.K
    for t_bits, size in ((s.t_bits_threshold - 1, K + 1), (s.t_bits_threshold, K + 2)):
        t = plain_modulus_batching(n, t_bits)
        assert t.bit_length() == t_bits
        o = Oracle("bfv", n, s.primes, t)
        d = DeviceSide("bfv", n, s.primes, t)
        ci = d.chain_index_for_K(K)
        assert d.ctx.total_coeff_modulus_bit_count(ci) == s.total_bits
        got = d.ctx.base_bsk(ci)
        assert len(got) == size, "%s, t of %d bits: |Bsk| = %d, expected %d" % (name, t_bits, len(got), size)
        assert got == o.base_bsk(K), "%s, t of %d bits: base Bsk differs from the oracle's" % (name, t_bits)


def case_classes(name):
    """what the configuration is there for: its |B| and with it the dispatch classes of the two kernels"""
    s = setup(name)
    assert s.nBsk - 1 - s.K == CONFIGS[name][3], "%s: |B| = %d at K = %d" % (name, s.nBsk - 1, s.K)


def case_evaluator(name, batch=3, seed=0xE7A1):
    """multiply out of place and in place, and square, against the oracle's multiply"""
    _, bits, t_bits, _ = CONFIGS[name]
    n = 64
    K = len(bits)
    primes = coeff_modulus_create(n, list(bits) + [60])
    if t_bits is None:
        t_bits = _t_bits_threshold(primes, K)[0]
    t = plain_modulus_batching(n, t_bits)
    o = Oracle("bfv", n, primes, t)
    d = DeviceSide("bfv", n, primes, t)
    assert len(d.ctx.base_bsk(d.chain_index_for_K(K))) - 1 - K == CONFIGS[name][3]
    rng = np.random.default_rng(seed)
    xs = [rand_ct(rng, primes, K, n) for _ in range(batch)]
    ys = [rand_ct(rng, primes, K, n) for _ in range(batch)]
    exp = [o.multiply(x, y) for x, y in zip(xs, ys)]
    cx, cy = d.ct(xs), d.ct(ys)
    dest = S.Ciphertext(d.ctx, batch=batch)
    d.ev.multiply(cx, cy, dest)
    got, kept = d.out(dest), d.out(cx)
    for b in range(batch):
        _eq(got[b], exp[b], "%s: multiply out of place, item %d" % (name, b))
        _eq(kept[b], xs[b], "%s: multiply out of place left its operand alone, item %d" % (name, b))
    d.ev.multiply_inplace(cx, cy)
    got = d.out(cx)
    for b in range(batch):
        _eq(got[b], exp[b], "%s: multiply in place, item %d" % (name, b))
    d.ev.square_inplace(cy)
    got = d.out(cy)
    for b in range(batch):
        _eq(got[b], o.multiply(ys[b], ys[b]), "%s: square, item %d" % (name, b))


def case_evaluator_3x2(name="K05_mixed", batch=3, seed=0xE7A2):
    """size 3 times size 2: the general product on the auxiliary base, four polynomials an item into the tail"""
    n, bits, t_bits, _ = CONFIGS[name]
    K = len(bits)
    primes = coeff_modulus_create(n, list(bits) + [60])
    t = plain_modulus_batching(n, t_bits)
    o = Oracle("bfv", n, primes, t)
    d = DeviceSide("bfv", n, primes, t)
    rng = np.random.default_rng(seed)
    xs = [rand_ct(rng, primes, K, n, size=3) for _ in range(batch)]
    ys = [rand_ct(rng, primes, K, n, size=2) for _ in range(batch)]
    cx, cy = d.ct(xs), d.ct(ys)
    dest = S.Ciphertext(d.ctx, batch=batch)
    d.ev.multiply(cx, cy, dest)
    assert dest.size() == 4
    got = d.out(dest)
    for b in range(batch):
        _eq(got[b], o.multiply(xs[b], ys[b]), "size 3 x size 2, item %d" % b)


def case_stride(kernel):
    """more coefficients than the capped grid has threads: the second trip of the grid-stride loop, which uses the first trip's LDS
    slots again.  The input is the configuration's pattern slabs one after the other, over and over; so is the expected output."""
    s, e = setup(STRIDE[0]), expected(STRIDE[0])
    K, nBsk = s.K, s.nBsk
    d, ci = s.device()
    slabs = STRIDE_POLYS // POLYS
    assert STRIDE_POLYS * s.n > 2048 * 256 and slabs * POLYS == STRIDE_POLYS

    def tiled(parts):
        reps = -(-slabs // len(parts))
        return np.concatenate(list(parts) * reps)[:STRIDE_POLYS]

    lift, tail = list(e.lift.values()), list(e.tail.values())
    if kernel == "lift":
        _eq(run_stage(d, ci, "lift", tiled([v[0] for v in lift]), nBsk), tiled([v[2] for v in lift]), "lift, %d polynomials" % STRIDE_POLYS)
    elif kernel == "floor_sk":
        _eq(run_stage(d, ci, "floor_sk", tiled([v[0] for v in tail]), K), tiled([v[3] for v in tail]), "floor_sk, %d polynomials" % STRIDE_POLYS)
    else:
        assert kernel == "stage"
        e0, e1 = tiled([v[1] for v in lift]), tiled([v[2] for v in lift])
        e2, e3 = tiled([v[2] for v in tail]), tiled([v[3] for v in tail])
        _eq(run_stage(d, ci, "fastbconv_m_tilde", tiled([v[0] for v in lift]), nBsk + 1), e0, "fastbconv_m_tilde, %d polynomials" % STRIDE_POLYS)
        _eq(run_stage(d, ci, "sm_mrq", e0, nBsk), e1, "sm_mrq, %d polynomials" % STRIDE_POLYS)
        _eq(run_stage(d, ci, "fast_floor", tiled([v[1] for v in tail]), nBsk), e2, "fast_floor, %d polynomials" % STRIDE_POLYS)
        _eq(run_stage(d, ci, "fastbconv_sk", e2, K), e3, "fastbconv_sk, %d polynomials" % STRIDE_POLYS)
    del d
    S.release_pool()
