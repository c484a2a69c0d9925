"""Float64 reference, case table and mutants of the fused attention + Wo launch (attn_wo.h) as the
one-launch hook yalm_attn_wo_one runs it, shared by test_attn_wo_cpu.py (table, bar and mutants on the
CPU) and test_gpu_attn_wo_one.py (every case on the device). TEST INFRASTRUCTURE ONLY.

A launch: a = attention of q over the first kv_len cache rows (attn_ref.mha_ref, head_dim 128), then
out = (add_base ? x : 0) + W a with W the stored Wo decoded exactly (f16 as is, E5M2 by its bits, e4m3
code x the row's scale). Inputs follow attn_ref: K, V random normal f16, q 2 x random normal, the
planted "ends" / "last" keys, rows past the longest kv_len of the case poisoned with f16 NaN or +inf.
Wo is uniform at models.WEIGHT_SCALE rounded to the stored type (e4m3: rows at 1, 2, 4 x that in
turn, so that neighbouring rows carry different power-of-two scales), x standard normal.

The table, from the kernel's constants (64-key chunks, head mode up to 4 chunks, 16 Wo rows per
workgroup, Wo rows of 1 / 2 / 4 / 8 KiB):
  kernels   every (type, Wo row) the launcher instantiates, each with every G in {1, 2, 4, 8} that
            n_heads allows: every attn_wo_kernel<WT, GT, KB> runs
  dim       16 (one Wo workgroup), 48, 272 (17 workgroups), and dim == q_dim at the 1-KiB rows
  window    330 (6 chunks, the last partial): kv_len 1 .. 330 x S in 1 (head mode throughout; forced:
            the plan never gives 1 at this window), 2 (3 chunks per split at 330: the prefetch loop),
            3, 6 (one chunk per split; fewer live splits than S at 257) and 0 (the plan's own);
            64 with S 1; 4224 with S 32 at kv_len 2049 and 4224 (two kernels only)
  sequences kv_len 330, 257, 100, 321, 64, 330 over ONE set of buffers (key mode over all splits, fewer
            live splits, head mode, key mode again), S 6 and 2, layer 1 of 3, epoch0 1 and 1000
  forms     alias 1 + add_base 1 everywhere; alias 0 with add_base 1 and 0 once per (type, Wo row)
Every case is seeded by its name.

The bar of `out` (no new number: the attention's and the GEMV's bars propagated):
  bar_i = sum_j |W_ij| (X_ATOL + X_RTOL |a_j|) + REL_TOL max_i |ref_i|
computed in float64 from the reference's own a. F32_WORST: the f32 restatement (f32 attention, then
the kernel's two multiply-add chains per thread, its lanes, its waves) against float64, worst case per
type in units of that bar, as test_attn_wo_cpu.py measures it; DEVICE_WORST: the same for the device
(profiles/attn_wo_one_tests.txt). Both must stay below 1; the restatement below a fifth.
"""
import functools
import types
import zlib

import numpy as np

import attn_ref as A
from gemv_ref import REL_TOL
from yalm_amd import models as M

D = 128
RPW = 16  # attn_wo.h AWO_RPW
TYPES = {"f16": M.F16, "fp8": M.F8E5M2, "e4m3": M.E4M3}
BYTES = {"f16": 2, "fp8": 1, "e4m3": 1}
EPL = {"f16": 8, "fp8": 16, "e4m3": 16}  # elements of one 16-byte piece
KERNELS = [(t, kb) for t in ("f16", "fp8") for kb in (1, 2, 4, 8)] + [("e4m3", 4), ("e4m3", 8)]
GTS = (1, 2, 4, 8)
DIMS = (16, 48, 272)
KV_330 = A.WINDOWS[330]
S_330 = (1, 2, 3, 6, 0)
SEQ = (330, 257, 100, 321, 64, 330)
X_ATOL, X_RTOL = A.X_ATOL, A.X_RTOL
# worst |f32 restatement - float64| / bar per type (test_attn_wo_cpu.py prints and checks them)
# f16 at f16-1k-g2-d48-w330-s1-kv330-ends-nan-b1a1-l0of1-e1, fp8 at fp8-1k-g8-d16-w330-s0-kv321-last-inf-b1a1-l0of1-e1,
# e4m3 at launch 0 of e4m3-4k-g2-d272-w330-s6-seq-last-nan-b1a1-l1of3-e1: the bar is dominated by the attention's
# X_ATOL / X_RTOL carried through |W|, which an f32 attention uses a thousandth of
F32_WORST = {"f16": 0.00056, "fp8": 0.00037, "e4m3": 0.00016}
# worst |device - float64| / bar per type on an MI355X (profiles/attn_wo_one_tests.txt)
# (f16 and fp8 at the 1-KiB rows, e4m3 at both; the Wo half alone, at REL_TOL: 0.007 / 0.007 / 0.017 bars; the
# granules at X_ATOL / X_RTOL: 0.036 / 0.047 / 0.058)
DEVICE_WORST = {"f16": 0.00040, "fp8": 0.00033, "e4m3": 0.00013}


def n_heads_of(t, kb):
    return kb * 1024 // (D * BYTES[t])


class Case:
    __slots__ = ("name", "t", "kb", "G", "n_heads", "n_kv", "dim", "msl", "S", "forced", "kv", "flavour", "poison",
                 "add_base", "alias", "layer", "n_layers", "epoch0")

    def __init__(self, t, kb, G, dim, msl, S, kv, flavour, poison, add_base=1, alias=1, layer=0, n_layers=1, epoch0=1):
        self.t, self.kb, self.G, self.dim, self.msl, self.S = t, kb, G, dim, msl, S
        self.n_heads = n_heads_of(t, kb)
        self.n_kv = self.n_heads // G
        self.kv = tuple(kv)
        self.flavour, self.poison = flavour, poison
        self.add_base, self.alias, self.layer, self.n_layers, self.epoch0 = add_base, alias, layer, n_layers, epoch0
        # a split count yalm_attn_wo_plan gives at no slot count: one split where contexts exceed head mode
        self.forced = S == 1 and nchunks(msl) > A.HEAD_MAX
        kvs = "seq" if len(self.kv) > 1 else f"kv{self.kv[0]}"
        self.name = (f"{t}-{kb}k-g{G}-d{dim}-w{msl}-s{S}-{kvs}-{flavour}-{poison}-b{add_base}a{alias}"
                     f"-l{layer}of{n_layers}-e{epoch0}")

    @property
    def dtype(self):
        return TYPES[self.t]

    @property
    def q_dim(self):
        return self.n_heads * D

    def __repr__(self):
        return self.name


def nchunks(msl):
    return -(-msl // A.CHUNK)


def splits(c, S=None):
    """The key splits of the launch for a given S (0: the plan's at generous slots)."""
    S = c.S if S is None else S
    return min(S if S else A.SPLITS, nchunks(c.msl))


def mode_of(c, kv_len, S=None):
    S = splits(c, S)
    hmax = nchunks(c.msl) if S <= 1 else A.HEAD_MAX
    return "head" if -(-kv_len // A.CHUNK) <= hmax else "key"


def _table():
    out = []
    for ki, (t, kb) in enumerate(KERNELS):
        gs = [g for g in GTS if g <= n_heads_of(t, kb)]
        n = 0
        for kv in KV_330:
            for S in S_330:
                fl = A.FLAVOURS[(n + ki) % 2] if kv > A.CHUNK else "ends"
                po = ("nan", "inf")[(n // 2 + ki) % 2]
                out.append(Case(t, kb, gs[n % len(gs)], DIMS[(n // len(gs)) % 3], 330, S, [kv], fl, po))
                n += 1
        for g in gs:  # every G once more at the window of one chunk
            out.append(Case(t, kb, g, DIMS[g % 3], 64, 1, [(1, 64)[g % 2]], "ends", ("nan", "inf")[g % 2]))
        # the forms of a tensor-parallel rank: out a buffer of its own, with and without the base
        out.append(Case(t, kb, gs[-1], 48, 330, 6, [257], "last", "nan", add_base=1, alias=0))
        out.append(Case(t, kb, gs[0], 272, 330, 2, [330], "ends", "inf", add_base=0, alias=0))
        if kb == 1:
            out.append(Case(t, kb, gs[-1], n_heads_of(t, kb) * D, 330, 6, [321], "last", "inf"))
    out.append(Case("f16", 4, 4, 48, 4224, 32, [2049], "last", "nan"))
    out.append(Case("f16", 4, 4, 48, 4224, 32, [4224], "ends", "inf"))
    out.append(Case("fp8", 8, 2, 48, 4224, 32, [2049], "ends", "inf"))
    out.append(Case("fp8", 8, 2, 48, 4224, 32, [4224], "last", "nan"))
    for t, kb, g in (("f16", 4, 4), ("fp8", 8, 8), ("e4m3", 4, 2)):
        for S in (6, 2):
            for e0 in (1, 1000):
                out.append(Case(t, kb, g, 272, 330, S, SEQ, "last", "nan", layer=1, n_layers=3, epoch0=e0))
    return out


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
BY_KERNEL = {k: [c for c in CASES if (c.t, c.kb) == k] for k in KERNELS}


# ---------------------------------------------------------------- inputs
class Inputs:
    __slots__ = ("kb", "vb", "q", "x", "out0", "wo", "W", "codes", "rscale")


@functools.lru_cache(maxsize=3)
def inputs(name):
    """The case's arrays, read-only: kb, vb (msl * kv_dim) f16, q (n_launch, q_dim), x (n_launch, dim),
    out0 (n_launch, dim: what `out` holds before the launches when it is no alias), wo (the stored rows),
    W (dim, q_dim) float64 (the exact values), and for e4m3 the code values and the row scales."""
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n, nl, kv_dim = max(c.kv), len(c.kv), c.n_kv * D
    i = Inputs()
    K = np.empty((c.msl, kv_dim), np.float16)
    V = np.empty((c.msl, kv_dim), np.float16)
    K[:n] = rng.standard_normal((n, kv_dim)).astype(np.float16)
    V[:n] = rng.standard_normal((n, kv_dim)).astype(np.float16)
    q = (rng.standard_normal((nl, c.n_heads, D)) * 2).astype(np.float32)
    # attn_ref's planted keys, for the first launch's q and the case's longest kv_len
    sh = types.SimpleNamespace(head_dim=D, G=c.G, n_kv=c.n_kv)
    rest = np.zeros(c.n_heads)
    for g in range(c.n_kv):
        s = K[1:n - 1, g * D:(g + 1) * D].astype(np.float64) @ q[0, g * c.G:(g + 1) * c.G].astype(np.float64).T / np.sqrt(D)
        rest[g * c.G:(g + 1) * c.G] = np.exp(s).sum(axis=0)
    if n <= 2:
        s_last = np.ones(c.n_heads)
        s_first = s_last if c.flavour == "ends" else s_last - 3.0
    elif c.flavour == "ends":
        s_last = s_first = np.log(rest / 2)
    else:
        s_last = np.log(rest / (1.0 - np.exp(-3.0)))
        s_first = s_last - 3.0
    A._plant(K, q[0], sh, 0, s_first)
    if n > 1:
        A._plant(K, q[0], sh, n - 1, s_last)
    K.view(np.uint16)[n:] = A.POISONS[c.poison]
    V.view(np.uint16)[n:] = A.POISONS[c.poison]
    i.kb, i.vb, i.q = K.reshape(-1), V.reshape(-1), q.reshape(nl, -1)
    i.x = rng.standard_normal((nl, c.dim)).astype(np.float32)
    i.out0 = rng.standard_normal((nl, c.dim)).astype(np.float32)
    v = (rng.random((c.dim, c.q_dim)) * 2 - 1) * M.WEIGHT_SCALE
    i.codes = i.rscale = None
    if c.t == "e4m3":
        v *= np.array([1.0, 2.0, 4.0])[np.arange(c.dim) % 3][:, None]
        i.wo = M.e4m3_quantize(v)
        codes, s = M.e4m3_unpack(i.wo, c.q_dim)
        i.codes, i.rscale = M.e4m3_table()[codes].astype(np.float64), s.astype(np.float64)
        assert np.all(i.rscale[:-1] != i.rscale[1:]), "neighbouring e4m3 rows must differ in scale"
        i.W = i.codes * i.rscale[:, None]
    else:
        i.wo = M.encode_weights(v.astype(np.float32), c.dtype)
        i.W = M.decode_weights(i.wo, c.dtype).astype(np.float64).reshape(c.dim, c.q_dim)
    for k in Inputs.__slots__:
        a = getattr(i, k)
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return i


# ---------------------------------------------------------------- reference and bar
def attention(c, l, **kw):
    """mha_ref of launch l (q_dim float64); kw: mha_ref's mutant arguments."""
    i = inputs(c.name)
    return A.mha_ref(i.kb, i.vb, i.q[l], D, c.kv[l], c.msl, c.n_heads, c.n_kv, **kw)[0]


def wo_ref(c, l, a, W=None, base=None):
    """out of launch l in float64 from attention output a: (add_base ? x : 0) + W a."""
    i = inputs(c.name)
    base = c.add_base if base is None else base
    return (i.x[l].astype(np.float64) if base else 0.0) + (i.W if W is None else W) @ np.asarray(a, np.float64)


class Ref:
    __slots__ = ("a", "out", "bar")


@functools.lru_cache(maxsize=None)  # (a few KiB to a few hundred per case: computed once, shared by the tests)
def reference(name):
    """Per launch: a (q_dim), out (dim) and the bar (dim), float64, as (n_launch, .) arrays."""
    c = BY_NAME[name]
    i = inputs(name)
    r = Ref()
    r.a = np.stack([attention(c, l) for l in range(len(c.kv))])
    r.out = np.stack([wo_ref(c, l, r.a[l]) for l in range(len(c.kv))])
    r.bar = np.stack([np.abs(i.W) @ (X_ATOL + X_RTOL * np.abs(r.a[l])) + REL_TOL * np.abs(r.out[l]).max()
                      for l in range(len(c.kv))])
    for k in Ref.__slots__:
        getattr(r, k).setflags(write=False)
    return r


def in_bars(got, want, bar):
    """max |got - want| / bar over the elements; inf for a NaN."""
    e = np.abs(np.asarray(got, np.float64) - want) / bar
    return float("inf") if np.isnan(e).any() else float(e.max())


def gemv_bars(got, want):
    """The decode GEMV's measure: max error over max |ref| per output vector, in units of REL_TOL."""
    e = np.abs(np.asarray(got, np.float64) - want).max() / (REL_TOL * np.abs(want).max())
    return float("inf") if np.isnan(e) else float(e)


# ---------------------------------------------------------------- the f32 restatement
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def attention32(c, l):
    """Attention of launch l in float32 arithmetic (scores, exponentials, sums and the mix)."""
    i = inputs(c.name)
    n, kv_dim = c.kv[l], c.n_kv * D
    K = i.kb.reshape(-1, kv_dim)[:n].astype(np.float32)
    V = i.vb.reshape(-1, kv_dim)[:n].astype(np.float32)
    q = i.q[l].reshape(c.n_heads, D)
    out = np.zeros((c.n_heads, D), np.float32)
    for h in range(c.n_heads):
        g = h // c.G
        s = (K[:, g * D:(g + 1) * D] @ q[h]) / np.float32(np.sqrt(np.float32(D)))
        p = np.exp(s - s.max())
        out[h] = (p @ V[:, g * D:(g + 1) * D]) / p.sum(dtype=np.float32)
    return out.reshape(-1)


def wo32(c, l, a32):
    """The Wo half in f32 in the kernel's order: thread t of 256 (rows under 4 KiB: of the row's 256 / RPL)
    holds the 16-byte pieces t, t + 256, .. of a row and runs two multiply-add chains over them (even and
    odd elements); the two are added, then the lanes of a wave pairwise (32, 16, 8, 4, 2, 1 apart), then
    the row's waves in order; e4m3: times the row's scale; then the residual."""
    i = inputs(c.name)
    epl = EPL[c.t]
    W = (i.codes if c.t == "e4m3" else i.W).astype(np.float32)
    tpr = min(256, c.q_dim // epl)  # threads per row
    xs = c.q_dim // (tpr * epl)     # pieces per thread
    Wp = W.reshape(c.dim, xs, tpr, epl)
    ap = np.asarray(a32, np.float32).reshape(xs, tpr, epl)
    a0 = np.zeros((c.dim, tpr), np.float32)
    a1 = np.zeros((c.dim, tpr), np.float32)
    for k in range(xs):
        for e in range(0, epl, 2):
            a0 = _fma32(Wp[:, k, :, e], ap[None, k, :, e], a0)
            a1 = _fma32(Wp[:, k, :, e + 1], ap[None, k, :, e + 1], a1)
    v = (a0 + a1).reshape(c.dim, tpr // 64, 64)
    for step in (32, 16, 8, 4, 2, 1):
        v = v[:, :, :step] + v[:, :, step:2 * step]
    v = v[:, :, 0]
    s = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3]) if tpr == 256 else (v[:, 0] + v[:, 1] if tpr == 128 else v[:, 0])
    if c.t == "e4m3":
        s = s * i.rscale.astype(np.float32)
    return (i.x[l] + s if c.add_base else s).astype(np.float32)


def restatement32(c, l):
    return wo32(c, l, attention32(c, l))


# ---------------------------------------------------------------- mutants
MUTANTS = (
    "Wo rows r and r ^ 1 swapped",
    "two 256-column pieces of the input swapped",
    "the previous launch's attention output",
    "the base left out",
    "the base added",
    "the e4m3 scale of the neighbouring row",
    "one key split's chunks left out",
    "head h reads the next head's q",
)


def applies(m, c, l):
    """Whether mutant m changes launch l of case c at all."""
    if m == MUTANTS[1]:  # one kv head and one key: every head's output is the same V row
        return not (c.kv[l] == 1 and c.n_kv == 1)
    if m == MUTANTS[2]:
        return l > 0
    if m == MUTANTS[3]:
        return c.add_base == 1
    if m == MUTANTS[4]:
        return c.add_base == 0
    if m == MUTANTS[5]:
        return c.t == "e4m3"
    if m == MUTANTS[6]:  # key mode alone has splits; S 0: the plan's at generous slots
        return mode_of(c, c.kv[l]) == "key"
    if m == MUTANTS[7]:  # one key: the softmax is 1 whatever q is
        return c.kv[l] > 1
    return True


def mutant(m, c, l):
    """out of launch l (float64) with mutant m switched in."""
    i, r = inputs(c.name), reference(c.name)
    a = r.a[l]
    if m == MUTANTS[0]:
        return wo_ref(c, l, a, W=i.W[np.arange(c.dim) ^ 1])
    if m == MUTANTS[1]:  # the first and the last piece: other kv heads wherever there are two
        p = a.reshape(-1, 256).copy()
        p[[0, -1]] = p[[-1, 0]]
        return wo_ref(c, l, p.reshape(-1))
    if m == MUTANTS[2]:
        return wo_ref(c, l, r.a[l - 1])
    if m == MUTANTS[3]:
        return wo_ref(c, l, a, base=0)
    if m == MUTANTS[4]:
        return wo_ref(c, l, a, base=1)
    if m == MUTANTS[5]:
        return wo_ref(c, l, a, W=i.codes * i.rscale[np.arange(c.dim) ^ 1][:, None])
    if m == MUTANTS[6]:  # the split that holds the last live chunk and with it a planted key (a later launch
        # of a sequence has its own q and no planted key: split 0, a sixth of the keys or more)
        S, ns = splits(c), -(-c.kv[l] // A.CHUNK)
        s = (ns - 1) % S if l == 0 else 0
        drop = np.concatenate([np.arange(k * A.CHUNK, min((k + 1) * A.CHUNK, c.kv[l])) for k in range(s, ns, S)])
        return wo_ref(c, l, attention(c, l, drop=tuple(drop)))
    if m == MUTANTS[7]:
        return wo_ref(c, l, attention(c, l, q_of_head=A.next_head_in_group(c.G, c.n_heads)))
    raise KeyError(m)
