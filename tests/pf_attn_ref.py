"""Float64 reference, numpy model and case table of the batched prefill's causal attention
(csrc/prefill.h attn_prefill_kernel, reached through yalm_attn_prefill_rows), shared by
test_pf_attn_cpu.py (which checks the table, the model, the bars and the mutants on the CPU) and
test_gpu_prefill_attention.py (which runs every case on the device). TEST INFRASTRUCTURE ONLY.

The kernel: query blocks of AQ = 128 rows, 4 waves x 32 queries, KT = 64 keys per tile. With
qw0 the first query row of a wave, qmax_blk the last row of its block and key0 = 64 kt, its
integer decisions are
  diag   key0 + 63 > pos0 + qw0            the tile needs the causal mask
  skip   key0 <= pos0 + qw0 + 31           the wave has a query that sees the tile
  ntile  (pos0 + qmax_blk) / 64 + 1        tiles a block walks
  fetch  kt + 1 < ntile                    the next tile is staged during this one
  clamp  min(key0 + r, pos0 + T - 1)       staged rows never pass the last valid cache row

The (T, pos0) pairs and the side of each decision they sit on by exactly one key (asserted by
test_pf_attn_cpu.py::test_edges_are_covered from the integers alone, over the waves that hold
a query and the tiles their block walks):
  diag   true by one  (key0 + 63 == pos0 + qw0 + 1): (129, 62) wave 0; (97, 30) wave 1
         false by one (key0 + 63 == pos0 + qw0):     (65, 63) wave 0; (33, 31) wave 1
  skip   true by one  (key0 == pos0 + qw0 + 31):     (130, 33) wave 0; (129, 1) wave 1
         false by one (key0 == pos0 + qw0 + 32):     (128, 0) wave 1; (257, 0)
  ntile  true by one  (the last tile holds one key, pos0 + qmax_blk = 0 mod 64): (1, 0), (1, 64)
         false by one (one more key would open a tile, = 63 mod 64): (1, 63), (32, 32), (33, 31)
  fetch  true by one  (the last staged-ahead tile is needed for one key): (1, 64), (129, 1)
         false by one (the tile not staged would start one key past the block's last): (65, 63),
                      (128, 0) block 0
  clamp  true by one  (one staged row is clamped, pos0 + T = 63 mod 64): (97, 30), (129, 62)
         false by one (the last tile ends on the last valid row, = 0 mod 64): (1, 63), (64, 0)
The other pairs: (257, 0) three query blocks (dispatched in reverse) whose last holds one row
and three idle waves; (129, 1), (129, 62) an idle-wave tail block; (200, 64) two blocks, pos0 + T
= 8 mod 64; (40, 600) and (64, 1100) 10 and 18 key tiles behind one block.

n_kv = 2 (the group index matters) except one n_kv = 1 case; G = n_heads / n_kv is spread over
the pairs (1, 3, 4, 8). Every pair runs at head_dim 64 and 128, in the fast and the split form
(q and o rows as f16 [hi | lo]), in five flavours. The cache has 70 rows past pos0 + T, all f16
NaN or +inf (alternating along the table); o has two guard rows of a sentinel bit pattern past
row T and NaN bits in the rows the kernel has to write.

Flavours. q = 0.5 x normal with its component along a unit vector u (one per kv head) replaced
by BETA, K[t] = normal + a_t sqrt(D) / BETA u, V = normal: the score of key t is a_t plus noise
of about 0.6 nats for every query.
  flat   a = 0, q and K plain standard normal: the data of test_gpu_prefill.py::test_attn_prefill.
         After tile 0 the running max never grows by 8 log2 units: no rescale.
  ramp   a_t = 0.5 t: the last visible key holds about 40 % of the mass at every row, and the
         max grows 46 log2 units per tile: a rescale on every tile with 32 keys in it.
  slow   a_t = 0.08 t: 7.4 log2 units per tile. A tile is mostly kept on the stale max (P up to
         2^8) and the next one rescales: both sides of the decision with a non-zero o.
  sink   a_0 = ln(n / 2), n = pos0 + T: key 0 keeps a large share at every row, so tile 0's
         contribution has to survive every later tile.
  step   a_t = 6 ln 2 on odd tiles and + 12 ln 2 on the last key: steps of +6 and -6 log2 units
         (no rescale, P up to 2^6 and down to 2^-6) and one of at least +12 (a rescale) for the
         wave that holds the last row. (The last key alone, and 12 not 9: 9 less the noise of a
         tile's largest score does not reach 8 reliably.)
Rescale counts asserted on the model: 0 for flat; above 0 for ramp from 96 keys, for slow from
160 keys (growth past 8 since tile 0), for step from 65 keys; stale tiles whose max grew above
0 for slow and step from 128 keys.

The model (model()) restates the kernel's arithmetic per wave and tile: every MFMA k-step adds
an exact 16-term partial sum to its f32 accumulator, the stale-max rule as written, exp2 and l in
f32 from the unrounded p, P as f16 (split: f16 hi + lo), o in f32, output f16 (split: hi + lo).
flush=True drops f16 subnormals among the MFMA inputs.

Bars. Fast, per element: |o - o64| <= 2^-10 A + 2^-11 |o64| + 1e-7, A = p @ |V| (P rounded to
f16: 2^-11 A, doubled for the f32 sum order and the 1-ulp hardware exp2; the output's f16
rounding: 2^-11 |o|). The split bar is SPLIT_UNITS x (fast bar / 1024): four times the worst
value the subnormals-kept model reaches against float64 over the whole table, measured on the
CPU by test_pf_attn_cpu.py::test_model_is_inside_the_bars, which asserts SPLIT_UNITS is that:
  measured worst 70.2 units (ramp at pos0 1100, head_dim 128: f32 scores near 6500 and 140 f32
  rescales of l and o; flat stays under 2, slow under 9, sink under 10, step under 18), so
  SPLIT_UNITS = 280.8: the split bar is 0.274 of the fast bar. The flush variant of the model is
  between 30 and 47 000 units wherever more than one key is visible, and above the bar on 50 of
  the 160 split cases (every ramp case and most step cases): the device run tells the two apart.
"""
import functools
import zlib

import numpy as np

AQ, KT, WQ = 128, 64, 32  # prefill.h: queries per block, keys per tile, queries per wave
RESCALE_LOG2 = 8.0
BETA = 4.0
TAIL, GUARDS = 70, 2
POISONS = (0x7E00, 0x7C00)  # f16 NaN, +inf
SENTINEL, UNWRITTEN = 0xBEEF, 0x7E00
HEAD_DIMS = (64, 128)
FORMS = ("fast", "split")
FLAVOURS = ("flat", "ramp", "slow", "sink", "step")
# (T, pos0, G, n_kv)
PAIRS = (
    (1, 0, 1, 2), (1, 63, 3, 2), (1, 64, 4, 2),
    (32, 32, 8, 2), (33, 31, 1, 2), (64, 0, 3, 2),
    (65, 63, 4, 2), (97, 30, 8, 2), (130, 33, 1, 2), (129, 62, 3, 2),
    (128, 0, 4, 2), (129, 1, 4, 1), (257, 0, 8, 2), (200, 64, 1, 2),
    (40, 600, 3, 2), (64, 1100, 8, 2),
)
# the split bar in units of fast bar / 1024: 4 x the worst value of the subnormals-kept model
MEASURED_SPLIT_WORST = 70.2  # d128-split-ramp-T64-p1100-g8x2; the bound on every case, see the docstring
SPLIT_UNITS = 4.0 * MEASURED_SPLIT_WORST


class Case:
    __slots__ = ("name", "T", "pos0", "G", "n_kv", "n_heads", "head_dim", "form", "flavour", "poison", "split")

    def __init__(self, T, pos0, G, n_kv, head_dim, form, flavour, poison):
        self.T, self.pos0, self.G, self.n_kv, self.n_heads = T, pos0, G, n_kv, G * n_kv
        self.head_dim, self.form, self.flavour, self.poison = head_dim, form, flavour, poison
        self.split = form == "split"
        self.name = f"d{head_dim}-{form}-{flavour}-T{T}-p{pos0}-g{G}x{n_kv}"

    def __repr__(self):
        return self.name


def _table():
    out = []
    for d in HEAD_DIMS:
        for form in FORMS:
            for fl in FLAVOURS:
                for T, pos0, G, n_kv in PAIRS:
                    out.append(Case(T, pos0, G, n_kv, d, form, fl, POISONS[len(out) % 2]))
    return out


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
GROUPS = {k: [c for c in CASES if (c.head_dim, c.form, c.flavour) == k]
          for k in [(d, f, fl) for d in HEAD_DIMS for f in FORMS for fl in FLAVOURS]}


# ------------------------------------------------------------------ the integer edges
def waves(T, pos0):
    """(qb, qw0, ntile) of every wave that holds a query row, in block order."""
    out = []
    for qb in range(-(-T // AQ)):
        qmax_blk = min(qb * AQ + AQ, T) - 1
        ntile = (pos0 + qmax_blk) // KT + 1
        out += [(qb, qb * AQ + w * WQ, ntile) for w in range(AQ // WQ) if qb * AQ + w * WQ < T]
    return out


def edges(T, pos0):
    """The set of (condition, side) the pair sits on by exactly one key (module docstring)."""
    got = set()
    kv_rows = pos0 + T
    for qb, qw0, ntile in waves(T, pos0):
        qmax_blk = min(qb * AQ + AQ, T) - 1
        if (pos0 + qmax_blk) % KT in (0, KT - 1):
            got.add(("ntile", (pos0 + qmax_blk) % KT == 0))
        for kt in range(ntile):
            key0 = kt * KT
            d = key0 + KT - 1 - (pos0 + qw0)  # diag: d > 0
            if d in (0, 1):
                got.add(("diag", d == 1))
            d = pos0 + qw0 + 31 - key0  # skip: d >= 0
            if d in (-1, 0):
                got.add(("skip", d == 0))
            if kt + 1 < ntile and kt + 2 == ntile and key0 + KT == pos0 + qmax_blk:
                got.add(("fetch", True))
            if kt + 1 == ntile and key0 + KT == pos0 + qmax_blk + 1:
                got.add(("fetch", False))
            d = key0 + KT - 1 - (kv_rows - 1)  # clamp: rows of the staged tile past the last valid one
            if d in (0, 1):
                got.add(("clamp", d == 1))
    return got


# ------------------------------------------------------------------ inputs
def _f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16)


def _hi_lo(x32):
    hi = _f16(x32)
    with np.errstate(invalid="ignore"):  # a mutant's inf - inf
        return hi, _f16(x32 - hi.astype(np.float32))


def scores_a(c):
    """a_t of the case's flavour for keys 0 .. pos0 + T - 1."""
    n = c.pos0 + c.T
    t = np.arange(n, dtype=np.float64)
    if c.flavour == "ramp":
        return 0.5 * t
    if c.flavour == "slow":
        return 0.08 * t
    a = np.zeros(n)
    if c.flavour == "sink":
        a[0] = np.log(max(n, 4) / 2)
    if c.flavour == "step":
        a[(np.arange(n) // KT) % 2 == 1] = 6 * np.log(2)
        a[-1] += 12 * np.log(2)
    return a


@functools.lru_cache(maxsize=8)
def inputs(name):
    """(q (T, W) f16, kc, vc (pos0 + T + TAIL, n_kv D) f16, o_init (T + GUARDS, W) f16); read-only."""
    c = BY_NAME[name]
    D, T, n = c.head_dim, c.T, c.pos0 + c.T
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    K = rng.standard_normal((n, c.n_kv, D))
    V = rng.standard_normal((n, c.n_kv, D))
    q = rng.standard_normal((T, c.n_heads, D))
    if c.flavour != "flat":
        u = rng.standard_normal((c.n_kv, D))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        uh = np.repeat(u, c.G, axis=0)  # per q head
        q *= 0.5
        q += (BETA - np.sum(q * uh, axis=2, keepdims=True)) * uh
        K += (scores_a(c) * np.sqrt(D) / BETA)[:, None, None] * u
    assert np.abs(K).max() < 4096.0, name  # far inside the f16 range
    kc = np.empty((n + TAIL, c.n_kv * D), np.float16)
    vc = np.empty_like(kc)
    kc[:n], vc[:n] = _f16(K.reshape(n, -1)), _f16(V.reshape(n, -1))
    kc.view(np.uint16)[n:] = c.poison
    vc.view(np.uint16)[n:] = c.poison
    q32 = q.reshape(T, -1).astype(np.float32)
    qq = np.concatenate(_hi_lo(q32), axis=1) if c.split else _f16(q32)
    o_init = np.empty((T + GUARDS, qq.shape[1]), np.float16)
    o_init.view(np.uint16)[:T] = UNWRITTEN
    o_init.view(np.uint16)[T:] = SENTINEL
    for a in (qq, kc, vc, o_init):
        a.setflags(write=False)
    return qq, kc, vc, o_init


def q_parts(c, q):
    """(hi, lo or None) of the q rows as float64 (T, n_heads, D)."""
    qd = c.n_heads * c.head_dim
    f = lambda a: a.astype(np.float64).reshape(c.T, c.n_heads, c.head_dim)
    return (f(q[:, :qd]), f(q[:, qd:])) if c.split else (f(q), None)


def out_value(c, o):
    """Rows < T of a kernel / model output as float64 (T, q_dim): hi + lo for the split form."""
    qd = c.n_heads * c.head_dim
    o = np.asarray(o)[:c.T].astype(np.float64)
    return o[:, :qd] + o[:, qd:] if c.split else o


# ------------------------------------------------------------------ float64 reference
def causal(c):
    """vis[r][t]: key t <= pos0 + r."""
    return np.arange(c.pos0 + c.T)[None, :] <= (c.pos0 + np.arange(c.T))[:, None]


def attn_f64(c, q, kc, vc, vis=None, kv_of_head=None, q_of_head=None, v_of_key=None):
    """(o, A), float64 (T, q_dim): causal GQA attention per (row, head) over keys 0 .. pos0 + row,
    head h reading kv head h // G; A = p @ |V|. It reads the f16 K / V values exactly and, for the
    split form, hi + lo of q. The mutants: vis, a boolean (T, pos0 + T) visibility matrix (a row
    that sees no key gives 0); kv_of_head, q_of_head, maps head -> kv head / head whose q it
    uses; v_of_key, the V row that key t's probability multiplies."""
    D, T, n = c.head_dim, c.T, c.pos0 + c.T
    K = np.asarray(kc)[:n].astype(np.float64).reshape(n, c.n_kv, D)
    V = np.asarray(vc)[:n].astype(np.float64).reshape(n, c.n_kv, D)
    if v_of_key is not None:
        V = V[np.asarray(v_of_key)]
    hi, lo = q_parts(c, q)
    qv = hi if lo is None else hi + lo
    vis = causal(c) if vis is None else vis
    seen = vis.any(axis=1)
    o = np.zeros((T, c.n_heads, D))
    A = np.zeros_like(o)
    for h in range(c.n_heads):
        g = h // c.G if kv_of_head is None else kv_of_head(h)
        s = qv[:, h if q_of_head is None else q_of_head(h)] @ K[:, g].T / np.sqrt(D)
        s = np.where(vis, s, -np.inf)
        s[~seen] = 0.0
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        p[~seen] = 0.0
        o[:, h], A[:, h] = p @ V[:, g], p @ np.abs(V[:, g])
    return o.reshape(T, -1), A.reshape(T, -1)


@functools.lru_cache(maxsize=8)
def reference(name):
    c = BY_NAME[name]
    q, kc, vc, _ = inputs(name)
    o, A = attn_f64(c, q, kc, vc)
    o.setflags(write=False)
    A.setflags(write=False)
    return o, A


def fast_bar(o64, A):
    return 2.0 ** -10 * A + 2.0 ** -11 * np.abs(o64) + 1e-7


def bar_of(c, o64, A):
    return fast_bar(o64, A) * (SPLIT_UNITS / 1024.0 if c.split else 1.0)


def in_bars(got, o64, bar):
    """max |got - o64| / bar; inf where got is not finite."""
    got = np.asarray(got, np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got - o64) / bar))


# ------------------------------------------------------------------ model of the kernel
def _flush(x16):
    """f16 subnormals -> 0 (as float64)."""
    x = x16.astype(np.float64)
    return np.where(np.abs(x) < 2.0 ** -14, 0.0, x)


def _acc(acc32, part64):
    """One MFMA k-step: the exact 16-term partial sum added to the f32 accumulator."""
    return (acc32.astype(np.float64) + part64).astype(np.float32)


def model(c, q, kc, vc, flush=False, mutant=None):
    """(o (T, W) f16, stats) of the kernel's arithmetic on the case's inputs. stats: "rescales",
    the (wave, head, tile > 0) count of rescale branches taken; "stale", the count of tiles > 0
    kept on the old max although some query's max grew; "pmax", the largest P.
    mutant "l_only": alpha scales l but not o; "stale": after tile 0 the max is never replaced."""
    D, T, pos0, H = c.head_dim, c.T, c.pos0, c.n_heads
    f32 = np.float32
    kv_rows = pos0 + T
    inp = _flush if flush else (lambda a: a.astype(np.float64))
    K = inp(np.asarray(kc)[:kv_rows]).reshape(kv_rows, c.n_kv, D)
    V = inp(np.asarray(vc)[:kv_rows]).reshape(kv_rows, c.n_kv, D)
    qd = H * D
    q = np.asarray(q)
    qh = inp(q[:, :qd]).reshape(T, H, D)
    ql = inp(q[:, qd:]).reshape(T, H, D) if c.split else None
    kvh = np.arange(H) // c.G
    sl2 = f32(1.4426950408889634) / np.sqrt(f32(D))
    out = np.zeros((T, H, D), f32)
    stats = {"rescales": 0, "stale": 0, "pmax": 0.0}
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for qb, qw0, ntile in waves(T, pos0):
            rows = np.minimum(qw0 + np.arange(WQ), T - 1)
            qpos = pos0 + qw0 + np.arange(WQ)
            Qh = qh[rows].transpose(1, 0, 2)  # (H, 32, D)
            Ql = ql[rows].transpose(1, 0, 2) if c.split else None
            o = np.zeros((H, WQ, D), f32)
            m = np.full((H, WQ), -np.finfo(f32).max, f32)
            l = np.zeros((H, WQ), f32)
            for kt in range(ntile):
                key0 = kt * KT
                if not key0 <= pos0 + qw0 + 31:
                    continue
                keys = key0 + np.arange(KT)
                kr = np.minimum(keys, kv_rows - 1)
                Kt = K[kr][:, kvh].transpose(1, 2, 0)  # (H, D, 64)
                Vt = V[kr][:, kvh].transpose(1, 0, 2)  # (H, 64, D)
                st = np.zeros((H, WQ, KT), f32)
                for s in range(0, D, 16):
                    st = _acc(st, Qh[:, :, s:s + 16] @ Kt[:, s:s + 16])
                    if c.split:
                        st = _acc(st, Ql[:, :, s:s + 16] @ Kt[:, s:s + 16])
                if key0 + KT - 1 > pos0 + qw0:
                    st[:, keys[None, :] > qpos[:, None]] = -np.inf
                mx = st.max(axis=2) * sl2
                fire = ~np.all(mx - m <= f32(RESCALE_LOG2), axis=1)  # per head: one wave each
                if mutant == "stale" and kt > 0:
                    fire[:] = False
                if kt > 0:
                    stats["rescales"] += int(fire.sum())
                    stats["stale"] += int((~fire & np.any(mx > m, axis=1)).sum())
                mn = np.maximum(m, mx)
                alpha = np.where(fire[:, None], np.exp2(m - mn), f32(1.0)).astype(f32)
                m = np.where(fire[:, None], mn, m)
                l = l * alpha
                if mutant != "l_only":
                    o = o * alpha[:, :, None]
                p = np.exp2((st.astype(np.float64) * np.float64(sl2) - m[:, :, None]).astype(f32))
                stats["pmax"] = max(stats["pmax"], float(p.max()))
                l = l + p.sum(axis=2, dtype=f32)
                ph = _f16(p)
                parts = [ph]
                if c.split:
                    parts.append(_f16(p - ph.astype(f32)))
                parts = [inp(x) for x in parts]
                for k in range(0, KT, 16):
                    for x in parts:
                        o = _acc(o, x[:, :, k:k + 16] @ Vt[:, k:k + 16])
            v = o * (f32(1.0) / l)[:, :, None]
            real = qw0 + np.arange(WQ) < T
            out[rows[real]] = v.transpose(1, 0, 2)[real]
    v = out.reshape(T, qd)
    hi, lo = _hi_lo(v)
    return (np.concatenate([hi, lo], axis=1) if c.split else hi), stats


# ------------------------------------------------------------------ the mutants
def _wave_of_rows(c):
    """Per row: (qw0, ntile) of its wave."""
    qw0 = np.empty(c.T, np.int64)
    nt = np.empty(c.T, np.int64)
    for _, w0, ntile in waves(c.T, c.pos0):
        qw0[w0:w0 + WQ], nt[w0:w0 + WQ] = w0, ntile
    return qw0, nt


def reference_mutants(c):
    """name -> keyword arguments of attn_f64 for the case, or None where the mutant changes
    nothing there. The numbers are those of the list in test_pf_attn_cpu.py."""
    T, pos0, n = c.T, c.pos0, c.pos0 + c.T
    vis0 = causal(c)
    keys = np.arange(n)[None, :]
    qpos = (pos0 + np.arange(T))[:, None]
    qw0, nt = _wave_of_rows(c)
    qw0, nt = qw0[:, None], nt[:, None]
    out = {}

    def vis(name, v):
        out[name] = {"vis": v} if (v != vis0).any() else None

    vis("1 key qpos + 1 visible at qpos % 64 == 63", vis0 | ((keys == qpos + 1) & (qpos % KT == KT - 1)))
    vis("2 own key invisible at qpos % 64 == 0", vis0 & ~((keys == qpos) & (qpos % KT == 0) & (qpos > 0)))
    k3 = pos0 + qw0 + 31  # the wave's tile at key0 == pos0 + qw0 + 31 is skipped
    vis("3 tile at key0 == pos0 + qw0 + 31 skipped", vis0 & ~((k3 % KT == 0) & (keys >= k3)))
    last = np.array([pos0 + min((r // AQ) * AQ + AQ, T) - 1 for r in range(T)])[:, None]
    vis("4 last tile dropped at pos0 + qmax_blk % 64 == 0", vis0 & ~((last % KT == 0) & (keys >= last)))
    vis("5 key 0 dropped past the first tile", vis0 & ~((keys == 0) & (qpos >= KT)))
    vis("6 one key per tile dropped", vis0 & ~(keys % KT == 17))
    blk0 = (np.arange(T)[:, None] // AQ) * AQ  # the block before's last row is blk0 - 1
    prev = np.where(blk0 > 0, (pos0 + blk0 - 1) // KT + 1, nt)
    vis("12 tile count of the block before", vis0 & (keys < prev * KT))
    swap = np.arange(n)
    for a in range(5, n - 4, 32):  # keys 32 b + 5 and 32 b + 9: two registers of one lane half
        swap[a], swap[a + 4] = a + 4, a
    out["7 two keys of a 32-key block swapped on the V side"] = {"v_of_key": swap} if n > 9 else None
    out["8 head h reads kv head (h / G + 1) % n_kv"] = (
        {"kv_of_head": lambda h: (h // c.G + 1) % c.n_kv} if c.n_kv > 1 else None)
    if c.G > 1:
        out["9 head h reads the q of head h + 1 of its group"] = {
            "q_of_head": lambda h: (h // c.G) * c.G + (h % c.G + 1) % c.G}
    else:  # a group of one head has no other: wrap over all the heads
        out["9 head h reads the q of head h + 1 of its group"] = {"q_of_head": lambda h: (h + 1) % c.n_heads}
    return out


MODEL_MUTANTS = {"10 l rescaled by alpha but not o": "l_only", "11 the stale max kept past 2^8": "stale"}
