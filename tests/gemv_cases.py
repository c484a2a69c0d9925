"""The case table of the single-row (decode) GEMV tests (gemv_rb_kernel and gemv_kernel through
yalm_gemv_one), shared by test_gemv_cpu.py and test_gpu_gemv.py. TEST INFRASTRUCTURE ONLY; needs
no library.

A case names the weight type, the epilogue policy, the shape, the launch geometry it asks for
(threads, unroll, workgroups per CU, CUs, whole-row mode allowed or not) and the path it is there
for, as conditions (`want`) on the facts of its launch plan (`facts`). Every case pins its CU count,
so the facts are the same on any device: 256, or 1 / 2 where a workgroup has to hold more groups
than it has threads, where the grid has to be smaller than the sink pairs, or where whole rows of
several chunks are wanted without megabytes of them (whole-row mode needs 2 W rows per workgroup in
every workgroup; at 256 CUs that is 2048 rows and more).

Chunks: CH = 64 lanes x EPL elements = 256 (f32), 512 (f16), 1024 (E5M2, e4m3), 2048 (q4); a chunk is
1 KiB of weights but for q4 (1 KiB of nibbles and 128 B of scales). A row that is a whole number of
chunks takes the row-block kernel, any other the generic one. R: rows per group (2 for store2, glu,
qkv*: a w1 | w3 pair, a RoPE pair).

The facts (row-block kernel; W = threads / 64 waves, nch = n / CH, nb workgroups, workgroup b holds
ngl groups = ngl R virtual rows = ngl R nch items, wave w of it `mine` of them):
  generic     the generic kernel
  threads, U, wpc   as launched
  nch         chunks per row
  rows        whole-row mode
  rows_off    the shape qualifies for whole-row mode and the case forbids it (rows = 0)
  rows_miss   a whole-row policy misses exactly one entry condition: "nb" (n_groups % nb), "w"
              ((ngl R) % W), "2w" (ngl R < 2 W)
  uneven      n_groups % nb != 0: workgroups differ in ngl
  capped      n_groups < cus wpc: nb = n_groups
  multistep   chunk order, W >= 2 nch and a wave with two items: advance steps more than one row
  idle        a wave with no item
  mine_lt_U   a wave with 0 < mine < U (the dummy refills from its first step)
  mine_mod_U  a wave with mine > U and mine % U != 0 (a last step with dummy refills and dead slots)
  flush       a wave that takes items of more than one row (the cvr != cur flush)
  cursor_row, cursor_chunk   a wave with items that starts past row 0 / past chunk 0
  xregs       x (and the norm weights) loaded ahead of the weight stream
  xcap        "at": n is the xregs capacity 4 xpre_n threads; "above": one chunk more; else None
  xclamp      xregs with n below the capacity: clamped n - 4 loads, guarded stores and norm sum
  lds_big     dynamic LDS above 64 KiB
  epi_loop    ngl > threads: the epilogue loop runs again (finish_all / the loaded row scale)
generic kernel (256 threads, one group per wave, U = 4):
  uloop, tail, ragged   the U = 4 loop runs; 1..3 whole chunks follow it; the row ends in a chunk
  past        a wave past n_groups
  q4_partial  q4 with n no multiple of 2048: the last x block is staged partly
QKV policies (from the case itself):
  head_dim, heads (q heads, kv heads), kv_sink, kv_pos ("0", "1", "2", "last", or the number), clip,
  rotary_partial (table entries (1, 0) past rotary_dim < head_dim), late_loops (threads nb <
  kv_sink kv_dim / 2: late's loop runs again and loads its own pairs)."""
F32, F16, F8, Q4, E4M3 = 0, 1, 3, 16, 17  # yalm_amd.models
DTYPES = (F32, F16, F8, Q4, E4M3)
DTYPE_NAMES = {F32: "f32", F16: "f16", F8: "fp8", Q4: "q4", E4M3: "e4m3"}
EPL = {F32: 4, F16: 8, F8: 16, Q4: 32, E4M3: 16}
CH = {t: 64 * e for t, e in EPL.items()}
STORE1, STORE2, RESIDUAL, ADDTO, GLU, QKV, QKVB, QKVN = range(8)  # yalm_gemv_one policies
POLICY_NAMES = ("store1", "store2", "residual", "addto", "glu", "qkv", "qkvb", "qkvn")
FAMILIES = {"store": (STORE1, STORE2), "residual": (RESIDUAL, ADDTO), "glu": (GLU,), "qkv": (QKV, QKVB, QKVN)}
POLICY_R = (1, 2, 1, 1, 2, 2, 2, 2)
ROWS_POLICIES = (RESIDUAL, GLU, QKV, QKVB, QKVN)  # gemv.h ROWS_MODE
QKV_POLICIES = (QKV, QKVB, QKVN)
GK_QKV, GK_WO, GK_GLU, GK_W2, GK_CLS = range(5)
GELU, SILU = 0, 1
PLAN_CUS = 256
GENERIC_THREADS, GENERIC_U = 256, 4
KV_SINKS = 2  # gemv.h PQKV::KV_SINKS

# yalm_hip.hip default_rb_cfg: {threads, U, workgroups per CU} per kind (QKV, Wo, W1|W3, W2, logits)
DEFAULT_CFG = {
    "q4": ((512, 2, 1), (512, 4, 1), (512, 2, 2), (512, 2, 1), (512, 4, 3)),
    "narrow": ((512, 4, 1), (512, 2, 2), (512, 4, 1), (512, 4, 1), (512, 2, 2)),
    "wide": ((512, 4, 1), (1024, 2, 2), (512, 4, 1), (1024, 2, 1), (512, 4, 4)),
}


def default_cfg(dtype, kind):
    return DEFAULT_CFG["q4" if dtype == Q4 else "narrow" if dtype in (F8, E4M3) else "wide"][kind]


def xpre_n(norm, threads):
    """gemv.h xpre_n: float4s of x a thread holds ahead of the weight stream."""
    return 2 if norm else (7 if threads == 512 else 4)


def xcap(norm, threads):
    return 4 * xpre_n(norm, threads) * threads


def xs_len(dtype, n):
    """gemv.h xs_len: floats of LDS x occupies."""
    return (n + 2047) & ~2047 if dtype == Q4 else (n + 3) & ~3


def plan(dtype, policy, kind, n, n_groups, norm=False, threads=0, unroll=0, wpc=0, cus=PLAN_CUS, rows=-1):
    """yalm_gemv_plan restated (test_gemv_cpu.py holds the library's function to it)."""
    R = POLICY_R[policy]
    if n % CH[dtype]:
        W = GENERIC_THREADS // 64
        nb = -(-n_groups // W)
        return dict(generic=1, threads=GENERIC_THREADS, unroll=GENERIC_U, nb=nb, rows=0, ngl_min=n_groups - (nb - 1) * W,
                    ngl_max=min(n_groups, W), xregs=0, lds=xs_len(dtype, n) * 4 + 256)
    dt, du, dw = default_cfg(dtype, kind)
    threads, unroll, wpc = threads or dt, unroll or du, wpc or dw
    threads = threads if threads in (256, 1024) else 512
    unroll = unroll if unroll in (2, 8) else 4
    W = threads // 64
    nb = max(1, min(n_groups, cus * max(1, wpc)))
    ngl = -(-n_groups // nb)
    whole = (policy in ROWS_POLICIES and rows != 0 and n_groups % nb == 0 and (ngl * R) % W == 0
             and ngl * R >= 2 * W)
    return dict(generic=0, threads=threads, unroll=unroll, nb=nb, rows=int(whole), ngl_min=n_groups // nb, ngl_max=ngl,
                xregs=int(n <= xcap(norm, threads)), lds=(xs_len(dtype, n) + 64 + ngl * R * W) * 4)


class Case:
    __slots__ = ("name", "dtype", "policy", "kind", "n", "d", "norm", "act", "threads", "unroll", "wpc", "cus",
                 "rows", "n_heads", "n_kv_heads", "head_dim", "kv_sink", "kv_pos", "cache_rows", "clip", "rotary",
                 "want")

    def __init__(self, dtype, policy, n, d=0, geo=(512, 4, 1), want=(), norm=False, act=SILU, cus=PLAN_CUS, rows=-1,
                 qkv=None, tag=""):
        self.dtype, self.policy, self.n, self.d, self.norm, self.act = dtype, policy, n, d, norm, act
        self.threads, self.unroll, self.wpc = geo
        self.cus, self.rows = cus, rows
        self.kind = {STORE1: GK_CLS, STORE2: GK_CLS, RESIDUAL: GK_W2, ADDTO: GK_WO, GLU: GK_GLU}.get(policy, GK_QKV)
        self.n_heads = self.n_kv_heads = self.head_dim = self.kv_sink = self.kv_pos = self.cache_rows = 0
        self.clip, self.rotary = False, 0
        shape = f"d{d}"
        if policy in QKV_POLICIES:
            q = dict(kv_sink=0, kv_pos=0, cache_rows=3, clip=False, rotary=0)
            q.update(qkv)
            for k, v in q.items():
                setattr(self, k, v)
            self.rotary = self.rotary or self.head_dim
            assert self.kv_sink <= self.kv_pos < self.cache_rows and self.cache_rows >= 2
            shape = (f"h{self.n_heads}x{self.n_kv_heads}x{self.head_dim}-s{self.kv_sink}p{self.kv_pos}r{self.cache_rows}"
                     + ("-clip" if self.clip else "") + (f"-rot{self.rotary}" if self.rotary != self.head_dim else ""))
        else:
            assert qkv is None and d > 0 and (policy != STORE2 or d % 2 == 0)
        assert n % (32 if dtype == Q4 else 16) == 0 and not (norm and policy == ADDTO)
        self.want = dict(want)
        self.name = (f"{DTYPE_NAMES[dtype]}-{POLICY_NAMES[policy]}-n{n}-{shape}-t{self.threads}u{self.unroll}w{self.wpc}"
                     f"c{cus}" + ("-rows0" if rows == 0 else "") + ("-norm" if norm else "")
                     + (("-gelu", "-silu")[act] if policy == GLU else "") + tag)

    @property
    def q_dim(self):
        return self.n_heads * self.head_dim

    @property
    def kv_dim(self):
        return self.n_kv_heads * self.head_dim

    @property
    def n_vrows(self):
        """Weight rows the launch streams (glu: w1 then w3; qkv*: wq, wk, wv)."""
        if self.policy in QKV_POLICIES:
            return self.q_dim + 2 * self.kv_dim
        return 2 * self.d if self.policy == GLU else self.d

    @property
    def n_groups(self):
        return self.n_vrows // 2 if POLICY_R[self.policy] == 2 else self.d

    @property
    def exact(self):
        """The exact (integer) family: every policy but glu, without the norm."""
        return self.policy != GLU and not self.norm

    @property
    def family(self):
        return next(f for f, ps in FAMILIES.items() if self.policy in ps)

    def plan(self):
        return plan(self.dtype, self.policy, self.kind, self.n, self.n_groups, self.norm, self.threads, self.unroll,
                    self.wpc, self.cus, self.rows)

    def __repr__(self):
        return self.name


def wave_mine(rows, ngl, R, nch, W, wave):
    """gemv_rb_kernel's `mine`: the items of one wave of a workgroup of ngl groups."""
    if rows:
        return ((ngl * R - 1 - wave) // W + 1) * nch if ngl * R > wave else 0
    items = ngl * R * nch
    return (items - 1 - wave) // W + 1 if items > wave else 0


def facts(c, p):
    """The path facts of case c under plan p (the dict of plan() / runtime.gemv_plan)."""
    ch, R = CH[c.dtype], POLICY_R[c.policy]
    f = dict(generic=bool(p["generic"]), lds_big=p["lds"] > 65536)
    if c.policy in QKV_POLICIES:
        pos = {0: "0", 1: "1", 2: "2"}.get(c.kv_pos, c.kv_pos)
        f.update(head_dim=c.head_dim, heads=(c.n_heads, c.n_kv_heads), kv_sink=c.kv_sink, clip=c.clip,
                 kv_pos="last" if c.kv_pos == c.cache_rows - 1 and c.kv_pos > 2 else pos,
                 rotary_partial=c.rotary < c.head_dim,
                 late_loops=p["threads"] * p["nb"] < c.kv_sink * c.kv_dim // 2)
    if p["generic"]:
        nfull, rem = c.n // ch, c.n % ch
        f.update(uloop=nfull >= GENERIC_U, tail=nfull % GENERIC_U > 0, ragged=rem > 0,
                 past=p["nb"] * (GENERIC_THREADS // 64) > c.n_groups, q4_partial=c.dtype == Q4 and c.n % 2048 > 0)
        return f
    W, U, nb, nch = p["threads"] // 64, p["unroll"], p["nb"], c.n // ch
    G = c.n_groups
    ngl = p["ngl_max"]
    cond = dict(nb=G % nb == 0, w=(ngl * R) % W == 0)
    cond["2w"] = ngl * R >= 2 * W
    missed = [k for k, v in cond.items() if not v]
    mines = [(w, wave_mine(p["rows"], g, R, nch, W, w)) for g in {p["ngl_min"], p["ngl_max"]} if g > 0
             for w in range(W)]
    live = [(w, m) for w, m in mines if m > 0]
    cap = xcap(c.norm, p["threads"])
    f.update(threads=p["threads"], U=U, wpc=c.wpc, nch=nch, rows=bool(p["rows"]),
             rows_off=c.policy in ROWS_POLICIES and c.rows == 0 and not missed,
             rows_miss=missed[0] if c.policy in ROWS_POLICIES and c.rows != 0 and len(missed) == 1 else None,
             uneven=G % nb != 0, capped=G < c.cus * c.wpc,
             multistep=not p["rows"] and W >= 2 * nch and any(m >= 2 for _, m in live),
             idle=any(m == 0 for _, m in mines), mine_lt_U=any(m < U for _, m in live),
             mine_mod_U=any(m > U and m % U for _, m in live),
             flush=(any(m > nch for _, m in live) if p["rows"]
                    else any((w + (m - 1) * W) // nch > w // nch for w, m in live)),
             cursor_row=not p["rows"] and any(w // nch > 0 for w, _ in live),
             cursor_chunk=not p["rows"] and any(w % nch > 0 for w, _ in live),
             xregs=bool(p["xregs"]), xcap="at" if c.n == cap else "above" if c.n == cap + ch else None,
             xclamp=bool(p["xregs"]) and c.n < cap, epi_loop=ngl > p["threads"])
    return f


def reaches(c, p):
    """The facts the case is there for that do not hold under plan p (empty: the path is reached)."""
    f = facts(c, p)
    return {k: (v, f.get(k)) for k, v in c.want.items() if f.get(k) != v}


def _qkv_shape(head_dim, n_heads, n_kv_heads, **kw):
    return dict(head_dim=head_dim, n_heads=n_heads, n_kv_heads=n_kv_heads, **kw)


def _table():
    out = []
    EXACT4 = (STORE1, STORE2, RESIDUAL, ADDTO)
    for dt in DTYPES:
        ch = CH[dt]
        k = 0

        def pol(i):  # the four exact matrix policies in turn; d even where store2 needs it
            return EXACT4[i % 4]

        def rows_for(p, d):
            return d + d % 2 if p == STORE2 else d

        # ---- row-block kernel, chunk order, 5 rows: nb = n_groups (capped), ngl = 1, so the few items
        # leave waves idle and every wave below U; all nine threads x U, nch 1 / 3 / 9, wpc 1 / 2 / 4
        for i, (threads, U) in enumerate((t, u) for t in (256, 512, 1024) for u in (2, 4, 8)):
            nch, wpc = (1, 3, 9)[(i + i // 3) % 3], (1, 2, 4)[i % 3]
            p = pol(k)
            W = threads // 64
            want = dict(generic=False, threads=threads, U=U, wpc=wpc, nch=nch, capped=True, uneven=False, rows=False)
            if nch == 1:
                want.update(xregs=True, xclamp=True)  # one chunk: below every capacity
            if p != STORE2 and nch < W:
                want.update(idle=True)  # R = 1: nch items over W waves
            if nch == 9 and W == 4 and p != STORE2:
                want.update(mine_lt_U=U > 2, flush=False)  # mine 3, 2, 2, 2
            out.append(Case(dt, p, nch * ch, rows_for(p, 5), (threads, U, wpc), want))
            k += 1
        # ---- more groups than workgroups at 256 CUs: uneven ngl, waves that cross rows, advance
        # stepping several rows at once, cursors that start past row 0 and past chunk 0
        # 300 rows over 256 workgroups (ngl 2 / 1), rows of 3 chunks, 4 waves: items 6 / 3
        out.append(Case(dt, STORE1, 3 * ch, 300, (256, 2, 1), dict(
            uneven=True, capped=False, nch=3, flush=True, cursor_row=True, cursor_chunk=True, idle=True,
            multistep=False, rows=False)))
        # 600 rows (ngl 3 / 2), 3 chunks, 8 waves >= 2 nch: wave 0 takes items 0 and 8, rows 0 and 2
        out.append(Case(dt, ADDTO, 3 * ch, 600, (512, 4, 1), dict(
            uneven=True, nch=3, multistep=True, flush=True, cursor_row=True, cursor_chunk=True, mine_lt_U=True)))
        # 1300 rows of one chunk (ngl 6 / 5), 4 waves: every advance steps 4 rows; mine 2, 2, 1, 1 at U = 2
        out.append(Case(dt, RESIDUAL, ch, 1300, (256, 2, 1), dict(
            uneven=True, nch=1, multistep=True, flush=True, cursor_row=True, cursor_chunk=False, mine_lt_U=True,
            rows=False, rows_miss=None)))
        # 1030 rows as 515 pairs over 512 workgroups (wpc 2), and 1030 singles over 1024 (wpc 4)
        out.append(Case(dt, STORE2, ch, 1030, (512, 2, 2), dict(uneven=True, wpc=2, capped=False, idle=True)))
        out.append(Case(dt, STORE1, ch, 1030, (1024, 8, 4), dict(uneven=True, wpc=4, capped=False, idle=True,
                                                                  multistep=False)))
        # one workgroup (1 CU) with 37 rows of 3 chunks at U = 2, 4 waves: 111 items, mine 28, 28, 28, 27:
        # a last step with a dead slot; at U = 8 with 9 chunks: 333 items, mine 84, 83, 83, 83
        out.append(Case(dt, STORE1, 3 * ch, 37, (256, 2, 1), dict(mine_mod_U=True, flush=True, nch=3, idle=False),
                        cus=1))
        out.append(Case(dt, RESIDUAL, 9 * ch, 37, (256, 8, 1), dict(mine_mod_U=True, flush=True, nch=9, idle=False,
                                                                      cursor_row=False, cursor_chunk=True), cus=1))
        out.append(Case(dt, STORE2, 3 * ch, 38, (1024, 4, 1), dict(mine_mod_U=True, multistep=True, flush=True),
                        cus=1))
        # ---- whole-row mode. At 256 CUs: 256 workgroups of 8 rows of one chunk at 4 waves (2 rows per wave).
        q1024 = _qkv_shape(128, 8, 4, kv_sink=2, kv_pos=2, cache_rows=4)  # 1024 + 2 * 512 rows = 1024 groups
        hit = dict(rows=True, uneven=False, capped=False, flush=True, nch=1, idle=False)
        out.append(Case(dt, RESIDUAL, ch, 2048, (256, 2, 1), hit))
        out.append(Case(dt, GLU, ch, 1024, (256, 4, 1), hit, act=SILU))
        out.append(Case(dt, GLU, ch, 1024, (256, 4, 1), hit, norm=True, act=GELU))
        for p in QKV_POLICIES:
            out.append(Case(dt, p, ch, geo=(256, 4, 1), want=hit, qkv=q1024))
        out.append(Case(dt, QKV, ch, geo=(256, 4, 1), want=hit, qkv=q1024, norm=True))
        # the same shapes in chunk order
        off = dict(rows=False, rows_off=True)
        out.append(Case(dt, RESIDUAL, ch, 2048, (256, 2, 1), off, rows=0))
        out.append(Case(dt, GLU, ch, 1024, (256, 4, 1), off, rows=0, act=SILU))
        out.append(Case(dt, QKVB, ch, geo=(256, 4, 1), want=off, qkv=q1024, rows=0))
        # one short of each entry condition: 1023 pairs (n_groups % nb); 9 rows per workgroup over 4
        # waves ((ngl R) % W); 4 rows per workgroup (ngl R = W < 2 W)
        out.append(Case(dt, GLU, ch, 1023, (256, 4, 1), dict(rows=False, rows_miss="nb", uneven=True), act=GELU))
        out.append(Case(dt, RESIDUAL, ch, 2304, (256, 4, 1), dict(rows=False, rows_miss="w")))
        out.append(Case(dt, RESIDUAL, ch, 1024, (256, 4, 1), dict(rows=False, rows_miss="2w")))
        # 2 CUs: whole rows of 3 and 9 chunks, 8 and 16 waves, 2 and 4 rows per wave; U below, at and
        # above the chunks of a row; and in chunk order
        q2 = _qkv_shape(16, 2, 1, kv_sink=0, kv_pos=1, cache_rows=3)  # 64 rows = 32 groups: 16 per workgroup
        for i, (threads, U, nch, d) in enumerate(((512, 2, 3, 16), (512, 4, 9, 32), (1024, 8, 3, 32))):
            want = dict(rows=True, nch=nch, threads=threads, U=U, flush=True, idle=False)
            out.append(Case(dt, GLU, nch * ch, d, (threads, U, 1), want, cus=2, act=(SILU, GELU)[i % 2]))
            out.append(Case(dt, GLU, nch * ch, d, (threads, U, 1), want, cus=2, norm=True, act=(GELU, SILU)[i % 2]))
            out.append(Case(dt, RESIDUAL, nch * ch, 2 * d, (threads, U, 1), want, cus=2))
            out.append(Case(dt, GLU, nch * ch, d, (threads, U, 1), dict(rows=False, rows_off=True, nch=nch), cus=2,
                            rows=0, norm=True, act=(SILU, GELU)[i % 2]))
        for i, p in enumerate(QKV_POLICIES):
            out.append(Case(dt, p, 3 * ch, geo=(512, (2, 4, 8)[i], 1), want=dict(rows=True, nch=3, flush=True), cus=2,
                            qkv=q2, norm=i != 1))
        # ---- staging of x: n at the xregs capacity and one chunk above, with and without the norm,
        # at each thread count (every capacity is a multiple of every CH); 5 rows
        for i, threads in enumerate((256, 512, 1024)):
            for norm in (False, True):
                cap = xcap(norm, threads)
                for n, xr, where in ((cap, True, "at"), (cap + ch, False, "above")):
                    want = dict(xregs=xr, xcap=where, xclamp=False, threads=threads, generic=False)
                    if norm:
                        p = (STORE1, GLU, RESIDUAL)[(i + (where == "at")) % 3]
                        out.append(Case(dt, p, n, 5, (threads, 4, 1), want, norm=True, act=(SILU, GELU)[i % 2]))
                    else:
                        out.append(Case(dt, pol(i + (where == "at")), n, rows_for(pol(i + (where == "at")), 5),
                                        (threads, 4, 1), want))
        # dynamic LDS above 64 KiB: Qwen2.5-7B's W2 rows (18944: whole chunks in f32 / f16 only)
        out.append(Case(dt, RESIDUAL, 18944, 5, (1024, 2, 1), dict(lds_big=True, generic=dt not in (F32, F16))))
        # ---- the epilogue loop past the first THREADS groups: one workgroup of 259 groups at 256
        # threads (1 CU); residual for every type (PRE), every policy family for e4m3 (the row scale)
        epi = dict(epi_loop=True, threads=256, uneven=False)
        q259 = _qkv_shape(74, 5, 1, kv_sink=2, kv_pos=3, cache_rows=5, clip=True)  # 370 + 2 * 74 = 518 rows
        out.append(Case(dt, RESIDUAL, ch, 259, (256, 4, 1), epi, cus=1))
        if dt == E4M3:
            out.append(Case(dt, STORE1, ch, 259, (256, 2, 1), epi, cus=1))
            out.append(Case(dt, STORE2, ch, 518, (256, 4, 1), epi, cus=1))
            out.append(Case(dt, ADDTO, ch, 259, (256, 8, 1), epi, cus=1))
            out.append(Case(dt, STORE1, 3 * ch, 259, (256, 4, 1), epi, cus=1, norm=True))
            out.append(Case(dt, GLU, ch, 259, (256, 4, 1), epi, cus=1, norm=True, act=SILU))
            out.append(Case(dt, GLU, ch, 259, (256, 2, 1), epi, cus=1, act=GELU))
            for p in QKV_POLICIES:
                out.append(Case(dt, p, ch, geo=(256, 4, 1), want=epi, cus=1, qkv=q259))
        # ---- generic kernel: a row shorter than a lane's piece times 64; a chunk less its last piece;
        # a tail and a ragged end; the U loop and a ragged end; U loop + tail + ragged end, twice; and
        # dim 3584 (Qwen2.5-7B) where it is no whole number of chunks. 5 groups: 3 waves past n_groups.
        step = 32 if dt == Q4 else 16
        shapes = [(step, dict(uloop=False, tail=False, ragged=True)),
                  (ch - step, dict(uloop=False, tail=False, ragged=True)),
                  (3 * ch + step, dict(uloop=False, tail=True, ragged=True)),
                  (4 * ch + step, dict(uloop=True, tail=False, ragged=True)),
                  (5 * ch + (64 if dt == Q4 else 48), dict(uloop=True, tail=True, ragged=True)),
                  (9 * ch + step, dict(uloop=True, tail=True, ragged=True))]
        if dt in (F8, E4M3, Q4):
            shapes.append((3584, dict(uloop=False, tail=True, ragged=True)))  # 3 chunks and a half; q4: 1 and 3 / 4
        q30 = _qkv_shape(6, 3, 1, kv_sink=2, kv_pos=2, cache_rows=4)  # 18 + 2 * 6 = 30 rows: 15 groups
        for i, (n, w) in enumerate(shapes):
            want = dict(w, generic=True, past=True)
            if dt == Q4:
                want.update(q4_partial=True)
            p = pol(i)
            out.append(Case(dt, p, n, rows_for(p, 5), want=want))
            out.append(Case(dt, pol(i + 2), n, rows_for(pol(i + 2), 37), want=want))
            out.append(Case(dt, GLU, n, 5, want=want, norm=i % 2 == 0, act=(SILU, GELU)[i % 2]))
            qp = QKV_POLICIES[i % 3]
            out.append(Case(dt, qp, n, want=want, qkv=dict(q30, clip=i % 2 == 1)))
            out.append(Case(dt, QKV_POLICIES[(i + 1) % 3], n, want=want, norm=True,
                            qkv=dict(q30, kv_sink=(0, 2)[i % 2], clip=i % 2 == 0, rotary=(6, 4)[i % 2])))
            if i % 2 == 0:
                out.append(Case(dt, (STORE1, STORE2, RESIDUAL)[(i // 2) % 3], n,
                                rows_for((STORE1, STORE2, RESIDUAL)[(i // 2) % 3], 5), want=want, norm=True))
        # ---- the QKV policies on the row-block kernel: every head_dim, 1 and 2 kv heads under 2 and 8 q
        # heads, kv_pos 0 / 1 / 2 / last, kv_sink 0 / 2, clip off and on, a table with (1, 0) past
        # rotary_dim; every policy on every shape, exact and with the norm (true cos / sin)
        qshapes = [_qkv_shape(16, 2, 1, kv_sink=0, kv_pos=0, cache_rows=3),
                   _qkv_shape(64, 8, 2, kv_sink=2, kv_pos=2, cache_rows=5, clip=True, rotary=32),
                   _qkv_shape(128, 2, 2, kv_sink=0, kv_pos=1, cache_rows=4, clip=True),
                   _qkv_shape(256, 8, 1, kv_sink=2, kv_pos=5, cache_rows=6, rotary=128)]
        for i, q in enumerate(qshapes):
            geo = ((512, 4, 1), (256, 2, 2), (1024, 8, 1), (512, 2, 4))[i]
            want = dict(generic=False, head_dim=q["head_dim"], heads=(q["n_heads"], q["n_kv_heads"]),
                        kv_sink=q["kv_sink"], kv_pos=("0", "2", "1", "last")[i], clip=q.get("clip", False),
                        rotary_partial="rotary" in q, late_loops=False)
            for j, p in enumerate(QKV_POLICIES):
                # (2560 rows under head_dim 256: one chunk each)
                out.append(Case(dt, p, (1, 3 if i < 3 else 1)[(i + j) % 2] * ch, geo=geo, want=want, qkv=q))
                out.append(Case(dt, p, (3 if i < 3 else 1, 1)[(i + j) % 2] * ch, geo=geo, want=want, qkv=q, norm=True))
        # one workgroup of 256 threads (1 CU) under 2 sink rows of 512: 512 pairs, late's loop runs twice
        qlate = _qkv_shape(256, 2, 2, kv_sink=2, kv_pos=3, cache_rows=5, clip=True)
        for j, p in enumerate(QKV_POLICIES):
            out.append(Case(dt, p, ch, geo=(256, 4, 1), want=dict(late_loops=True, epi_loop=True, kv_sink=2), cus=1,
                            qkv=qlate, norm=j == 1))
        # ---- the norm on the row-block kernel with store1 / store2 (logits), glu, residual
        for i, (threads, U) in enumerate(((256, 4), (512, 8), (1024, 2))):
            nch = (3, 1, 9)[i]
            want = dict(generic=False, threads=threads, U=U, nch=nch)
            if nch == 1:
                want.update(xregs=True, xclamp=True)
            out.append(Case(dt, (STORE1, STORE2, STORE1)[i], nch * ch, 38, (threads, U, 1), want, norm=True))
            out.append(Case(dt, GLU, nch * ch, 37, (threads, U, 1), want, norm=True, act=(SILU, GELU)[i % 2]))
            out.append(Case(dt, RESIDUAL, nch * ch, 37, (threads, U, 1), want, norm=True))
        # the logits launch in small: pairs of rows, the norm, 4 workgroups per CU, n_groups % nb != 0
        # (Mistral-7B: 16000 pairs over 1024 workgroups; here 1250)
        out.append(Case(dt, STORE2, ch, 2500, (512, 4, 4), dict(uneven=True, capped=False, wpc=4), norm=True))
    return out


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names are unique"
BY_KIND = {(dt, fam): [c for c in CASES if c.dtype == dt and c.family == fam] for dt in DTYPES for fam in FAMILIES}

# Every fact the suite is there for, as (fact, value, types): at least one case of each of the types
# must want it (test_gemv_cpu.py). None: every type.
NARROW = (F8, Q4, E4M3)
REQUIRED = (
    [("threads", t, None) for t in (256, 512, 1024)] + [("U", u, None) for u in (2, 4, 8)]
    + [("wpc", w, None) for w in (1, 2, 4)] + [("nch", k, None) for k in (1, 3, 9)]
    + [(k, True, None) for k in ("multistep", "idle", "mine_lt_U", "mine_mod_U", "uneven", "capped", "flush",
                                 "cursor_row", "cursor_chunk", "rows", "rows_off", "xclamp", "lds_big", "epi_loop",
                                 "generic", "uloop", "tail", "ragged", "past", "clip", "rotary_partial",
                                 "late_loops")]
    + [("rows_miss", m, None) for m in ("nb", "w", "2w")]
    + [("xregs", v, None) for v in (True, False)] + [("xcap", v, None) for v in ("at", "above")]
    + [("q4_partial", True, (Q4,))]
    + [("head_dim", h, None) for h in (16, 64, 128, 256)] + [("heads", h, None) for h in ((2, 1), (8, 2), (2, 2), (8, 1))]
    + [("kv_sink", s, None) for s in (0, 2)] + [("kv_pos", p, None) for p in ("0", "1", "2", "last")]
    + [("clip", False, None)]
)
