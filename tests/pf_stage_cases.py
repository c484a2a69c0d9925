"""The case table of the prefill stage tests (the row norm, the QKV / residual / GLU / logits GEMM
epilogues, the skinny reduce and logprob_kernel through yalm_prefill_stage), shared by
test_pf_stage_cpu.py and test_gpu_pf_stage.py. TEST INFRASTRUCTURE ONLY; needs no library.

A case names the stage, the family (exact: bit for bit; float: against float64 in bars), the forms
spec it runs under, the CU count its tile widths and grid are sized for (pinned, so the path is the
same on any device), the shape, and the path it is there for: conditions (`want`) on the info the
hook reports. `expect(case)` restates prefill.hip's choices (pick_bn, sk_pick_ks, the QKV form, the
persistent grid, the norm bracket) from the case alone; test_pf_stage_cpu.py holds every case's
`want` to it, the GPU test holds the library's report to `want` (reaches)."""
NORM, QKV, RESIDUAL, GLU, LOGPROB = range(5)  # yalm_prefill_stage stages
STAGE_NAMES = ("norm", "qkv", "residual", "glu", "logprob")
PG = dict(qkv=0, wo=1, glu=2, w2=3, cls=4)
PF_WO, PF_W2 = 1, 3
GELU, SILU = 0, 1
CUS = 256
SK_MAX_T, SK_KSTEP, SK_ROWS, G_BM = 64, 256, 64, 256


def parse_forms(spec):
    f = dict(qkv=-1, wo=-1, glu=-1, w2=-1, cls=-1, p8=1, persist=1, skinny=1, qkv1=1, skl=1, wnorm=1)
    for kv in filter(None, spec.split(",")):
        k, v = kv.split(":")
        f["p8" if k == "8p" else k] = int(v)
    return f


def pick_bn(f, kind, M, n_eff, glu, cus):
    """prefill.hip pick_bn."""
    fits = lambda bn: n_eff % bn == 0 and (not glu or bn in (128, 256))
    if f[kind] > 0 and fits(f[kind]):
        return f[kind]
    tiles_m = -(-M // G_BM)
    best, best_cost = 0, 0
    for bn in (128, 192, 256, 320):
        if not fits(bn):
            continue
        rounds = -(-(tiles_m * (n_eff // bn)) // cus)
        cost = rounds * (bn + 64) * (3 if f["p8"] and bn in (192, 256) else 4)
        if not best or cost < best_cost or (cost == best_cost and bn > best):
            best, best_cost = bn, cost
    return best


def sk_pick_ks(gemms, T):
    """prefill.hip sk_pick_ks: gemms = ((N, K, mult), ...) sharing one partial buffer."""
    TP = 16 * (-(-T // 16))
    best, kmin, wg1 = -1, min(K // m for _, K, m in gemms), sum(N // SK_ROWS * m for N, _, m in gemms)
    for ks in range(1, kmin // SK_KSTEP + 1):
        if not all(K % (ks * m) == 0 and (K // (ks * m)) % SK_KSTEP == 0 and TP * (K // (ks * m)) * 2 <= 32768
                   for _, K, m in gemms):
            continue
        best = ks
        if wg1 * ks >= 512:
            break
    return best


def _gemm(f, bn, glu_plain128, T, N, cus, two=False):
    """One large-tile launch: (bn, 8-phase?, tiles, grid)."""
    p8 = bool(f["p8"]) and (bn in (192, 256) or (bn == 128 and glu_plain128))
    tiles = -(-T // G_BM) * (N // bn)
    grid = cus if (p8 and f["persist"] and tiles > cus and not two) else tiles
    return bn, p8, tiles, grid


def expect(c):
    """The info yalm_prefill_stage must report for case c (prefill.hip restated)."""
    f, cus, T = parse_forms(c.forms), c.cus, c.T
    e = dict(skinny=0, ks=0, ks2=0, n_gemm=0, bn=(0, 0), eight_phase=0, two_depth=0, tiles=0, grid=0, persistent=0,
             norm_nv=0)
    if c.stage == NORM:
        nv = -(-(c.dim // 4) // 64)
        e["norm_nv"] = 0 if not f["wnorm"] or nv > 32 else next(b for b in (4, 8, 12, 16, 24, 32) if nv <= b)
        return e
    can_small = T <= SK_MAX_T and f["skinny"] and not c.split
    launches = []
    if c.stage == QKV:
        ks = sk_pick_ks(((c.q_dim, c.dim, 1), (2 * c.kv_dim, 2 * c.dim, 2)), T)
        if can_small and ks > 0:
            e.update(skinny=1, ks=ks, ks2=2 * ks)
        elif c.split:
            n = c.q_dim + 2 * c.kv_dim
            launches = [_gemm(f, pick_bn(f, "qkv", T, n, False, cus), True, T, n, cus)]
        elif f["qkv1"] and f["p8"] and f["qkv"] < 0 and c.q_dim % 256 == 0 and (2 * c.kv_dim) % 256 == 0:
            launches = [_gemm(f, 256, True, T, c.q_dim + 2 * c.kv_dim, cus, two=True)]
            e["two_depth"] = 1
        else:
            launches = [_gemm(f, pick_bn(f, "qkv", T, n, False, cus), True, T, n, cus) for n in (c.q_dim, 2 * c.kv_dim)]
    elif c.stage == RESIDUAL:
        ks = sk_pick_ks(((c.n, c.k, 1),), T)
        if can_small and ks > 0:
            e.update(skinny=1, ks=ks, ks2=ks)
        else:
            kind = "wo" if c.kind == PF_WO else "w2"
            launches = [_gemm(f, pick_bn(f, kind, T, c.n, False, cus), True, T, c.n, cus)]
    elif c.stage == GLU:
        ks = sk_pick_ks(((2 * c.hidden, c.dim, 1),), T)
        if can_small and ks > 0:
            e.update(skinny=1, ks=ks, ks2=ks)
        else:  # (the GLU row policy has no 8-phase form at width 128)
            launches = [_gemm(f, pick_bn(f, "glu", T, 2 * c.hidden, True, cus), False, T, 2 * c.hidden, cus)]
    else:
        launches = [_gemm(f, pick_bn(f, "cls", T, c.vocab, False, cus), True, T, c.vocab, cus)]
    if launches:
        e["n_gemm"] = len(launches)
        e["bn"] = tuple(l[0] for l in launches) + (0,) * (2 - len(launches))
        e["eight_phase"] = sum(int(l[1]) << i for i, l in enumerate(launches))
        _, _, e["tiles"], e["grid"] = launches[-1]
        e["persistent"] = int(e["grid"] < e["tiles"])
    return e


class Case:
    def __init__(self, stage, tag, why, family, T, forms="", cus=CUS, split=0, want=(), **p):
        self.stage, self.why, self.family, self.T, self.forms, self.cus, self.split = stage, why, family, T, forms, cus, split
        self.exact = family == "exact"
        self.__dict__.update(p)
        if stage == QKV:
            self.q_dim, self.kv_dim = self.n_heads * self.head_dim, self.n_kv_heads * self.head_dim
        self.want = dict(want)
        self.name = f"{STAGE_NAMES[stage]}-{family}-{tag}-T{T}" + ("-split" if split else "") + (
            f"-{forms.replace(',', '-').replace(':', '')}" if forms else "") + (f"-c{cus}" if cus != CUS else "")

    def __repr__(self):
        return self.name


def reaches(c, info):
    """The conditions of c.want that info (the hook's report, or expect(c)) misses; empty = reached."""
    return [f"{k}: want {v}, got {info[k]}" for k, v in c.want.items()
            if (tuple(info[k]) if k == "bn" else info[k]) != v]


CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


# ---------------------------------------------------------------- NORM: every NV bracket, the
# fallback past 32, the forced workgroup kernel, T = 5 (the 4-rows-per-block tail), both splits
for dim, nv in ((384, 4), (1152, 8), (2176, 12), (3200, 16), (4224, 24), (6272, 32), (8320, 0)):
    for split in (0, 1):
        _add(NORM, f"d{dim}", f"NV bracket {nv}", "exact", 5, split=split, want=dict(norm_nv=nv), dim=dim, mode="pow2")
        _add(NORM, f"d{dim}", f"NV bracket {nv}", "float", 5, split=split, want=dict(norm_nv=nv), dim=dim, mode="gauss")
for split in (0, 1):
    _add(NORM, "d384", "wnorm:0 forces the workgroup kernel", "exact", 5, forms="wnorm:0", split=split,
         want=dict(norm_nv=0), dim=384, mode="pow2")
    _add(NORM, "d1152", "wnorm:0 forces the workgroup kernel", "float", 5, forms="wnorm:0", split=split,
         want=dict(norm_nv=0), dim=1152, mode="gauss")
    _add(NORM, "d384-big", "a row above 65504: the range slot holds its largest |y|", "exact", 5, split=split,
         want=dict(norm_nv=4), dim=384, mode="big")
    _add(NORM, "d1152-nan", "a row with a NaN reads as inf in the range slot", "exact", 5, split=split,
         want=dict(norm_nv=8), dim=1152, mode="nan")
_add(NORM, "d8320-big", "the workgroup kernel's range note", "exact", 5, split=1, want=dict(norm_nv=0), dim=8320, mode="big")


# ---------------------------------------------------------------- QKV
def _qkv(tag, why, family, T, heads, forms="", split=0, want=(), dim=128, pos0=3, bias=False, cus=CUS, **p):
    nh, nkv, hd = heads
    _add(QKV, f"{tag}-k{dim}-h{nh}x{nkv}x{hd}-p{pos0}" + ("-bias" if bias else ""), why, family, T, forms=forms,
         split=split, want=want, cus=cus, dim=dim, n_heads=nh, n_kv_heads=nkv, head_dim=hd, pos0=pos0, bias=bias, **p)


for fam in ("exact", "float"):
    # the skinny path: the reduce's partial counts (KS of the q columns, KS2 = 2 KS of k | v), both
    # weight paths (skl), every MT bracket, head_dim 64 and 128
    for dim, ks, T, heads, bias in ((256, 1, 1, (2, 2, 64), False), (256, 1, 16, (1, 1, 128), True),
                                    (512, 2, 17, (2, 2, 64), True), (768, 3, 33, (1, 1, 128), False),
                                    (1024, 4, 64, (2, 2, 64), False), (1280, 5, 17, (3, 1, 128), True)):
        for skl in (1, 0):
            _qkv("skinny", f"skinny reduce: {ks} partials of q, {2 * ks} of k | v", fam, T, heads, dim=dim, bias=bias,
                 forms="" if skl else "skl:0", want=dict(skinny=1, ks=ks, ks2=2 * ks))
    # q then k | v at c0 = q_dim, every width both launches can take, 8-phase and 2-phase
    for bn, heads in ((128, (2, 2, 64)), (192, (3, 3, 128)), (256, (4, 2, 64)), (320, (5, 5, 128))):
        for p8 in (1, 0):
            for T, bias in ((65, False), (257, True)):
                _qkv("two", f"q then k | v at width {bn}, {'8' if p8 else '2'}-phase", fam, T, heads, bias=bias,
                     forms=f"qkv:{bn}" + ("" if p8 else ",8p:0"),
                     want=dict(skinny=0, n_gemm=2, bn=(bn, bn), eight_phase=3 if p8 and bn != 320 else 0, two_depth=0))
    _qkv("two", "a 256-wide k | v tile across k | v (kv_dim 128), T = 17 on the large tiles", fam, 17, (2, 1, 128),
         forms="qkv:256,skinny:0", want=dict(skinny=0, n_gemm=2, bn=(256, 256), eight_phase=3))
    _qkv("two", "q then k | v by qkv1:0 at the automatic widths, T = 256 (a full M tile)", fam, 256, (2, 1, 128),
         forms="qkv1:0", want=dict(skinny=0, n_gemm=2, two_depth=0))
    # the one-launch two-depth form
    for T, heads, bias, dim in ((65, (2, 1, 128), False, 128), (64, (4, 2, 64), True, 192), (257, (4, 4, 64), False, 64)):
        _qkv("depth2", "one launch, two depths: k | v tiles over 2 dim first, q tiles over dim", fam, T, heads, bias=bias,
             dim=dim, forms="skinny:0" if T <= 64 else "",
             want=dict(skinny=0, n_gemm=1, bn=(256, 0), two_depth=1, persistent=0))
    # the split-operand form: one GEMM over [hi | lo], Q stored [hi | lo]
    for bn, heads, T, p8, why in ((192, (1, 1, 128), 65, 1, "a 192-wide tile across q | k and k | v"),
                                  (192, (2, 2, 64), 1, 0, "a 192-wide tile across q | k and k | v, 2-phase, T = 1"),
                                  (320, (3, 1, 128), 257, 1, "q_dim 384, kv_dim 128: a 320-wide tile across q | k | v"),
                                  (320, (6, 2, 64), 17, 0, "q_dim 384, kv_dim 128 at head_dim 64"),
                                  (256, (2, 1, 128), 256, 1, "a 256-wide tile across k | v"),
                                  (256, (4, 2, 64), 64, 0, "a 256-wide tile across k | v, 2-phase"),
                                  (128, (1, 1, 128), 65, 1, "width 128, 8-phase"),
                                  (128, (2, 2, 64), 17, 0, "width 128, 2-phase")):
        for bias in (False, True):
            _qkv("one", "split form: " + why, fam, T, heads, split=1, bias=bias, forms=f"qkv:{bn}" + ("" if p8 else ",8p:0"),
                 want=dict(skinny=0, n_gemm=1, bn=(bn, 0), eight_phase=int(bool(p8 and bn != 320)), two_depth=0))
_qkv("one-wide", "split form: Q values of more than 11 bits, lo != 0 and exact", "exact", 65, (2, 1, 128), split=1,
     bias=True, wide=True, want=dict(skinny=0, n_gemm=1))
_qkv("two-persist", "the persistent loop under the QKV epilogue: 4 + 8 tiles on 2 CUs", "exact", 257, (3, 3, 128),
     forms="qkv:192", cus=2, want=dict(n_gemm=2, bn=(192, 192), persistent=1, grid=2, tiles=8))


# ---------------------------------------------------------------- RESIDUAL (Wo, W2)
def _res(tag, why, family, T, n, k, kind=PF_WO, scale=1.0, **kw):
    _add(RESIDUAL, f"{tag}-n{n}-k{k}-{'wo' if kind == PF_WO else 'w2'}-s{scale:g}", why, family, T, n=n, k=k, kind=kind,
         scale=scale, **kw)


for fam in ("exact", "float"):
    # the skinny reduce: partial counts 1, 2, 3 (remainder loop only), 4, 5, 6 (> 4, no multiple of 4), 8
    for k, ks, T in ((256, 1, 1), (512, 2, 16), (768, 3, 17), (1024, 4, 33), (1280, 5, 64), (1536, 6, 17), (2048, 8, 64)):
        for skl in (1, 0):
            _res("skinny", f"skinny reduce: {ks} partials", fam, T, 128, k, kind=PF_W2 if ks % 2 else PF_WO,
                 scale=8.0 if ks in (2, 5) else 1.0, forms="" if skl else "skl:0", want=dict(skinny=1, ks=ks, ks2=ks))
    for bn, n in ((128, 768), (192, 768), (256, 768), (320, 640)):
        for p8 in (1, 0):
            for T, k, kind, scale in ((65, 192, PF_WO, 1.0), (257, 128, PF_W2, 8.0)):
                key = "wo" if kind == PF_WO else "w2"
                _res("tile", f"width {bn}, {'8' if p8 else '2'}-phase, {k // 64} K tiles, the M tail", fam, T, n, k,
                     kind=kind, scale=scale, forms=f"{key}:{bn}" + ("" if p8 else ",8p:0"),
                     want=dict(skinny=0, n_gemm=1, bn=(bn, 0), eight_phase=int(bool(p8 and bn != 320)), persistent=0))
    _res("tile", "one K tile (the 8-phase prologue alone)", fam, 65, 256, 64, forms="wo:256",
         want=dict(skinny=0, bn=(256, 0), eight_phase=1))
    for split, k in ((0, 320), (1, 192)):
        _res("persist", "the persistent tile loop: 8 tiles on 3 CUs", fam, 300, 768, k, kind=PF_W2, scale=8.0, split=split,
             forms="w2:192", cus=3, want=dict(bn=(192, 0), eight_phase=1, tiles=8, grid=3, persistent=1))
    _res("auto", "the automatic width at T = 17 on the large tiles", fam, 17, 384, 128, forms="skinny:0",
         want=dict(skinny=0, n_gemm=1))

# ---------------------------------------------------------------- GLU (float family: integer A / W, so
# the bar measures the activation alone)
for act in (SILU, GELU):
    an = "silu" if act == SILU else "gelu"
    for bn, p8, T, split, hs in ((128, 1, 65, 0, 1.0), (128, 0, 257, 1, 0.0625), (256, 1, 257, 0, 0.0625),
                                 (256, 0, 65, 1, 1.0), (256, 1, 17, 1, 1.0)):
        _add(GLU, f"{an}-h256-k128-hs{hs:g}", f"width {bn}, {'8' if p8 else '2'}-phase", "float", T, split=split,
             forms=f"glu:{bn}" + ("" if p8 else ",8p:0"), dim=128, hidden=256, act=act, hscale=hs, amp=2,
             want=dict(skinny=0, n_gemm=1, bn=(bn, 0), eight_phase=int(bool(p8 and bn == 256))))
    # the skinny path: the interleaved W1 / W3 remap of a block's first hidden column
    for k, ks, T in ((256, 1, 1), (768, 3, 17), (1024, 4, 64), (1280, 5, 33)):
        _add(GLU, f"{an}-skinny-h256-k{k}", f"skinny GLU reduce: {ks} partials", "float", T, dim=k, hidden=256, act=act,
             hscale=1.0, amp=1, forms="" if ks != 3 else "skl:0", want=dict(skinny=1, ks=ks, ks2=ks))
    # the range slot: products past 65504 at hscale 1 are noted (their largest |v|), at 2^-4 they fit
    for hs in (1.0, 0.0625):
        _add(GLU, f"{an}-range-h256-k256-hs{hs:g}", "the GLU range slot" + (" stays clear" if hs != 1.0 else ""), "float",
             65, dim=256, hidden=256, act=act, hscale=hs, amp=4, forms="glu:256", over=hs == 1.0,
             want=dict(skinny=0, bn=(256, 0)))
    _add(GLU, f"{an}-persist-h384-k64", "the persistent loop under the GLU epilogue: 6 tiles on 4 CUs", "float", 300,
         dim=64, hidden=384, act=act, hscale=1.0, amp=3, forms="glu:256", cus=4,
         want=dict(bn=(256, 0), eight_phase=1, tiles=6, grid=4, persistent=1))

# ---------------------------------------------------------------- LOGPROB
for fam in ("exact", "float"):
    for bn in (128, 192, 256, 320):
        for p8, T in ((1, 17), (0, 257)):
            _add(LOGPROB, f"v3840-k64-w{bn}", f"width {bn}, {'8' if p8 else '2'}-phase: the target at every edge column",
                 fam, T, forms=f"cls:{bn}" + ("" if p8 else ",8p:0"), dim=64, vocab=3840,
                 want=dict(n_gemm=1, bn=(bn, 0), eight_phase=int(bool(p8 and bn != 320)), persistent=0))
    _add(LOGPROB, "v3840-k128", "T = 1", fam, 1, forms="cls:256", dim=128, vocab=3840, want=dict(bn=(256, 0)))
    _add(LOGPROB, "v3840-k64", "T = 256, the split-operand A", fam, 256, forms="cls:192", split=1, dim=64, vocab=3840,
         want=dict(bn=(192, 0)))
    for bn, cus in ((256, 7), (192, 11), (128, 13)):
        _add(LOGPROB, f"v3840-k64-w{bn}", "E16Logits in the persistent tile loop: the LDS partials reused per tile", fam,
             513, forms=f"cls:{bn}", cus=cus, dim=64, vocab=3840,
             want=dict(bn=(bn, 0), eight_phase=1, tiles=3 * (3840 // bn), grid=cus, persistent=1))
    _add(LOGPROB, "v33280-k64-w128", "logprob_kernel past 256 vocab tiles", fam, 3, forms="cls:128", dim=64, vocab=33280,
         want=dict(bn=(128, 0), tiles=260, grid=256, persistent=1))

BY_STAGE = {}
for _c in CASES:
    BY_STAGE.setdefault((_c.stage, _c.family), []).append(_c)
assert len({c.name for c in CASES}) == len(CASES), "case names must be unique"
