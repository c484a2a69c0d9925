"""The case table of the multi-row GEMV tests (gemv_rows_kernel through yalm_matmul_rows), shared
by test_rows_cpu.py and test_gpu_rows.py. TEST INFRASTRUCTURE ONLY; needs no library.

A case names dtype, T, n, d, epilogue, norm, act, xstride, ostride and the path it is there for,
as conditions (`want`) on the facts of its launch plan (`facts`) at 256 CUs. The facts:
  nseg     K segments of the staged x (1: staged whole)
  gpw      groups per wave
  uloop    the last segment runs the U = 4 chunk loop
  tail     the last segment has 1..3 whole chunks after the U loop (the chunk-at-a-time loop)
  ragged   the row ends inside a chunk (only lanes below the end read it)
  idle     the grid holds waves without a valid group (they sit through every barrier)
  partial  the last wave with a valid group has an invalid one too (gpw > 1)
  clamp    an odd row count under RStore / RResidual: the last group's second row is clamped
Chunks: CH = 64 lanes x EPL elements = 256 (f32), 512 (f16), 1024 (fp8). kcap(T), the longest row
staged whole: 32768 / T floats rounded down to whole chunks.

Strides: xstride defaults to n and ostride to d rounded up to a multiple of 4 (the hook refuses
other strides), so almost every case has sentinels behind its outputs; the stride cases have
xstride = n + 4 and ostride = d + 3 with d = 1 mod 4."""
F32, F16, F8 = 0, 1, 3  # yalm_amd.models F32, F16, F8E5M2
STORE, RESIDUAL, GLU = 0, 1, 2  # yalm_matmul_rows epilogues
GELU, SILU = 0, 1
DTYPES = (F32, F16, F8)
DTYPE_NAMES = {F32: "f32", F16: "f16", F8: "fp8"}
EPILOGUE_NAMES = {STORE: "store", RESIDUAL: "residual", GLU: "glu"}
EPL = {F32: 4, F16: 8, F8: 16}
CH = {t: 64 * e for t, e in EPL.items()}
ROWS_X_BYTES = 128 * 1024
ROWS_U = 4
WAVES = 8  # ROWS_THREADS / 64
R = 2      # weight rows per group
PLAN_CUS = 256


def kcap(dtype, T):
    return ROWS_X_BYTES // 4 // T // CH[dtype] * CH[dtype]


def plan(dtype, n, n_groups, T, cus=PLAN_CUS):
    """yalm_rows_plan restated (test_rows_cpu.py holds the library's function to it)."""
    ch = CH[dtype]
    kseg = min(-(-n // ch) * ch, kcap(dtype, T))
    nseg = -(-n // kseg)
    gpw = 1 if nseg > 1 else max(1, n_groups // (WAVES * cus))
    blocks = -(-n_groups // (WAVES * gpw))
    return dict(kseg=kseg, nseg=nseg, gpw=gpw, blocks=blocks, lds=(T * kseg + T * 16) * 4)


class Case:
    __slots__ = ("name", "dtype", "T", "n", "d", "epilogue", "norm", "act", "xstride", "ostride", "want")

    def __init__(self, dtype, T, n, d, epilogue, want, norm=False, act=SILU, strided=False):
        self.dtype, self.T, self.n, self.d, self.epilogue, self.norm, self.act = dtype, T, n, d, epilogue, norm, act
        self.xstride = n + 4 if strided else n
        self.ostride = d + 3 if strided else (d + 3) // 4 * 4
        assert self.ostride % 4 == 0 and n % 16 == 0
        self.want = dict(want)
        self.name = (f"{DTYPE_NAMES[dtype]}-{EPILOGUE_NAMES[epilogue]}-T{T}-n{n}-d{d}"
                     + ("-norm" if norm else "") + (("-gelu", "-silu")[act] if epilogue == GLU else "")
                     + ("-strided" if strided else ""))

    @property
    def n_groups(self):
        return self.d if self.epilogue == GLU else (self.d + 1) // R

    @property
    def exact(self):
        """The exact (integer) family: RStore / RResidual without the norm."""
        return self.epilogue != GLU and not self.norm

    def __repr__(self):
        return self.name


def facts(c, p):
    """The path facts of case c under plan p (a dict with kseg, nseg, gpw, blocks)."""
    ch = CH[c.dtype]
    kl = c.n - (p["nseg"] - 1) * p["kseg"]  # the last segment
    nfull, rem = kl // ch, kl % ch
    slots = p["blocks"] * WAVES * p["gpw"]
    return dict(nseg=p["nseg"], gpw=p["gpw"], uloop=nfull >= ROWS_U, tail=nfull % ROWS_U > 0, ragged=rem > 0,
                idle=slots - c.n_groups >= p["gpw"], partial=c.n_groups % p["gpw"] > 0,
                clamp=c.epilogue != GLU and c.d % 2 == 1)


def reaches(c, p):
    """The facts the case is there for that do not hold under plan p (empty: the path is reached)."""
    f = facts(c, p)
    return {k: (v, f[k]) for k, v in c.want.items() if f[k] != v}


def _table():
    out = []
    for dt in DTYPES:
        ch, epl = CH[dt], EPL[dt]
        # ---- x staged whole, gpw 1. n: a row shorter than a chunk; a chunk less its last 16
        # elements; one chunk; a tail only; the U loop only; U loop + tail + ragged end, twice
        shapes = [(16, dict(uloop=False, tail=False, ragged=True)),
                  (ch - 16, dict(uloop=False, tail=False, ragged=True)),
                  (ch, dict(uloop=False, tail=True, ragged=False)),
                  (3 * ch, dict(uloop=False, tail=True, ragged=False)),
                  (4 * ch, dict(uloop=True, tail=False, ragged=False)),
                  (5 * ch + 48, dict(uloop=True, tail=True, ragged=True)),
                  (9 * ch + 16, dict(uloop=True, tail=True, ragged=True))]
        assert (ch - 16) % epl == 0
        k = 0
        for T in (1, 2, 3, 4):
            shapes = shapes[:6] + [(9 * ch + 16, dict(uloop=True, tail=True, ragged=True))]
            if 9 * ch + 16 > kcap(dt, T):
                # fp8 at T = 4: 9232 elements are above kcap = 8192, so this row is staged in two
                # segments (it stays, as that); 7 chunks + 16 are the longest whole-staged shape
                shapes[6] = (7 * ch + 16, dict(uloop=True, tail=True, ragged=True))
                for d in (5, 37):
                    want = dict(nseg=2, gpw=1, uloop=False, tail=True, ragged=True, idle=True, clamp=True)
                    out.append(Case(dt, T, 9 * ch + 16, d, (STORE, RESIDUAL)[k % 2], want))
                    k += 1
            for n, w in shapes:
                for d in (5, 37):  # odd: the clamp; 5 rows are 3 groups, 5 of the 8 waves idle
                    want = dict(w, nseg=1, gpw=1, idle=True, clamp=True)
                    out.append(Case(dt, T, n, d, (STORE, RESIDUAL)[k % 2], want))
                    k += 1
            # the norm as production runs it: logits (RStore) and W1 | W3 (RGlu), and with RResidual
            want = dict(nseg=1, gpw=1, uloop=True, tail=True, ragged=True, idle=True)
            out.append(Case(dt, T, 5 * ch + 48, 37, STORE, dict(want, clamp=True), norm=True))
            out.append(Case(dt, T, shapes[6][0], 5, RESIDUAL, dict(want, clamp=True), norm=True))
            for i, (n, w) in enumerate((shapes[1], shapes[5], shapes[6])):
                out.append(Case(dt, T, n, (5, 37)[(T + i) % 2], GLU, dict(w, nseg=1, gpw=1, idle=True), norm=True,
                                act=(SILU, GELU)[(T + i) % 2]))
                out.append(Case(dt, T, n, (37, 5)[(T + i) % 2], GLU, dict(w, nseg=1, gpw=1, idle=True), norm=True,
                                act=(GELU, SILU)[(T + i) % 2]))
        # ---- x staged by K segments (gpw 1): a second segment that is a ragged end only; a last
        # segment with the U loop, a chunk tail and a ragged end; three segments at T = 4. 5 rows:
        # the idle waves sit through every segment's barriers.
        for T in (1, 2, 3, 4):
            kc = kcap(dt, T)
            segs = [(kc + 16, dict(nseg=2, uloop=False, tail=False, ragged=True)),
                    (kc + 5 * ch + 48, dict(nseg=2, uloop=True, tail=True, ragged=True))]
            if T == 4:
                segs.append((2 * kc + ch + 16, dict(nseg=3, uloop=False, tail=True, ragged=True)))
            for n, w in segs:
                for d in (5, 19):
                    want = dict(w, gpw=1, idle=True, clamp=True)
                    out.append(Case(dt, T, n, d, (STORE, RESIDUAL)[k % 2], want))
                    k += 1
            # with the norm (normw is read at k0 + i): no production launch is segmented with it
            n, w = segs[1]
            out.append(Case(dt, T, n, 5, STORE, dict(w, gpw=1, idle=True, clamp=True), norm=True))
            n, w = segs[-1]
            out.append(Case(dt, T, n, 5, GLU, dict(w, gpw=1, idle=True), norm=True, act=(SILU, GELU)[T % 2]))
        # ---- gpw > 1 (short rows, many of them). d 8192: gpw 2, every wave whole. d 12299 =
        # 2 (3 * 2048 + 5) + 1: gpw 3, odd, 6150 groups = 2050 whole waves. d 12297: 6149 groups,
        # the last wave holds two valid groups and an invalid one. RGlu: 6149 groups.
        for i, T in enumerate((1, 3, 4)):
            ns = (64, 128) if i % 2 == 0 else (128, 64)
            for j, (n, d, w) in enumerate(((ns[0], 8192, dict(gpw=2, idle=False, partial=False, clamp=False)),
                                           (ns[1], 8192, dict(gpw=2, idle=False, partial=False, clamp=False)),
                                           (ns[0], 12299, dict(gpw=3, idle=True, partial=False, clamp=True)),
                                           (ns[1], 12297, dict(gpw=3, idle=True, partial=True, clamp=True)))):
                out.append(Case(dt, T, n, d, (STORE, RESIDUAL)[(i + j) % 2], dict(w, nseg=1)))
            for j, n in enumerate(ns):
                out.append(Case(dt, T, n, 6149, GLU, dict(nseg=1, gpw=3, idle=True, partial=True), norm=True,
                                act=(SILU, GELU)[(i + j) % 2]))
        # ---- strides: xstride = n + 4, ostride = d + 3, every epilogue; whole and segmented
        want = dict(nseg=1, gpw=1, uloop=True, tail=True, ragged=True, idle=True)
        out.append(Case(dt, 4, 5 * ch + 48, 5, STORE, dict(want, clamp=True), strided=True))
        out.append(Case(dt, 3, 5 * ch + 48, 37, RESIDUAL, dict(want, clamp=True), strided=True))
        out.append(Case(dt, 4, 5 * ch + 48, 5, GLU, want, norm=True, act=SILU, strided=True))
        out.append(Case(dt, 2, 5 * ch + 48, 37, GLU, want, norm=True, act=GELU, strided=True))
        out.append(Case(dt, 2, 5 * ch + 48, 5, STORE, dict(want, clamp=True), norm=True, strided=True))
        want = dict(nseg=2, gpw=1, uloop=True, tail=True, ragged=True, idle=True, clamp=True)
        out.append(Case(dt, 4, kcap(dt, 4) + 5 * ch + 48, 5, RESIDUAL, want, strided=True))
        out.append(Case(dt, 3, kcap(dt, 3) + 5 * ch + 48, 5, STORE, want, norm=True, strided=True))
    return out


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names are unique"
BY_KIND = {(dt, ep): [c for c in CASES if (c.dtype, c.epilogue) == (dt, ep)] for dt in DTYPES
           for ep in (STORE, RESIDUAL, GLU)}
