"""CPU: speculative sampled decode (include/yalm_hip.h, yalm_generate_speculative_sampled) as a
numpy model of the device loop -- the draw by tests/sampling_ref.py, drafts and acceptance by
tests/spec_ref.py, a toy next-logits function of the history -- against the plain sampled
sequence; the slips the rule guards against, each seen by a named case; and the new names in the
header, the library, the binding and the CLI."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import sampling_ref as R
import spec_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")

V = 64
TEMP, TOP_K, TOP_P = 0.8, 8, 0.9
CAP = 4096  # the model's token buffer


@functools.lru_cache(maxsize=None)
def _tables(seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((V, V)) * 2).astype(np.float32)
    b = (rng.standard_normal((V, V)) * 1).astype(np.float32)
    for t in range(V):
        a[t, (5 * t + 1) % V] += 3.0  # a likely successor: the sequences repeat, the n-gram drafter hits
    return a, b


def toy_logits(fed, seed=0, zero_bias=0.0):
    """The logits after feeding the token sequence `fed`: a function of its last two tokens."""
    a, b = _tables(seed)
    l = a[fed[-1]] + (b[fed[-2]] if len(fed) > 1 else 0)
    l = l.astype(np.float32).copy()
    l[0] += np.float32(zero_bias)
    return l


def draw(l, u, top_k=TOP_K, top_p=TOP_P):
    return R.Rule(l, R.weights_f32(l, TEMP), top_k, top_p).draw(u)


def plain_sampled(logits_of, fed, n, u):
    fed, out = list(fed), []
    for i in range(n):
        out.append(draw(logits_of(fed), u[i]))
        fed.append(out[-1])
    return out


SLIPS = ("same_u", "adv_1", "adv_T", "same_row", "none_is_0", "trunc_row0", "carry_u")


class Device:
    """The state one decoder keeps between calls: the KV rows (the token fed at each position),
    the token buffer and what a slip carries over."""

    def __init__(self, prompt):
        self.kv = list(prompt[:-1])
        self.carry = 0


def spec_sampled(dev, logits_of, token, pos, n, rows, u, context=None, stream=None, ngram=(3, 1), max_seq_len=1 << 30,
                 slip=None):
    """The device loop of yalm_generate_speculative_sampled, state by state: (tokens, stats)."""
    assert slip is None or slip in SLIPS
    ctx = (list(context) if context else [token])[-S.HISTORY_CAP:]
    assert ctx[-1] == token and (slip or len(dev.kv) == pos)
    gen, n_gen = [0] * CAP, 0
    steps = accepted = plain = 0
    base = dev.carry if slip == "carry_u" else 0  # the slip: the last call's overshoot moved the stream on

    def uni(i):
        return u[min(max(i + base, 0), n - 1)]

    def feed(p, t):
        del dev.kv[p:]
        dev.kv.append(t)
        return logits_of(dev.kv)

    while n_gen < n:
        if pos + rows > max_seq_len:  # a plain step: one row, uniforms[n_gen]
            t = draw(feed(pos, token), uni(n_gen))
            gen[n_gen] = t
            n_gen, token, pos, plain = n_gen + 1, t, pos + 1, plain + 1
            continue
        hist = ctx + gen[:n_gen]
        d = S.stream_drafts(stream, n_gen, rows) if stream is not None else S.draft(hist, rows, *ngram)
        d = [x if 0 <= x < V else S.NONE for x in d]
        drawn = []
        for t in range(rows):
            l = feed(pos + t, token if t == 0 else (d[t - 1] if d[t - 1] != S.NONE else 0))
            k, p = (0, 1.0) if slip == "trunc_row0" and t > 0 else (TOP_K, TOP_P)
            drawn.append(draw(l, uni(n_gen if slip == "same_u" else n_gen + t), k, p))
        if slip == "same_row":
            a = S.accept(d, drawn[1:] + [S.NONE - 1])
        elif slip == "none_is_0":
            a = S.accept([0 if x == S.NONE else x for x in d], drawn)
        else:
            a = S.accept(d, drawn)
        for j in range(a):
            gen[n_gen + j] = drawn[j]
        n_gen += 1 if slip == "adv_1" else rows if slip == "adv_T" else a
        token, pos = drawn[a - 1], pos + a
        steps, accepted = steps + 1, accepted + a - 1
    over = n_gen - n
    dev.carry = over
    del dev.kv[pos - over:]  # spec_fix_kernel: the device continues at pos + n
    return gen[:n], {"spec_steps": steps, "accepted_drafts": accepted - over, "plain_steps": plain}


PROMPT = [3, 17, 41, 5, 22, 9]


def _streams(seq):
    return {
        "ngram": None,
        "right": list(seq),
        "wrong": [(t + 1) % V for t in seq],
        "third": [(t + 1) % V if j % 3 == 2 else t for j, t in enumerate(seq)],
    }


def _cases():
    """name -> (logits function, calls [(n, ...)], rows, stream kind, max_seq_len)."""
    out = {}
    for rows in (2, 3, 4):
        for kind in ("ngram", "right", "wrong", "third"):
            out[f"rows{rows}-{kind}"] = dict(rows=rows, kind=kind, calls=[30])
    out["window-right"] = dict(rows=4, kind="right", calls=[30], max_seq_len=24)  # crosses into plain steps
    out["window-ngram"] = dict(rows=3, kind="ngram", calls=[30], max_seq_len=24)
    out["chunks-right"] = dict(rows=4, kind="right", calls=[5, 7, 6])  # every call's last step overshoots
    out["zeros-none"] = dict(rows=4, kind="empty", calls=[24], zero_bias=7.0)  # no drafts, draws of token 0
    return out


CASES = _cases()


def run_case(name, slip=None):
    """((tokens, stats per call) of the model, (tokens, stats per call) expected)."""
    c = CASES[name]
    rows, calls, msl = c["rows"], c["calls"], c.get("max_seq_len", 1 << 30)
    logits_of = functools.partial(toy_logits, seed=1, zero_bias=c.get("zero_bias", 0.0))
    total = sum(calls)
    u = np.random.default_rng(42).random(total, dtype=np.float32)
    seq = plain_sampled(logits_of, PROMPT, total + 4, np.r_[u, np.full(4, 0.5, np.float32)])
    dev = Device(PROMPT)
    got, want = [], []
    token, pos, ctx, done = PROMPT[-1], len(PROMPT) - 1, list(PROMPT), 0
    for n in calls:
        rest = seq[done:]
        stream = [] if c["kind"] == "empty" else _streams(rest[:n])[c["kind"]]
        uc = u[done:done + n]
        got.append(spec_sampled(dev, logits_of, token, pos, n, rows, uc, context=ctx, stream=stream, max_seq_len=msl,
                                slip=slip))
        _, st, _ = S.predict(rest, token, n, rows, ngram_max=3, ngram_min=1, context=ctx, stream=stream, pos=pos,
                             max_seq_len=msl, vocab=V)
        want.append((rest[:n], st))
        token, pos, ctx, done = rest[n - 1], pos + n, ctx + rest[:n], done + n
    return got, want


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_reproduces_the_plain_sampled_sequence(name):
    got, want = run_case(name)
    assert got == want
    if name.startswith("window"):
        assert got[0][1]["plain_steps"] > 0 and got[0][1]["spec_steps"] > 0
    if name == "chunks-right":  # the requests are no multiples of the rows: the last steps overshoot
        assert all(st["spec_steps"] * 4 > n for (_, st), n in zip(got, CASES[name]["calls"]))
    if name == "zeros-none":
        assert sum(t == 0 for t in got[0][0]) > 4 and got[0][1]["accepted_drafts"] == 0
    if name == "rows4-ngram":
        assert got[0][1]["accepted_drafts"] > 0  # the toy sequence repeats enough for the drafter to hit


def test_sequence_is_a_sampled_one():
    got, _ = run_case("rows4-right")
    toks = got[0][0]
    greedy = plain_sampled(functools.partial(toy_logits, seed=1), PROMPT, 30, np.zeros(30, np.float32))
    assert len(set(toks)) > 4 and toks != greedy


# the slip -> a case that sees it (tokens or step counts differ from the plain sequence's)
SEEN_BY = {
    "same_u": "rows4-right",      # an accepted row drawn with row 0's uniform
    "adv_1": "rows4-right",       # accepted tokens overwritten by the next step's
    "adv_T": "rows4-wrong",       # rejected rows leave holes in the output
    "same_row": "rows4-right",    # right drafts are compared with the token after them
    "none_is_0": "zeros-none",    # a row without a draft counted as accepted when the draw is token 0
    "trunc_row0": "rows4-right",  # rows 1.. draw from the whole vocabulary
    "carry_u": "chunks-right",    # the second call's first draw reads its uniform `overshoot` places on
}


@pytest.mark.parametrize("slip", SLIPS)
def test_each_slip_is_seen(slip):
    assert set(SEEN_BY) == set(SLIPS)
    name = SEEN_BY[slip]
    got, want = run_case(name, slip)
    assert got != want, f"the slip {slip} went unseen by case {name}"
    seen = [n for n in sorted(CASES) if (lambda g, w: g != w)(*run_case(n, slip))]
    print(f"{slip}: seen by {seen}")


# ------------------------------------------------------------------ names
def _declared():
    src = open(os.path.join(ROOT, "include", "yalm_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_new_names_in_header_library_and_binding():
    from yalm_amd import runtime

    src = _declared()
    out = subprocess.run(["nm", "-D", "--defined-only", runtime.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in ("yalm_generate_speculative_sampled", "yalm_spec_sample_rows"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in runtime.EXPORTED and hasattr(runtime.lib, name)
    assert callable(runtime.spec_sample_rows) and callable(runtime.Decoder.generate_speculative_sampled)
    full = open(os.path.join(ROOT, "include", "yalm_hip.h")).read()
    assert re.search(r"tokens are\s+\*?\s*yalm_generate_sampled's for the same uniforms", full)
    assert "different orders" in full  # the caveat


def test_cli_usage_lists_sampled_speculation():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(HOST, "yalm")], capture_output=True)
    assert r.returncode == 1
    usage = r.stderr.decode()
    m = re.search(r"^\s*-s <int>.*?(?=^\s*Choose one)", usage, re.M | re.S)
    assert m and "-t 0" in m.group(0) and "-k" in m.group(0) and "-p" in m.group(0), usage
