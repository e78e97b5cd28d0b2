"""Shared by tests/test_gpu_logits_streams.py and tests/test_logits_streams_host.py.  A helper, not a test: rows with NaN padding,
count tables at aligned and misaligned bases, one sequence's penalty state and one sequence's rules and history as the two streams
entry points take them (raw calls through ctypes, so that refused calls can be made at all), and the table of refusals."""
import ctypes as C

import torch

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
VS = [1, 5, 8, 129, 4099]
OK, BAD, UNSUPPORTED = 0, -1, -2
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if dev == "cuda" else None


def _rows(T, V, stride, dtype, dev, g):
    """[T, stride] with NaN behind the V elements of every row; the rows hold both signs, zeros of both signs, an infinity and a NaN"""
    buf = torch.full((T, stride), NAN, dtype=dtype)
    x = torch.randn(T, V, generator=g) * 4
    x[:, ::7] = 0.0
    x[:, 3::11] = -0.0
    if V > 4:
        x[0, 2], x[-1, 4], x[-1, 1] = float("inf"), -float("inf"), NAN
    buf[:, :V] = x.to(dtype)
    return buf.to(dev)


def _table(values, misaligned):
    """a contiguous tensor of `values` whose base is 16-byte aligned, or 4 bytes past such a base"""
    big = torch.zeros(values.numel() + 8, dtype=values.dtype, device=values.device)
    off = 4 - (big.data_ptr() % 16) // 4 if big.data_ptr() % 16 else 0
    view = big[off + (1 if misaligned else 0):][:values.numel()]
    view.copy_(values)
    assert (view.data_ptr() % 16 == 0) != misaligned
    return view


class PenState:
    def __init__(self, V, dev, g, gen_start, r, f, p, biased, misaligned):
        i32 = lambda: _table(torch.randint(0, 3, (V,), generator=g, dtype=torch.int32).to(dev), misaligned)  # noqa: E731
        self.prompt_count, self.gen_count = i32(), i32()
        self.gen_start = torch.tensor([gen_start], dtype=torch.int32, device=dev)
        self.r, self.f, self.p = r, f, p
        self.bias = None
        if biased:
            b = torch.randn(V, generator=g)
            b[V // 2] = -float("inf")
            self.bias = _table(b.to(dev), misaligned)

    def clone(self):
        o = object.__new__(PenState)
        o.__dict__.update(self.__dict__)
        mis = self.prompt_count.data_ptr() % 16 != 0
        o.prompt_count, o.gen_count = _table(self.prompt_count, mis), _table(self.gen_count, mis)
        return o

    def record(self):
        from cold_compress_amd import _abi

        return _abi.PenaltyRow(self.prompt_count.data_ptr(), self.gen_count.data_ptr(), self.gen_start.data_ptr(),
                               None if self.bias is None else self.bias.data_ptr(), self.r, self.f, self.p)


def pen_streams(x, out, T, V, stride, dtype, states, tokens, pos, dev="cuda"):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    recs = (_abi.PenaltyRow * max(len(states), 1))()
    for t, s in enumerate(states):
        if s is not None:
            recs[t] = s.record() if hasattr(s, "record") else s
    return _abi.lib()["cc_logits_penalize_streams"](_ptr(x), _ptr(out), T, V, stride, glue._DT.get(dtype, dtype), recs, _ptr(tokens), _ptr(pos),
                                                    _stream(dev))


PEN_SETTINGS = [(1.3, 0.4, 0.2, True), (0.7, 0.0, -0.5, False), (1.0, 1.25, 0.0, True), (2.0, -0.3, 0.1, False)]  # r, f, p, biased
GEN_STARTS = [5, 7, 0, 1000]


# ---------------------------------------------------------------------------------------------------------------- constraints


class ConState:
    """one sequence's rules and history: hist is periodic (period 5 over the ids 0 .. 4, so that n-grams up to 32 repeat) with a few
    ids outside every vocabulary, and holds a sentinel where the launch is to store the row's token"""

    def __init__(self, cap, dev, p, token, gen_start, ngram=0, from_gen=False, m=0, terms=(), bad_words=()):
        h = torch.arange(cap, dtype=torch.int32) % 5
        h[1], h[min(2, cap - 1)] = -1, 1 << 20
        self.host = h.tolist()
        if token is not None and 0 <= p < cap:
            self.host[p] = token
            h[p] = 424242  # (never read by the launch: the position's token is taken from `tokens`)
        self.hist = h.to(dev)
        self.cap, self.p, self.gen_start_host = cap, p, gen_start
        self.gen_start = torch.tensor([gen_start], dtype=torch.int32, device=dev)
        self.ngram, self.from_gen, self.m, self.terms_host, self.bad_words = ngram, from_gen, m, list(terms), [list(w) for w in bad_words]
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
        self.terms = i32(self.terms_host) if terms else None
        self.bw_tokens = i32([v for w in self.bad_words for v in w]) if bad_words else None
        offs = [0]
        for w in self.bad_words:
            offs.append(offs[-1] + len(w))
        self.bw_offsets = i32(offs) if bad_words else None

    def clone(self):
        o = object.__new__(ConState)
        o.__dict__.update(self.__dict__)
        o.hist = self.hist.clone()
        return o

    def record(self):
        from cold_compress_amd import _abi

        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return _abi.ConstraintRow(self.hist.data_ptr(), self.cap, self.gen_start.data_ptr(), self.ngram, int(self.from_gen), self.m, ptr(self.terms),
                                  len(self.terms_host), ptr(self.bw_tokens), ptr(self.bw_offsets), len(self.bad_words))

    def banned(self, V):
        """the ids of [0, V) that the row's rules ban together, sorted (the harness's plain-Python contract)"""
        from cold_compress_amd.harness.constraints import _banned

        if not 0 <= self.p < self.cap:
            return []
        ban = _banned(self.host[:self.p + 1], self.p, self.gen_start_host, self.ngram, self.from_gen, self.m, self.terms_host, self.bad_words)
        return sorted(w for w in ban if 0 <= w < V)

    def hits(self, V):
        """per rule the number of elements of [0, V) that the rule alone bans for this row (the harness's plain-Python contract)"""
        from cold_compress_amd.harness.constraints import _banned

        if not 0 <= self.p < self.cap:
            return {}
        s, gs = self.host[:self.p + 1], self.gen_start_host
        inside = lambda ban: len([w for w in ban if 0 <= w < V])  # noqa: E731
        out = {}
        if self.ngram:
            out[f"ngram{self.ngram}-{'gen' if self.from_gen else 'all'}"] = inside(_banned(s, self.p, gs, self.ngram, self.from_gen, 0, [], []))
        if self.m:
            out["min_new_tokens"] = inside(_banned(s, self.p, gs, 0, False, self.m, self.terms_host, []))
        for w in self.bad_words:
            out[f"bad_words{len(w)}"] = inside(_banned(s, self.p, gs, 0, False, 0, [], [w]))
        return out


def con_streams(x, out, T, V, stride, dtype, states, tokens, pos, dev="cuda"):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    recs = (_abi.ConstraintRow * max(len(states), 1))()
    for t, s in enumerate(states):
        if s is not None:
            recs[t] = s.record() if hasattr(s, "record") else s
    return _abi.lib()["cc_logits_constrain_streams"](_ptr(x), _ptr(out), T, V, stride, glue._DT.get(dtype, dtype), recs, _ptr(tokens), _ptr(pos),
                                                     _stream(dev))


def _rules(k, p, V):
    """the k-th rule set for a row at position p: n-gram sizes 1, 2, 3 and 32 in both scopes, a minimum length, banned sequences of
    lengths 1 and 3 (the longer one is the periodic history's own continuation, so that it matches)"""
    nxt = [(p - 1) % 5, p % 5, (p + 1) % 5]  # s[p-1], s[p] and what the pattern continues with
    return [dict(ngram=2), dict(ngram=1, from_gen=True, m=4, terms=[0, V - 1, V + 3, -1]), dict(ngram=3, bad_words=[[0], nxt]),
            dict(ngram=32), dict(ngram=2, from_gen=True, bad_words=[[V - 1]]), dict(ngram=3, from_gen=True, m=1000, terms=[0]),
            dict(ngram=32, from_gen=True), dict(ngram=1)][k % 8]


RULE_NAMES = {f"ngram{n}-{sc}" for n in (1, 2, 3, 32) for sc in ("all", "gen")} | {"min_new_tokens", "bad_words1", "bad_words3"}


def con_cases(cap, dev):
    """The calls of the constraints comparison for a history of `cap` positions: every V of VS, T = 1 .. 4, out of place and in place,
    with tokens and without; per row an unrelated position (0, 5, 1023, 1024, cap - 1, one past the history, ..), a rule set, a
    gen_start in front of, near or behind the row, and a token that continues the pattern or lies outside the vocabulary — drawn from
    a seeded generator.  -> dicts of V, T, stride, inplace, ps (positions), toks (or None), states (row 1 of T >= 3 is None)."""
    import random

    positions = [0, 5, 1023, 1024, cap - 1, cap + 3, 40, 2100 if cap > 2100 else 17]  # (1023 / 1024 lie past a history of 64)
    rnd = random.Random(cap)
    k = 0
    for V in VS:
        for T in (1, 2, 3, 4):
            for inplace, with_tokens in ((False, True), (True, True), (True, False)):
                k += 1
                ps = [positions[(k + 3 * t) % len(positions)] for t in range(T)]
                toks = [[p % 5, p % 5, p % 5, -1, V][rnd.randrange(5)] for p in ps] if with_tokens else None
                states = []
                for t, p in enumerate(ps):
                    gs = [0, 0, max(p - 40, 0), p + 2, max(p - 3, 0)][rnd.randrange(5)]  # (p + 2: the row sits in front of its gen_start)
                    rule = rnd.randrange(8)
                    if 36 <= p < cap and rnd.randrange(2):  # a history long enough for a 32-gram to repeat: the two rules of that size
                        rule = (3, 6)[rnd.randrange(2)]
                    states.append(ConState(cap, dev, p, toks[t] if with_tokens else None, gs, **_rules(rule, p, V)))
                if T >= 3:
                    states[1] = None  # a NULL-state row in the middle
                yield dict(V=V, T=T, stride=V + (k % 2) * 3, inplace=inplace, ps=ps, toks=toks, states=states)


def con_hits(cap):
    """per rule the number of elements that the rule alone bans over all rows of con_cases(cap): on the host, no device needed"""
    hits = {}
    for c in con_cases(cap, "cpu"):
        for s in c["states"]:
            if s is not None:
                for rule, n in s.hits(c["V"]).items():
                    hits[rule] = hits.get(rule, 0) + n
    return hits


# ---------------------------------------------------------------------------------------------------------------- refusals


def _refusals(dev):
    """(what, call -> code, expected code, tensors that must stay as they are) for both entry points; nothing is launched"""
    from cold_compress_amd import _abi

    V, T, dt = 8, 2, torch.float32
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    x, out = torch.randn(T, V).to(dev), torch.zeros(T, V, device=dev)
    tokens, pos = i32([1, 2]), i32([3, 4])
    g = torch.Generator().manual_seed(1)
    a, b = (PenState(V, dev, g, 2, 1.2, 0.1, 0.1, True, False) for _ in range(2))
    keep = [x, out, tokens, pos, a.prompt_count, a.gen_count, b.prompt_count, b.gen_count]
    cases = []

    def pen(what, code, states=None, **kw):
        args = dict(x=x, out=out, T=T, V=V, stride=V, dtype=dt, states=[a, b] if states is None else states, tokens=tokens, pos=pos, dev=dev)
        args.update(kw)
        cases.append(("penalize: " + what, lambda: pen_streams(**args), code))

    def rec(s, **kw):
        r = s.record()
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    odd = lambda t: C.c_void_p(t.data_ptr() + 2)  # noqa: E731

    class Raw:  # (a pointer that is not a tensor's base)
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p

    for T_bad in (0, 5, -1):
        pen(f"T = {T_bad}", BAD, T=T_bad, states=[a, b, None, None, None][:max(T_bad, 1)])
    pen("V = 0", BAD, V=0)
    pen("row_stride < V", BAD, stride=V - 1)
    pen("NULL logits", BAD, x=None)
    pen("NULL out", BAD, out=None)
    pen("tokens without pos", BAD, pos=None)
    pen("out overlapping logits", BAD, out=Raw(x.data_ptr() + 4 * V))
    pen("misaligned logits", BAD, x=Raw(x.data_ptr() + 2))
    pen("misaligned tokens", BAD, tokens=Raw(tokens.data_ptr() + 2))
    pen("a dtype that is none of the three", UNSUPPORTED, dtype=7)
    for k, v in (("gen_count", None), ("gen_start", None), ("r", 0.0), ("r", -1.0), ("r", NAN), ("r", float("inf")), ("f", NAN), ("f", float("inf")),
                 ("p", -float("inf")), ("prompt_count", a.prompt_count.data_ptr() + 2), ("bias", a.bias.data_ptr() + 1)):
        pen(f"record 1 with {k} = {v}", BAD, states=[a, rec(b, **{k: v})])
    pen("two records with one prompt_count", BAD, states=[a, rec(b, prompt_count=a.prompt_count.data_ptr())])
    pen("two records with one gen_count", BAD, states=[a, rec(b, gen_count=a.gen_count.data_ptr())])
    pen("one table as prompt_count here and gen_count there", BAD, states=[a, rec(b, gen_count=a.prompt_count.data_ptr())])
    pen("the same record twice", BAD, states=[a, a])

    ca, cb = ConState(64, dev, 3, 1, 2, ngram=2, m=2, terms=[1], bad_words=[[1, 2]]), ConState(64, dev, 4, 2, 2, ngram=2, m=2, terms=[1], bad_words=[[3]])
    keep += [ca.hist, cb.hist]

    def con(what, code, states=None, **kw):
        args = dict(x=x, out=out, T=T, V=V, stride=V, dtype=dt, states=[ca, cb] if states is None else states, tokens=tokens, pos=pos, dev=dev)
        args.update(kw)
        cases.append(("constrain: " + what, lambda: con_streams(**args), code))

    for T_bad in (0, 5, -1):
        con(f"T = {T_bad}", BAD, T=T_bad, states=[ca, cb, None, None, None][:max(T_bad, 1)])
    con("V = 0", BAD, V=0)
    con("row_stride < V", BAD, stride=V - 1)
    con("NULL logits", BAD, x=None)
    con("NULL out", BAD, out=None)
    con("NULL pos", BAD, pos=None)
    con("out overlapping logits", BAD, out=Raw(x.data_ptr() + 4 * V))
    con("misaligned pos", BAD, pos=Raw(pos.data_ptr() + 2))
    con("a dtype that is none of the three", UNSUPPORTED, dtype=7)
    con("a bad argument is named before the dtype", BAD, dtype=7, V=0)
    for k, v in (("cap", 0), ("cap", -3), ("gen_start", None), ("ngram", -1), ("ngram", 33), ("min_new_tokens", -1), ("n_term", -1), ("n_term", 65),
                 ("term_ids", None), ("n_bw", -1), ("n_bw", 1025), ("bw_tokens", None), ("bw_offsets", None), ("hist", cb.hist.data_ptr() + 2)):
        con(f"record 1 with {k} = {v}", BAD, states=[ca, rec(cb, **{k: v})])
    con("two records sharing one hist", BAD, states=[ca, rec(cb, hist=ca.hist.data_ptr())])
    con("the same record twice", BAD, states=[ca, ca])
    assert isinstance(_abi.PenaltyRow(), C.Structure)
    return cases, keep


def _check_refusals(dev):
    cases, keep = _refusals(dev)
    before = [t.clone() for t in keep]
    for what, call, code in cases:
        assert call() == code, what
    if dev == "cuda":
        torch.cuda.synchronize()
    for t, b in zip(keep, before):
        assert torch.equal(_bits(t), _bits(b))
    assert len(cases) > 50
