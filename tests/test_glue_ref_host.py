"""CPU checks of tests/glue_ref.py, the references tests/test_gpu_glue_shapes.py holds the glue kernels and the greedy tail to:
every case's oracle twin lies inside the reference (bit for bit on the exact parts), the 2 % condition on open bands, the launcher
constants against their source lines, the known answers against CPU torch, the refusal table against the twins, and TEETH: wrong
variants of every kernel, written out as numpy, each of which the case list must reject.

Where the twin is expected to differ from the device: it sums in double and calls the host's libm (inside the band all the same),
and it knows neither vector widths, nor the register cap of cc_add_rmsnorm, nor a workspace — see glue_ref.refusals()."""
import os

import numpy as np
import pytest
import torch

import compact_ref as R
import glue_ref as G

F32, BF, HF = R.F32, R.BF, R.HF
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cold_compress_amd", "csrc")


@pytest.fixture(scope="module")
def cases():
    """every case once (the generators are deterministic; the tensors are never written)."""
    return {op: list(gen()) for op, gen in G.CASES.items()}


def test_launcher_constants_are_the_source_lines():
    for fname, lines in G.MIRRORED_LINES.items():
        src = " ".join(open(os.path.join(CSRC, fname)).read().split())
        for line in lines:
            assert " ".join(line.split()) in src, f"{fname} no longer contains: {line}"
    assert G.WS_BYTES == G.SM_BLOCKS * 8 + 8 + 4 + 4  # float2 part[128]; key; ticket; padding to the key's alignment


def test_case_list_reaches_every_listed_path(cases):
    norm = cases["add_rmsnorm"]
    for dt in R.DTYPES:
        v = G.vec(dt)
        assert {c.dim for c in norm if c.dtype == dt} == {n * v for n in G.NORM_DIMS} and max(G.NORM_DIMS) == G.NORM_THREADS * G.NORM_MAX_VEC
        assert {(c.T, c.t["delta"] is None) for c in norm if c.dtype == dt} == {(T, d) for T in G.NORM_T for d in (True, False)}
        assert {c.n for c in cases["silu_mul"] if c.dtype == dt} >= {1, v - 1, v, v + 1, 256 * v + 3, G.silu_second_pass_n(dt)}
        n = G.silu_second_pass_n(dt)
        assert R.passes(n // v, G.CAP_SILU) == 2 and n % v == v - 1
        assert {(c.T, c.HQ, c.H, c.D) for c in cases["qkv_rope"] if c.dtype == dt} >= set(G.ROPE_SHAPES) | {G.ROPE_SECOND_PASS}
        assert {c.V for c in cases["softmax_argmax"] if c.dtype == dt and "sigma" in c.id} == set(G.SM_V)
    T, HQ, H, D = G.ROPE_SECOND_PASS
    assert R.passes(T * (HQ + 2 * H) * D // 2, G.CAP_ROPE) == 2 and max(R.passes(t * (q + 2 * h) * d // 2, G.CAP_ROPE) for t, q, h, d in G.ROPE_SHAPES) == 1
    assert G.slice_len(131072) == G.SM_REGS * G.SM_THREADS < G.slice_len(131080)  # the threshold of the reload branch
    ids = [c.id for c in cases["softmax_argmax"]]
    assert len(set(ids)) == len(ids)
    for word in ("reload-first", "tie-slices", "tie-256-apart", "slice-first", "slice-last", "special-tokens-inf", "every-second-slice-inf"):
        assert any(word in i for i in ids), word
    assert G.slice_len(128256) * 127 == 128016 and G.slice_len(1024) == 8  # the slices the issue names


# ------------------------------------------------------------------------------------------------ twin inside the reference
@pytest.mark.parametrize("op", sorted(G.CASES))
def test_oracle_twin_lies_inside_the_reference_and_bands_stay_closed(oracle, cases, op):
    worst = 0.0
    for c in cases[op]:
        rc, got = G.run_oracle(oracle, c)
        assert rc == 0, f"{c.id}: oracle -> {rc}"
        bad = G.verdict(c, got)
        assert bad is None, bad
        for n, (lo, hi, *_) in G.reference(c).items():
            share = G.open_share(lo, hi)
            if n != G.BANDED.get(op):
                assert share == 0.0, f"{c.id}: '{n}' is an exact output"
            elif c.dtype != F32:
                if lo.numel() >= 50:  # (below 50 elements 2 % is less than one element: ONE open element is let through there)
                    worst = max(worst, share)
                assert share <= G.OPEN_SHARE_MAX or share * lo.numel() < 1.5, f"{c.id}: {share:.4f} of '{n}' has an open band"
    print(f"{op}: largest open-band share of a 16-bit case {worst:.5f}")


def test_silu_special_points_are_exact_in_the_reference(cases):
    for c in cases["silu_mul"]:
        if hasattr(c, "exact_np"):
            lo, hi = G.reference(c)["out"]
            assert G.special_ok(c, lo) and G.special_ok(c, hi), c.id


def test_softmax_known_answers_are_cpu_torch(cases):
    """one finite logit -> exactly (1, 0, ...); all -inf, a +inf, a NaN (also in a slice of -inf) -> all NaN and torch.argmax 0."""
    n = 0
    for c in cases["softmax_argmax"]:
        if not hasattr(c, "exact"):
            continue
        x = c.t["logits"]
        p = torch.softmax(x.float(), dim=-1).to(c.dtype)
        want = c.exact["probs"]
        assert bool(torch.isnan(p).all()) if bool(torch.isnan(want).all()) else R.same(p, want), c.id
        assert int(torch.argmax(p)) == c.token == G.token_of(p), c.id
        n += 1
    assert n == 10
    c = next(c for c in cases["softmax_argmax"] if "near-tie" in c.id)
    lo, hi = G.reference(c)["probs"][:2]
    assert R.same(lo[[10, 500]], hi[[10, 500]]) and float(lo[10]) == float(lo[500]) and float(c.t["logits"][500]) > float(c.t["logits"][10])


# ------------------------------------------------------------------------------------------------ teeth
def _norm_wrong(c, kind):
    dt = c.dtype
    h = G.f32(c.t["x"])
    out = {}
    if c.t["delta"] is not None and kind != "ignores delta":
        h = G.rnd(h + G.f32(c.t["delta"]), dt)
    if c.t["delta"] is not None and c.t["h_out"] is not None:
        out["h_out"] = G.tens(h, dt)
    elif c.t["h_out"] is not None:
        out["h_out"] = c.t["h_out"]
    h64 = h.astype(np.float64)
    sq = h64 * h64
    if kind == "drops the last register vector":
        sq = sq[:, : (G.NORM_MAX_VEC - 1) * G.NORM_THREADS * G.vec(dt)]
    count = c.dim - 1 if kind == "divides by the wrong count" else c.dim
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = (1.0 / np.sqrt(sq.sum(axis=1, keepdims=True) / count + (0.0 if kind == "omits eps" else np.float64(np.float32(c.eps))))).astype(np.float32)
        t = h * rs
        if kind != "skips the intermediate rounding":
            t = G.rnd(t, dt)
        w = G.f32(c.t["w"])
        w = w[np.arange(c.T) % c.dim][:, None] if kind == "indexes the weight by row" else w[None]
        out["out"] = G.tens(t * w, dt)
    return out


def _rope_wrong(c, kind):
    dt, T, HQ, H, D = c.dtype, c.T, c.HQ, c.H, c.D
    heads, half = HQ + 2 * H, D // 2
    x = G.f32(c.t["qkv"]).reshape(T, heads, D)
    f = G.f32(c.t["freqs"]).reshape(T, 1, half, 2)
    cs, sn = (f[..., 1], f[..., 0]) if kind == "swaps c and s" else (f[..., 0], f[..., 1])
    x0, x1 = (x[..., :half], x[..., half:]) if kind == "half-split pairs" else (x[..., 0::2], x[..., 1::2])
    if kind == "fuses a product into the add":
        o0 = (x0.astype(np.float64) * cs - (x1 * sn).astype(np.float64)).astype(np.float32)
        o1 = (x1.astype(np.float64) * cs + (x0 * sn).astype(np.float64)).astype(np.float32)
    else:
        o0, o1 = x0 * cs - x1 * sn, x1 * cs + x0 * sn
    rot = np.concatenate([o0, o1], -1) if kind == "half-split pairs" else np.stack([o0, o1], -1).reshape(T, heads, D)
    parts = dict(q=rot[:, :HQ], k=rot[:, HQ:HQ + H], v=rot[:, HQ + H:] if kind == "rotates V" else x[:, HQ + H:])
    if kind == "token-major output":
        return {n: G.tens(p, dt).reshape(p.shape[1], T, D) for n, p in parts.items()}
    return {n: G.tens(p.transpose(1, 0, 2), dt) for n, p in parts.items()}


def _silu_wrong(c, kind):
    dt = c.dtype
    a = G.f32(c.t["a"]).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = (a / (1.0 + np.exp(a))).astype(np.float32) if kind == "exp(+a)" else G.silu64(a).astype(np.float32)
        if kind != "rounds only once":
            s = G.rnd(s, dt)
        out = G.tens(s * G.f32(c.t["b"]), dt)
    if kind == "drops the tail":
        out[c.n // G.vec(dt) * G.vec(dt):] = float("nan")  # still the sentinel
    return dict(out=out)


def _softmax_wrong(c, kind):
    dt, V = c.dtype, c.V
    x = G.f32(c.t["logits"])
    per = G.slice_len(V)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "slice maximum (the kernel before the fix)":
            m = np.full(G.SM_BLOCKS, -np.inf, np.float32)
            s = np.zeros(G.SM_BLOCKS)
            for g in range(-(-V // per)):
                sl = x[g * per:(g + 1) * per]
                m[g] = np.fmax.reduce(np.concatenate([np.float32([-np.inf]), sl]))  # fmaxf skips NaN
                s[g] = np.exp((sl - m[g]).astype(np.float64)).sum()
            M = m.max()
            use = (s > 0) | np.isnan(s)
            S = (s[use] * np.exp((m[use] - M).astype(np.float64))).sum()
            p = np.exp((x - M).astype(np.float64)) / S
        else:
            M = np.fmax.reduce(x)
            e = np.exp((x - M).astype(np.float64))
            off = np.arange(V) % per
            S = e[(off < 4 * G.SM_THREADS) | (off >= 5 * G.SM_THREADS)].sum() if kind == "drops the fifth element per thread" else e.sum()
            p = e / S
    probs = G.tens(p.astype(np.float32), dt)
    tok = G.token_of(probs)
    if kind == "last index wins ties" and not bool(torch.isnan(probs).any()):
        tok = V - 1 - int(probs.float().numpy()[::-1].argmax())
    if kind == "argmax of unrounded probabilities" and not np.isnan(p).any():
        tok = int(p.argmax())
    return dict(probs=probs, idx=torch.tensor([tok], dtype=torch.int32))


WRONG = {
    "add_rmsnorm": (_norm_wrong, ("drops the last register vector", "omits eps", "divides by the wrong count", "skips the intermediate rounding",
                                  "indexes the weight by row", "ignores delta")),
    "qkv_rope": (_rope_wrong, ("swaps c and s", "fuses a product into the add", "token-major output", "rotates V", "half-split pairs")),
    "silu_mul": (_silu_wrong, ("drops the tail", "rounds only once", "exp(+a)")),
    "softmax_argmax": (_softmax_wrong, ("slice maximum (the kernel before the fix)", "last index wins ties", "argmax of unrounded probabilities",
                                        "drops the fifth element per thread")),
}


def _small(c):
    return "second-pass" not in c.id


@pytest.mark.parametrize("op", sorted(WRONG))
def test_the_case_list_rejects_every_wrong_variant(cases, op):
    fn, kinds = WRONG[op]
    for kind in kinds:
        rejected = [c.id for c in cases[op] if _small(c) and G.verdict(c, fn(c, kind)) is not None]
        assert rejected, f"{op}: a kernel that {kind} passes every case"
        print(f"{op}: '{kind}' rejected by {len(rejected)} cases")


def test_the_slice_maximum_bug_is_what_the_inf_cases_catch_and_nothing_else_does(cases):
    """the kernel as it stood before the fix (per-slice maximum: a slice of -inf gives exp(-inf + inf) = NaN) is rejected by exactly
    the cases that hold a whole slice of -inf in a row that has an answer."""
    kind = WRONG["softmax_argmax"][1][0]
    for c in cases["softmax_argmax"]:
        x = G.f32(c.t["logits"])
        per = G.slice_len(c.V)
        whole = any(bool((x[g * per:(g + 1) * per] == -np.inf).all()) for g in range(-(-c.V // per)))
        rejected = G.verdict(c, _softmax_wrong(c, kind)) is not None
        assert rejected == (whole and not G.poisoned(x)), c.id


# ------------------------------------------------------------------------------------------------ refusals
def test_refusal_table_against_the_oracle_twins(oracle):
    table = G.refusals()
    assert len(table) >= 36 and {rc for _, _, rc, _ in table} == {G.BAD_ARG, G.UNSUPPORTED, G.WORKSPACE}
    for what, c, _, twin_rc in table:
        rc, got = G.run_oracle(oracle, c)
        assert rc == twin_rc, f"{what}: oracle -> {rc}"
        if rc != G.OK:
            for n, g in got.items():
                assert R.same(g, c.t[n]), f"{what}: the oracle's twin touched '{n}'"
