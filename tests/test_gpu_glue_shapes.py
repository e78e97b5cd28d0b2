"""The caller-glue kernels and the greedy tail of csrc/cc_glue.hip — cc_add_rmsnorm, cc_qkv_rope, cc_silu_mul, cc_softmax_argmax —
against the references of tests/glue_ref.py (held to the oracle's twins and shown to have teeth by tests/test_glue_ref_host.py):
bit patterns where the arithmetic is exact, the derived band of glue_ref's docstring where the device evaluates rsqrtf / expf /
v_exp_f32 or sums in its own order.  The library is called through raw pointers (compact_ref.run_device): each tensor of a call
lives inside a larger device buffer pre-filled with a sentinel (NaN, -7, 0xAB); margins must survive, inputs must come back
unchanged, outputs the contract does not write must still hold the sentinel, the return code is checked.

  a. every case of glue_ref.CASES: the smallest shapes that reach each path (a single vector, an idle part of a wave, the register
     cap; nvec == 0 and scalar tails; the reload branch of the softmax above V = 131072; the second grid-stride pass of cc_qkv_rope
     and cc_silu_mul), structured inputs, known answers, the -inf table;
  b. three greedy tails back to back on one workspace;
  c. the refusal table;
  d. generate() with a ban over whole softmax slices.

Each banded test reports the worst observed error as a fraction of its delta (the smallest rung of glue_ref.LADDER whose scaled band
still holds every output) through `audit`; above 1 the comparison has failed."""
import argparse
import ctypes as C

import pytest
import torch

import compact_ref as R
import glue_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, HF = R.F32, R.BF, R.HF


def _run(c):
    rc, got = G.run_device(c)
    assert rc == 0, f"{c.id}: device -> {rc}"
    bad = G.verdict(c, got)
    assert bad is None, bad
    return got


def _select(op, dt, pick=lambda c: True):
    return [c for c in G.CASES[op]() if c.dtype == dt and pick(c)]


def _report(audit, op, dt, worst):
    audit(f"{op} {R.DT_NAME[dt]}: worst observed error <= {worst:g} of delta")


# ------------------------------------------------------------------------------------------------ a. every case
@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_add_rmsnorm_shapes(audit, dt):
    worst = 0.0
    for c in _select("add_rmsnorm", dt):
        got = _run(c)
        worst = max(worst, G.fraction_of_delta(c, got))
    _report(audit, "add_rmsnorm", dt, worst)


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_qkv_rope_shapes(dt):
    cases = _select("qkv_rope", dt)
    assert sum(R.passes(c.T * (c.HQ + 2 * c.H) * c.D // 2, G.CAP_ROPE) == 2 for c in cases) == 1
    for c in cases:
        _run(c)


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_silu_mul_shapes(audit, dt):
    worst = 0.0
    cases = _select("silu_mul", dt)
    assert sum(R.passes(c.n // G.vec(dt), G.CAP_SILU) == 2 for c in cases) == 1
    for c in cases:
        got = _run(c)
        if c.n < 1 << 20:  # (the ladder costs seven references: not on the second-pass case)
            worst = max(worst, G.fraction_of_delta(c, got))
    _report(audit, "silu_mul", dt, worst)


@pytest.mark.parametrize("dt", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_softmax_argmax_random_logits(audit, dt):
    from cold_compress_amd import _abi

    assert int(_abi.lib()["cc_softmax_argmax_workspace_bytes"]()) == G.WS_BYTES
    worst = 0.0
    for c in G.cases_softmax_random():
        if c.dtype == dt:
            got = _run(c)
            worst = max(worst, G.fraction_of_delta(c, got))
    _report(audit, "softmax_argmax", dt, worst)


def test_softmax_argmax_dominated_and_equal_maxima():
    n = 0
    for c in G.cases_softmax_maxima():
        got = _run(c)
        assert int(got["idx"][0]) == c.token
        n += 1
    assert n > 60


def test_softmax_argmax_inf_table():
    """-inf (one, whole slices, every second slice), the known answers, NaN and +inf.  Every case runs; the failures are listed
    together."""
    bad = []
    for c in G.cases_softmax_inf():
        rc, got = G.run_device(c)
        assert rc == 0, c.id
        bad.append(G.verdict(c, got))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ b. one workspace, no synchronisation
def test_three_greedy_tails_back_to_back_on_one_workspace():
    """(bf16, 128256), (f32, 1025), (f16, 151936) launched one after the other on ONE workspace with nothing between them: the
    second call's first kernel re-arms the key and the ticket the first call's last workgroup used."""
    from cold_compress_amd import _abi

    lib = _abi.lib()
    ws = torch.full((G.WS_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    cases = [G.sm_case(dt, V, G._logits(V, 3, "chain", i), f"chain{i}") for i, (dt, V) in enumerate(((BF, 128256), (F32, 1025), (HF, 151936)))]
    dev = [(c.t["logits"].to(DEV), torch.full((c.V,), float("nan"), dtype=c.dtype, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV))
           for c in cases]
    torch.cuda.synchronize()
    for c, (x, p, i) in zip(cases, dev):
        rc = lib["cc_softmax_argmax"](C.c_void_p(x.data_ptr()), c.V, c.code, C.c_void_p(p.data_ptr()), C.c_void_p(i.data_ptr()),
                                      C.c_void_p(ws.data_ptr()), G.WS_BYTES, None)
        assert rc == 0
    torch.cuda.synchronize()
    for c, (x, p, i) in zip(cases, dev):
        bad = G.verdict(c, dict(probs=p.cpu(), idx=i.cpu()))
        assert bad is None, bad


# ------------------------------------------------------------------------------------------------ c. refusals
def test_refusals_leave_every_output_untouched():
    table = G.refusals()
    assert len(table) >= 36
    for what, c, want_rc, _ in table:
        rc, got = G.run_device(c)
        assert rc == want_rc, f"{what}: device -> {rc}"
        for n, g in got.items():
            assert R.same(g, c.t[n]), f"{what}: '{n}' was written"


# ------------------------------------------------------------------------------------------------ d. the harness
def test_greedy_generate_with_whole_slices_banned_matches_eager_torch(monkeypatch):
    """The tiny model (V = 128: slices of 8 ids) decoding greedily with ids 8..31 banned by LogitPenalties — three whole slices of
    -inf in every row: the same tokens and rows as the loop whose greedy tail is torch.softmax + torch.argmax."""
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import CONFIGS, LogitPenalties, ModelArgs, Transformer, decode_one_token, generate, glue, prefill, setup_caches

    torch.manual_seed(3)
    model = Transformer(ModelArgs(**CONFIGS["tiny"])).to(torch.bfloat16).eval().to(DEV)
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=["recent_global"], prompt_compression_strategy=["recent_global"], max_cache_length=[32], global_tokens=4)
    setup_caches(model, None, DEV, 64, dict(kw))
    V = model.config.vocab_size
    assert G.slice_len(V) == 8
    prompt = torch.randint(32, V, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    ban = {i: -float("inf") for i in range(8, 32)}

    def run():
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, rows, _ = generate(model, prompt, prefill, decode_one_token, max_new_tokens=12, penalties=LogitPenalties(V, DEV, 1.0, 0.0, 0.0, ban))
        torch.cuda.synchronize()
        return seq.cpu(), [r.cpu() for r in rows]

    native = run()

    def eager(logits):
        probs = torch.softmax(logits, dim=-1)
        return probs, torch.argmax(probs, keepdim=True).to(torch.int32)

    monkeypatch.setattr(glue, "softmax_argmax", eager)
    torch_path = run()
    new = native[0][len(prompt):].tolist()
    assert new == torch_path[0][len(prompt):].tolist() and not set(new) & set(ban)
    assert len(native[1]) == len(torch_path[1]) > 0
    for a, b in zip(native[1], torch_path[1]):
        assert not bool(torch.isnan(a).any()) and bool((a[8:32] == 0).all())
        assert float((a.float() - b.float()).abs().max()) <= 2.0 ** -8 * float(b.float().max())
