"""Repetition / frequency / presence penalties and the logit bias on the host side (no GPU): the torch twin of cc_logits_penalize's
contract against an independent scalar restatement, the harness's CPU path of `LogitPenalties`, the ABI rows and the refusals, and
the generation loop with `penalties=` on the tiny model over tests/cpu_twin.py (neutral settings, a ban, the counts and their split,
forced blocks, the rewind, validation)."""
import argparse
import ctypes as C
import os
import re

import pytest
import torch

import penalty_twin as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731
VS = (1, 7, 8, 9, 255, 1025)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=_ID)
def test_the_twin_is_the_scalar_restatement(dtype):
    """Every family, V in (1, 7, 8, 9, 255, 1025), T = 1 .. 4 with all three penalties and a bias on (and no tokens at T = 1 of the
    smallest sizes); each penalty alone at V = 255, T = 4: rows and counts bit for bit, NaNs as a class."""
    cases = [(V, T, P.ALL_ON, True) for V in VS for T in (1, 2, 3, 4)] + [(255, 4, s, False) for s in P.SETTINGS[:-1]]
    for V, T, (r, f, p), with_bias in cases:
        pc, gc = P.counts(V)
        toks, pos = P.block_inputs(V, T)
        if V <= 8 and T == 1:
            toks = pos = None
        bias = P.bias_vec(V) if with_bias else None
        for name in P.FAMILIES:
            rows = P.family(name, dtype, V)[:T]
            out, cp, cg = P.twin(rows, pc, gc, P.GEN_START, toks, pos, r, f, p, bias)
            ref, rp, rg = P.scalar_restatement(rows, pc, gc, P.GEN_START, toks, pos, r, f, p, bias)
            assert P.same_bits(out.float(), torch.from_numpy(ref)), (name, V, T, r, f, p)
            assert out.dtype == dtype and cp.tolist() == rp and cg.tolist() == rg, (name, V, T)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=_ID)
def test_logit_penalties_on_cpu_tensors(dtype):
    """LogitPenalties.apply on CPU tensors is the twin bit for bit — rows and counts — over every family, after a reset that put a
    prompt and a generated tail into the counts; the input logits are left as they were."""
    from cold_compress_amd.harness import LogitPenalties

    for V in (7, 9, 255, 1025):
        g = torch.Generator().manual_seed(V)
        fed = torch.randint(0, V, (P.GEN_START + 9,), generator=g, dtype=torch.int32)
        for (r, f, p), with_bias in [(s, False) for s in P.SETTINGS] + [(P.ALL_ON, True)]:
            bias = P.bias_vec(V) if with_bias else None
            pen = LogitPenalties(V, "cpu", r, f, p, None if bias is None else {i: float(b) for i, b in enumerate(bias) if b != 0})
            for T in (1, 2, 3, 4):
                pen.reset(fed, P.GEN_START)
                assert pen.prompt_count.tolist() == torch.bincount(fed[:P.GEN_START].long(), minlength=V).tolist()
                assert pen.gen_count.tolist() == torch.bincount(fed[P.GEN_START:].long(), minlength=V).tolist()
                toks, pos = P.block_inputs(V, T)
                for name in P.FAMILIES:
                    rows = P.family(name, dtype, V)[:T]
                    keep = rows.clone()
                    pc, gc = pen.prompt_count.clone(), pen.gen_count.clone()
                    got = pen.apply(rows.unsqueeze(0), torch.tensor(toks, dtype=torch.int32), torch.tensor(pos, dtype=torch.int32))
                    want, cp, cg = P.twin(rows, pc, gc, P.GEN_START, toks, pos, pen.repetition_penalty, pen.frequency_penalty,
                                          pen.presence_penalty, bias)
                    assert got.shape == (1, T, V) and P.same_bits(got[0], want), (name, V, T, r, f, p)
                    assert torch.equal(pen.prompt_count, cp) and torch.equal(pen.gen_count, cg)
                    assert P.same_bits(rows, keep)
                got = pen.apply(rows.unsqueeze(0))  # no tokens: nothing is counted
                assert torch.equal(pen.prompt_count, cp) and torch.equal(pen.gen_count, cg)
                assert P.same_bits(got[0], P.twin(rows, cp, cg, P.GEN_START, None, None, pen.repetition_penalty, pen.frequency_penalty,
                                                  pen.presence_penalty, bias)[0])


def test_abi_surface_and_refusals():
    """Both symbols are in the header and in _abi.py with matching argument counts, device-only and exported; every refusal comes
    before any launch (this machine has no device: a launch would fail with another code)."""
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    for name, n in (("cc_token_counts_add", 8), ("cc_logits_penalize", 16)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES[name][1]) == n, name
        assert name in _abi.DEVICE_ONLY
    assert "cc_penalty.hip" in _build.SOURCES
    fns = _abi.bind(C.CDLL(_build.build()))
    buf = (C.c_char * 256)()
    p = (C.addressof(buf) + 15) & ~15
    OK, BAD, UNSUPPORTED = 0, -1, -2
    inf, nan = float("inf"), float("nan")

    add = fns["cc_token_counts_add"]
    ok = dict(prompt_count=p, gen_count=p + 64, V=8, tokens=p + 128, n=4, first_pos=0, gen_start=p + 192, stream=None)
    for kw in (dict(prompt_count=None), dict(gen_count=None), dict(gen_start=None), dict(tokens=None), dict(V=0), dict(V=-1), dict(n=-1)):
        assert add(*{**ok, **kw}.values()) == BAD, kw
    assert add(*{**ok, "n": 0}.values()) == OK and add(*{**ok, "n": 0, "tokens": None}.values()) == OK  # (no launch)

    f = fns["cc_logits_penalize"]
    ok = dict(logits=p, out=p, T=1, V=8, row_stride=8, dtype=0, prompt_count=p + 64, gen_count=p + 96, tokens=p + 128, pos=p + 144,
              gen_start=p + 160, r=1.2, f=0.1, p=0.1, bias=None, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    for kw in (dict(T=0), dict(T=-1), dict(T=5), dict(V=0), dict(V=-8), dict(row_stride=7), dict(row_stride=-8), dict(logits=None),
               dict(out=None), dict(prompt_count=None), dict(gen_count=None), dict(gen_start=None), dict(pos=None),
               dict(out=p + 4),  # a partial overlap
               dict(r=0.0), dict(r=-1.0), dict(r=inf), dict(r=nan), dict(f=inf), dict(f=-inf), dict(f=nan), dict(p=inf), dict(p=-inf),
               dict(p=nan)):
        assert call(**kw) == BAD, kw
    for dt in (3, -1, 17):
        assert call(dtype=dt) == UNSUPPORTED, dt
    assert call(T=5, dtype=3) == BAD  # a bad argument is named before the dtype


class Tok:  # (the ids the block-eligible tiny model's caches ask for)
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


V_TINY = 128


def _tiny(strategy="heavy_hitter"):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import ModelArgs, Transformer, setup_caches

    torch.manual_seed(3)
    cfg = dict(block_size=256, vocab_size=V_TINY, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)
    model = Transformer(ModelArgs(**cfg)).to(torch.float32).eval()
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=[strategy], prompt_compression_strategy=["recent_global"], max_cache_length=[32.0], global_tokens=4, recent_window=8)
    setup_caches(model, Tok(), "cpu", 64, dict(kw))
    return model


def _runner(model, prompt, max_new_tokens=16):
    from cold_compress_amd.harness import decode_one_token, generate, prefill

    def run(prompt=prompt, **kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, rows, _ = generate(model, prompt, prefill, decode_one_token, max_new_tokens=max_new_tokens, **kw)
        return seq, rows

    return run


def _same_rows(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _prompt(n=20, seed=1):
    return torch.randint(0, V_TINY, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def test_neutral_settings_are_no_penalties(monkeypatch, oracle):
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import LogitPenalties

    model = _tiny()
    run = _runner(model, _prompt())
    neutral = LogitPenalties(V_TINY, "cpu", logit_bias={3: 0.0})
    assert neutral.neutral and not LogitPenalties(V_TINY, "cpu", presence_penalty=0.5).neutral
    with cpu_twin(monkeypatch, oracle):
        for sampling in (dict(), dict(temperature=0.8, top_k=20, seed=1)):
            seq0, rows0 = run(**sampling)
            seq1, rows1 = run(penalties=neutral, **sampling)
            assert torch.equal(seq0, seq1) and _same_rows(rows0, rows1)
    assert int(neutral.prompt_count.sum()) == 0 and int(neutral.gen_count.sum()) == 0  # (nothing ran)
    x = torch.randn(1, 2, V_TINY)
    assert neutral.apply(x, torch.tensor([1, 2]), torch.tensor([0, 1])) is x


def test_a_banned_token_never_appears(monkeypatch, oracle):
    """The token the unpenalised greedy run emits most often, banned with logit_bias = {tok: -inf}, never appears again; its
    probability is exactly 0 in every returned row."""
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import LogitPenalties

    model = _tiny()
    prompt = _prompt()
    run = _runner(model, prompt, max_new_tokens=24)
    with cpu_twin(monkeypatch, oracle):
        seq0, _ = run()
        gen0 = seq0[len(prompt):]
        tok = int(torch.bincount(gen0.long(), minlength=V_TINY).argmax())
        assert tok in gen0.tolist()
        seq1, rows1 = run(penalties=LogitPenalties(V_TINY, "cpu", logit_bias={tok: -float("inf")}))
    gen1 = seq1[len(prompt):]
    assert len(gen1) == len(gen0) == 24 and tok not in gen1.tolist()
    assert all(float(r[tok]) == 0.0 for r in rows1)


@pytest.mark.parametrize("mode", ["plain", "feed_long_prompts", "decode_first_token", "next_tokens"])
def test_counts_are_the_histogram_of_the_inputs(monkeypatch, oracle, mode):
    """After generate, prompt_count + gen_count is the bincount of every input the run fed (all of the returned sequence but its last
    token), split at the ORIGINAL prompt length: a prompt tail fed through decode steps is prompt, a forced continuation generated."""
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import LogitPenalties

    model = _tiny()
    n = 40 if mode == "feed_long_prompts" else 20
    prompt = _prompt(n, seed=5)
    kw = {"plain": {}, "feed_long_prompts": dict(feed_long_prompts=True), "decode_first_token": dict(decode_first_token=True),
          "next_tokens": dict(next_tokens=_prompt(13, seed=2))}[mode]
    pen = LogitPenalties(V_TINY, "cpu", 1.3, 0.2, 0.4)
    with cpu_twin(monkeypatch, oracle):
        assert n < model.min_cache_length() or mode == "feed_long_prompts"
        seq, _ = _runner(model, prompt, max_new_tokens=8)(penalties=pen, temperature=0.8, top_k=20, seed=3, **kw)
    assert torch.equal(seq[:n], prompt) and len(seq) == n + (13 if mode == "next_tokens" else 8)
    assert pen.prompt_count.tolist() == torch.bincount(seq[:n].long(), minlength=V_TINY).tolist()
    assert pen.gen_count.tolist() == torch.bincount(seq[n:-1].long(), minlength=V_TINY).tolist()
    assert int(pen.gen_start) == n


def test_forced_blocks_are_the_token_loop(monkeypatch, oracle):
    """forced_block = 4 gives the token-by-token loop's tokens, probability rows and counts bit for bit, with sampling and all
    three penalties (and a bias) on — and did run blocks of 4, each with one apply call."""
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import LogitPenalties

    model = _tiny()
    forced = _prompt(13, seed=2)
    blocks, applies = [], []
    real = model.forward_block

    def counted(idx, input_pos, **kw):
        blocks.append(int(idx.shape[1]))
        return real(idx, input_pos, **kw)

    model.forward_block = counted
    run = _runner(model, _prompt())
    pens = [LogitPenalties(V_TINY, "cpu", 1.3, 0.2, 0.4, {7: -float("inf"), 9: 1.5}) for _ in range(2)]
    real_apply = pens[1].apply
    pens[1].apply = lambda logits, *a: (applies.append(int(logits.shape[1])), real_apply(logits, *a))[1]
    sampling = dict(temperature=0.8, top_k=20, seed=1)
    with cpu_twin(monkeypatch, oracle):
        assert model.block_eligible()
        seq0, rows0 = run(next_tokens=forced, penalties=pens[0], **sampling)
        assert not blocks
        seq1, rows1 = run(next_tokens=forced, penalties=pens[1], forced_block=4, **sampling)
    assert blocks and max(blocks) == 4 and [a for a in applies if a > 1] == blocks
    assert torch.equal(seq0, seq1) and _same_rows(rows0, rows1)
    assert torch.equal(pens[0].prompt_count, pens[1].prompt_count) and torch.equal(pens[0].gen_count, pens[1].gen_count)
    assert int(pens[0].gen_count.sum()) == len(forced) - 1


def test_rewind_rebuilds_the_counts(monkeypatch):
    """The decode loop over a stand-in device (the watch of test_host_logic.py's rewind test, subclassed here): a token whose
    single-launch step fails is seen `lag` tokens late; its own launch and every launch behind it chose garbage and COUNTED garbage
    inputs.  The rewound run ends with the fault-free run's sequence and counts."""
    from cold_compress_amd.harness import LogitPenalties
    from cold_compress_amd.harness import generation as G

    V, P0 = 1024, 40
    real_watch = G._StatusWatch
    live = {"state": None, "fail_at": None}
    prompt = torch.randint(0, V, (P0,), generator=torch.Generator().manual_seed(4), dtype=torch.int32)

    def step(model, x, pos, next_token=None, attn_top_k=1.0, penalties=None, **kw):
        logits = torch.randn(1, 1, V, generator=torch.Generator().manual_seed(int(x.view(-1)[0]) * 7919 + int(pos[0])))
        t = torch.argmax(penalties.apply(logits, x, pos)[0, -1]).view(1).to(torch.int32)
        st = live["state"]
        k = int(pos[0]) - P0
        if st is not None and (st["set"] or (k == live["fail_at"] and not st["failed_once"])):
            t = torch.tensor([977], dtype=torch.int32)  # the launch did nothing: garbage, which the next step counts
        return (next_token if next_token is not None else t), torch.ones(1)

    def run(fail_at, lag, n=12):
        state = {"set": False, "failed_once": False}
        live["state"], live["fail_at"] = state, fail_at

        class Watch(real_watch):
            def __init__(self, dev):
                super().__init__(dev, depth=64)

            def _open(self, dev):
                self.values, self.started, self.n_posted = {}, {}, 0

            def _start(self, slot):
                i = self.n_posted
                if i == fail_at and not state["failed_once"]:
                    state["set"], state["failed_once"] = True, True
                self.values[slot] = int(state["set"])
                self.started[slot] = i
                self.n_posted += 1

            def post(self, token_index):
                self.n_posted = token_index
                super().post(token_index)

            def _is_done(self, slot):
                return self.n_posted - 1 - self.started[slot] >= lag

            def _wait_done(self, slot):
                pass

            def _status(self, slot):
                return self.values[slot]

        def recover(model, cur, pos, fn, nt, npb, forced, top_k, kw, max_retries=6, rebuild=None):
            assert state["set"] and rebuild is not None
            state["set"] = False
            rebuild()  # (what _recover_token does before every retry)
            return fn(model, cur, pos, next_token=forced, attn_top_k=top_k, **kw)

        monkeypatch.setattr(G, "_StatusWatch", Watch)
        monkeypatch.setattr(G, "_recover_token", recover)
        pen = LogitPenalties(V, "cpu", 1.5, 0.7, 0.9)
        pen.reset(prompt, P0)
        pos = torch.tensor([P0], dtype=torch.int32)
        toks, _ = G.decode_n_tokens(None, torch.tensor([[3]], dtype=torch.int32), pos, step, n, recover=fail_at is not None or None,
                                    penalties=pen)
        return [int(t) for t in toks], int(pos[0]), pen

    clean, end, pen0 = run(None, 0)
    assert end == P0 + 12 and len(clean) == 12 and 977 not in clean
    assert pen0.gen_count.tolist() == torch.bincount(torch.tensor([3] + clean[:-1]), minlength=V).tolist()
    assert pen0.prompt_count.tolist() == torch.bincount(prompt.long(), minlength=V).tolist()
    for fail_at in (0, 1, 5):
        for lag in (0, 3, 20):
            got, e, pen = run(fail_at, lag)
            assert got == clean and e == end, (fail_at, lag, got, clean)
            assert torch.equal(pen.gen_count, pen0.gen_count) and torch.equal(pen.prompt_count, pen0.prompt_count), (fail_at, lag)


def test_the_real_recover_token_rebuilds_before_every_retry(monkeypatch):
    """_recover_token itself (its device queries stubbed out): `rebuild` runs once before each retry."""
    import contextlib

    from cold_compress_amd import _abi
    from cold_compress_amd import attention_utils as au
    from cold_compress_amd.harness import generation as G

    status = {"left": 2}
    events = []
    monkeypatch.setattr(G, "_collective_status", lambda dev: int(status["left"] > 0))
    monkeypatch.setattr(au, "reset_single_launch_status", lambda dev: None)
    monkeypatch.setattr(G.time, "sleep", lambda s: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(_abi, "lib", lambda: {"cc_decode_step_l2_handoff": lambda: 0})

    class M:
        layers = []

    def fn(model, cur, pos, next_token=None, attn_top_k=1.0, **kw):
        events.append("step")
        status["left"] -= 1
        return torch.tensor([5]), torch.ones(1)

    nt, _ = G._recover_token(M(), torch.tensor([[1]]), torch.tensor([3]), fn, None, None, None, 1.0, {}, rebuild=lambda: events.append("rebuild"))
    assert events == ["rebuild", "step", "rebuild", "step"] and int(nt) == 5


def test_invalid_settings_raise():
    from cold_compress_amd.harness import LogitPenalties

    inf, nan = float("inf"), float("nan")
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=inf), dict(repetition_penalty=nan),
               dict(frequency_penalty=inf), dict(frequency_penalty=-inf), dict(frequency_penalty=nan), dict(presence_penalty=inf),
               dict(presence_penalty=-inf), dict(presence_penalty=nan), dict(logit_bias={3: inf}), dict(logit_bias={3: nan}),
               dict(logit_bias={-1: 1.0}), dict(logit_bias={V_TINY: 1.0}), dict(logit_bias={1.5: 1.0}), dict(repetition_penalty=1e39)):
        with pytest.raises(ValueError):
            LogitPenalties(V_TINY, "cpu", **kw)
    with pytest.raises(ValueError):
        LogitPenalties(0, "cpu")
    pen = LogitPenalties(V_TINY, "cpu", 1.2, logit_bias={0: -inf, V_TINY - 1: 2.0})
    assert not pen.neutral and float(pen.bias[0]) == -inf and float(pen.bias[V_TINY - 1]) == 2.0
    with pytest.raises(ValueError):
        pen.apply(torch.zeros(1, 1, V_TINY + 1))
    with pytest.raises(ValueError):
        pen.apply(torch.zeros(1, 2, V_TINY), torch.tensor([1]), torch.tensor([0]))
