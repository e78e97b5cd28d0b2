"""`forced_block` of harness.decode_n_tokens without a GPU: the generate() branches of tests/golden/f1_generate_branches.npz replayed
over tests/cpu_twin.py with blocks of 2, 3 and 4 known tokens (Transformer.forward_block's row-by-row CPU twin) against the
reference's recorded tokens and against the token-by-token run, bit for bit; the block scheduling on its own with a stand-in model
that records every (idx, input_pos) it is handed; and Transformer.block_eligible's truth table."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from cpu_twin import cpu_twin


class Tok:  # (the ids oracle/gen_golden.py::FakeTok hands the reference)
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


@pytest.fixture()
def twin(monkeypatch, oracle):
    with cpu_twin(monkeypatch, oracle) as fns:
        yield fns


# ------------------------------------------------------------------------------------------------ the reference's branches, in blocks
def _branch_cases():
    from helpers import GOLDEN

    return [str(c) for c in np.load(os.path.join(GOLDEN, "f1_generate_branches.npz"))["cases"]]


def _branch_run(f, name, forced_block, counts):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import ModelArgs, Transformer, decode_one_token, generate, prefill, setup_caches

    cfg = dict(block_size=256, vocab_size=128, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)
    model = Transformer(ModelArgs(**cfg)).to(torch.float32).eval()
    model.load_state_dict({k[3:]: v for k, v in f.items() if k.startswith("sd.")}, strict=True)
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(json.loads(f[name + ".cache_args_json"]))
    gk = json.loads(f[name + ".gen_kwargs_json"])
    if "next_tokens" in gk:
        gk["next_tokens"] = torch.tensor(gk["next_tokens"], dtype=torch.int32)
    setup_caches(model, Tok(), "cpu", int(f[name + ".total"]), dict(kw))
    real = model.forward_block

    def counted(idx, input_pos, **k2):
        counts.append(int(idx.shape[1]))
        return real(idx, input_pos, **k2)

    model.forward_block = counted
    extra = {} if forced_block is None else {"forced_block": forced_block}
    seq, probs, stats = generate(model, f[name + ".prompt"], prefill, decode_one_token, max_new_tokens=int(f[name + ".new_tokens"]), **gk, **extra)
    state = [{n: b.clone() for n, b in layer.attention.kv_cache._buffers.items() if b is not None} for layer in model.layers]
    return seq, probs, stats, state, gk


@pytest.mark.parametrize("forced_block", [2, 3, 4])
def test_generate_branches_in_blocks_match_reference_and_single_steps(twin, forced_block):
    """feed_long_prompts, a prompt as long as the cache, decode_first_token, next_tokens, early stop on a terminator (and the other
    recorded cases): with forced_block the returned sequence is the reference's (where the token-by-token run reproduces it: the
    hybrid cases part ways by construction, tests/test_host_e2e_cpu.py) and sequence, probabilities and every cache buffer equal the
    forced_block-less run bit for bit.  Cases with known input tokens must actually have run blocks."""
    from helpers import load_golden

    f = load_golden("f1_generate_branches.npz")
    blocks_by_branch = {}
    for name in _branch_cases():
        c1, cb = [], []
        seq1, probs1, stats1, state1, gk = _branch_run(f, name, None, c1)
        seqb, probsb, statsb, stateb, _ = _branch_run(f, name, forced_block, cb)
        assert not c1, f"{name}: the default loop ran a block"
        assert all(2 <= t <= forced_block for t in cb), (name, cb)
        assert torch.equal(seqb, seq1), f"{name}: sequence differs from the token-by-token run"
        if f"{name}.cache_strategies_L0" not in f:
            assert torch.equal(seqb, f[name + ".seq"]), f"{name}: sequence differs from the reference's"
        assert (statsb["prefill_tokens"], statsb["decode_tokens"], len(probsb)) == (int(f[name + ".prefill_tokens"]), int(f[name + ".decode_tokens"]),
                                                                               int(f[name + ".n_probs"])), name
        assert len(probsb) == len(probs1) and all(torch.equal(a, b) for a, b in zip(probsb, probs1)), f"{name}: probabilities"
        for li, (sa, sb) in enumerate(zip(state1, stateb)):
            assert sa.keys() == sb.keys()
            for n in sa:
                assert torch.equal(sa[n], sb[n]), f"{name}: layer {li} buffer {n}"
        blocks_by_branch[name] = cb
    # the branches the issue names were all replayed; those with two or more known inputs in a row ran blocks (a prompt as long as
    # the cache and decode_first_token force ONE token, the prefill's: nothing is known behind it, and their runs are single steps)
    assert {"feed_long", "prompt_equals_cache", "decode_first", "teacher_forced", "terminator"} <= set(blocks_by_branch), blocks_by_branch
    assert sum(blocks_by_branch["feed_long"]) >= 23 and sum(blocks_by_branch["teacher_forced"]) >= 6, blocks_by_branch


# ------------------------------------------------------------------------------------------------ the scheduling alone
V = 32


class StandIn:
    """forward_block / the single step of a 'model' whose next token is (input + 1) % V, recording what each is handed."""

    def __init__(self, eligible=True):
        self.eligible = eligible
        self.blocks, self.singles = [], []

    def block_eligible(self, attn_top_k=1.0):
        return self.eligible

    @staticmethod
    def _logits(tokens):
        out = torch.zeros(1, len(tokens), V)
        for t, tok in enumerate(tokens):
            out[0, t, (int(tok) + 1) % V] = 8.0
        return out

    def forward_block(self, idx, input_pos, attn_top_k=1.0):
        assert idx.shape == (1, len(input_pos))
        self.blocks.append((idx.view(-1).tolist(), input_pos.tolist()))
        return self._logits(idx.view(-1).tolist())

    def single(self, model, x, input_pos, next_token=None, **kw):
        from cold_compress_amd.harness.generation import greedy

        assert model is self
        self.singles.append((x.view(-1).tolist(), input_pos.tolist()))
        return greedy(self._logits(x.view(-1).tolist()), next_token)


def _schedule(n_steps, prefix, forced_block, terminators=None, eligible=True, first=3, pos0=10):
    from cold_compress_amd.harness.generation import decode_n_tokens

    m = StandIn(eligible)
    pos = torch.tensor([pos0], dtype=torch.int32)
    kw = {} if forced_block is None else {"forced_block": forced_block}
    toks, probs = decode_n_tokens(m, torch.tensor([[first]], dtype=torch.int32), pos, m.single, n_steps, terminator_ids=terminators,
                                  prefix=None if prefix is None else torch.tensor(prefix, dtype=torch.int32), **kw)
    return m, [int(t) for t in toks], probs, int(pos)


def _single_reference(n_steps, prefix, terminators=None, first=3, pos0=10):
    return _schedule(n_steps, prefix, None, terminators, first=first, pos0=pos0)


def test_block_boundaries_and_tail():
    """13 forced steps in blocks of 4: inputs cur, p0..p2 | p3..p6 | p7..p10 at consecutive positions, then the tail of one step
    (its input p11 is known, but a block needs two) through the single step."""
    prefix = list(range(20, 33))  # 13 forced tokens
    m, toks, probs, pos = _schedule(13, prefix, 4)
    assert m.blocks == [([3, 20, 21, 22], [10, 11, 12, 13]), ([23, 24, 25, 26], [14, 15, 16, 17]), ([27, 28, 29, 30], [18, 19, 20, 21])]
    assert m.singles == [([31], [22])]
    r, rtoks, rprobs, rpos = _single_reference(13, prefix)
    assert toks == rtoks == prefix and pos == rpos == 23 and not r.blocks and len(r.singles) == 13
    assert all(torch.equal(a, b) for a, b in zip(probs, rprobs))


def test_last_step_of_a_block_may_be_free_and_no_block_crosses_a_free_step():
    """5 forced tokens, 9 steps: steps 0..4 forced, 5.. free.  Blocks: steps 0-3 (inputs cur, p0, p1, p2), then steps 4-5 — step 5
    is FREE but its input p4 is known; its token is drawn from its row.  Steps 6.. depend on that draw: single steps."""
    prefix = [7, 9, 11, 13, 15]
    m, toks, probs, pos = _schedule(9, prefix, 4)
    assert m.blocks == [([3, 7, 9, 11], [10, 11, 12, 13]), ([13, 15], [14, 15])]
    assert m.singles == [([16], [16]), ([17], [17]), ([18], [18])]
    assert toks == prefix + [16, 17, 18, 19] and pos == 19
    r, rtoks, rprobs, rpos = _single_reference(9, prefix)
    assert toks == rtoks and pos == rpos and all(torch.equal(a, b) for a, b in zip(probs, rprobs))


@pytest.mark.parametrize("forced_block,want", [(2, [2, 2, 2]), (3, [3, 3]), (4, [4, 2]), (9, [4, 2]), (1, []), (None, [])])
def test_block_sizes_and_the_clamp(forced_block, want):
    """6 steps, 5 of them forced: every block size, forced_block above 4 clamps to 4, 1 / absent runs no block."""
    prefix = [4, 5, 6, 7, 8]
    m, toks, _, pos = _schedule(6, prefix, forced_block)
    assert [len(b[0]) for b in m.blocks] == want
    assert toks == prefix + [9] and pos == 16
    assert len(m.singles) == 6 - sum(want)


def test_terminator_on_the_free_step_behind_a_block_and_forced_terminators():
    """A forced token that is a terminator does not stop (teacher forcing); the free last step of a block drawing one does, and
    nothing runs behind it — as in the token-by-token loop."""
    prefix = [4, 9, 6]  # 9 is a terminator id, forced: ignored
    for fb in (4, 2, None):
        m, toks, probs, pos = _schedule(8, prefix, fb, terminators=[9, 7])  # step 3 is free: input 6 -> draws 7: stop
        assert toks == [4, 9, 6, 7] and pos == 13 and len(probs) == 4, fb
        if fb == 4:
            assert m.blocks == [([3, 4, 9, 6], [10, 11, 12, 13])] and not m.singles
        if fb == 2:
            assert m.blocks == [([3, 4], [10, 11]), ([9, 6], [12, 13])] and not m.singles
    # a terminator drawn on a free SINGLE step right behind a block
    m, toks, _, pos = _schedule(8, [4, 5], 2, terminators=[7])  # block: steps 0-1 (forced 4, 5); step 2 free in the block?  no: T = 2
    assert toks == [4, 5, 6, 7] and m.blocks == [([3, 4], [10, 11])] and m.singles == [([5], [12]), ([6], [13])] and pos == 13


def test_ineligible_model_and_missing_prefix_run_token_by_token():
    m, toks, _, _ = _schedule(6, [4, 5, 6, 7, 8], 4, eligible=False)
    assert not m.blocks and len(m.singles) == 6 and toks == [4, 5, 6, 7, 8, 9]
    m, toks, _, _ = _schedule(4, None, 4)
    assert not m.blocks and len(m.singles) == 4 and toks == [4, 5, 6, 7]
    m, toks, _, _ = _schedule(4, [9], 4)  # one known input behind cur: a block of 2 (step 1 free)
    assert [len(b[0]) for b in m.blocks] == [2] and toks == [9, 10, 11, 12]


# ------------------------------------------------------------------------------------------------ block_eligible
def _tiny(strategy="heavy_hitter", n_local_heads=2, dim=64, dtype=torch.float32, **cache_kw):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import ModelArgs, Transformer, setup_caches

    torch.manual_seed(0)
    cfg = dict(block_size=256, vocab_size=128, n_layer=2, n_head=4, n_local_heads=n_local_heads, dim=dim, intermediate_size=128)
    model = Transformer(ModelArgs(**cfg)).to(dtype).eval()
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(dict(cache_strategy=[strategy], prompt_compression_strategy=["recent_global"], max_cache_length=[32.0], global_tokens=4,
                   recent_window=8), **cache_kw)
    setup_caches(model, Tok(), "cpu", 64, dict(kw))
    return model


def test_block_eligible_truth_table(twin, monkeypatch):
    from cold_compress_amd.harness import glue

    m = _tiny()
    assert m.block_eligible() and m.block_eligible(1.0)
    assert not m.block_eligible(0.5), "attn_top_k < 1"
    m.layers[1].attention.fuse_qkv_step = True
    assert not m.block_eligible(), "the single-launch QKV step"
    m.layers[1].attention.fuse_qkv_step = False
    assert m.block_eligible()
    # a cache that quantises in reference mode is out, the fused modes are in
    assert not _tiny(cache_bits=8).block_eligible(), "--cache_bits 8 in reference mode"
    # (uint8 images; the fused modes serve 16-bit models, head_dim 128, multiples of 4 query heads per kv head)
    q = _tiny(n_local_heads=1, dim=512, dtype=torch.bfloat16, cache_bits=8, cache_quant_mode="fused")
    assert all(l.attention.kv_cache.fused_quant for l in q.layers) and q.block_eligible(), "fused uint8"
    # weight-only weights
    m.layers[0].feed_forward.w2.weight = torch.nn.Parameter(torch.zeros(64, 128, dtype=torch.int8), requires_grad=False)
    assert not m.block_eligible(), "int8 weights"
    m = _tiny()
    m.output.weight = torch.nn.Parameter(torch.zeros(128, 32, dtype=torch.uint8), requires_grad=False)
    assert not m.block_eligible(), "uint8 (int4 / MXFP4) LM head"
    # an analysis cache
    m = _tiny()
    from cold_compress_amd.cache import KVCacheAnalysis

    m.layers[0].attention.kv_cache.__class__ = type("A", (KVCacheAnalysis,), {"__init__": lambda self: None})
    assert not m.block_eligible(), "KVCacheAnalysis"
    # tensor parallelism
    m = _tiny()
    import cold_compress_amd.harness.generation as G

    monkeypatch.setattr(G, "_tp_world", lambda: 2)
    assert not m.block_eligible(), "world size 2"
    monkeypatch.setattr(G, "_tp_world", lambda: 1)
    # before setup_caches
    from cold_compress_amd.harness import ModelArgs, Transformer

    assert not Transformer(ModelArgs(block_size=64, vocab_size=32, n_layer=1, n_head=2, dim=32)).block_eligible()
    # device conditions (device tensors): fuse_gemv off or a shape the GEMV does not take -> not eligible.  Judged on a CPU model by
    # pretending its tensors are device tensors.
    m = _tiny()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(glue, "gemv_supported", lambda *w: True)
    assert m.block_eligible()
    m.layers[0].fuse_gemv = False
    assert not m.block_eligible(), "fuse_gemv off"
    m.layers[0].fuse_gemv = True
    monkeypatch.setattr(glue, "gemv_supported", lambda *w: False)
    assert not m.block_eligible(), "a shape the streamed GEMV does not serve"
