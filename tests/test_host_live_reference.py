"""The host-side budget arithmetic against the reference on random inputs: normalize_cache_length, apply_pyramid_pattern
(PyramidKV budgets, increasing and decreasing), apply_pattern (tile / repeat / pyramid / funnel) and find_multiple — same value, or the
same exception type on both sides; and setup_caches on random configurations.  The reference's answers were captured on CPU by
oracle/gen_golden.py (tests/golden/f8_budgets_random.json, f8_setup_random.json); tests/golden/f8_budgets.json pins the fixed table."""
import json
import os

from helpers import GOLDEN


def _golden_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _ours(fn, args):
    import contextlib
    import io

    from cold_compress_amd.harness import generation as G
    from cold_compress_amd.harness.model import find_multiple

    f = {"normalize": G.normalize_cache_length, "pyramid": lambda a, b, c, d: G.apply_pyramid_pattern(a, b, c, decreasing=d),
         "pattern": lambda p, n, s, m: G.apply_pattern(p, n, s, m), "find_multiple": find_multiple}[fn]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return f(*args)
    except Exception as e:
        return type(e).__name__


def test_budget_arithmetic_matches_reference_on_random_inputs():
    rows = _golden_json("f8_budgets_random.json")
    cases, ref = [c for c, _ in rows], [w for _, w in rows]
    assert len(cases) == 1000
    bad = [(c, want, _ours(*c)) for c, want in zip(cases, ref) if _ours(*c) != want]
    assert not bad, f"{len(bad)} of {len(cases)} differ, first: {bad[:3]}"
    assert sum(1 for x in ref if not isinstance(x, str)) > 0.5 * len(cases)  # (mostly values, not mostly refusals)


def test_setup_caches_matches_reference_on_random_configs(monkeypatch, oracle):
    """setup_caches (ref: generation_utils.py:324-388, model.py:191-233) on random configurations — strategies and their patterns, cache
    lengths as fractions or counts with tile / repeat / pyramid / funnel, recent windows as fractions or counts, layer counts — against
    the reference's: the normalised keyword lists it returns, and per layer the cache class, its length, buffer shape, window, sinks
    and the prompt compressor's class; or the same exception type.  (The caches are built on CPU tensors over the oracle's twins.)"""
    import argparse
    import contextlib
    import io
    import sys as _sys

    _sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    from cpu_twin import cpu_twin

    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import ModelArgs, Transformer, setup_caches

    rows = _golden_json("f8_setup_random.json")
    assert len(rows) == 80
    n_ok = 0
    with cpu_twin(monkeypatch, oracle):
        for (n_layer, max_seq, kw), want in rows:
            cfg = dict(block_size=max(256, max_seq), vocab_size=128, n_layer=n_layer, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)
            model = Transformer(ModelArgs(**cfg)).to(torch.float32).eval()
            ap = argparse.ArgumentParser()
            cache.add_cache_arguments(ap)
            ck = vars(ap.parse_args([]))
            ck.update(kw)

            class Tok:
                def special_ids(self):
                    return [[1], [2, 3]]

                def punctuation_ids(self):
                    return [5, 6, 7]

            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    got_kw = setup_caches(model, Tok(), "cpu", max_seq, dict(ck))
                layers = [[type(l.attention.kv_cache).__name__, int(l.attention.kv_cache.max_cache_length), list(l.attention.kv_cache.pos.shape),
                           int(getattr(l.attention.kv_cache, "recent_window", -1)), int(getattr(l.attention.kv_cache, "global_tokens", -1)),
                           type(l.attention.prompt_compressor).__name__] for l in model.layers]
                got = {"max_cache_length": list(got_kw["max_cache_length"]), "recent_window": list(got_kw["recent_window"]),
                       "cache_strategy": list(got_kw["cache_strategy"]), "prompt_compression_strategy": list(got_kw["prompt_compression_strategy"]),
                       "layers": layers}
            except Exception as e:
                got = type(e).__name__
            assert got == want, f"n_layer {n_layer}, max_seq {max_seq}, {kw}:\nours      {got}\nreference {want}"
            n_ok += isinstance(want, dict)
    assert n_ok >= 30, f"only {n_ok} of {len(rows)} configurations were valid in the reference: the draw is too hostile"
