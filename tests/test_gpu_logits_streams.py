"""cc_logits_penalize_streams and cc_logits_constrain_streams against their single-sequence neighbours (include/coldcompress.h): row
t of a T-row call carries exactly the bits, in `out` and in the state afterwards, that cc_logits_penalize / cc_logits_constrain
write at T = 1 for that row on that row's state.  Every comparison is equality of bits: no tolerance.  Rows whose base is not
16-byte aligned (odd V), count tables and biases at misaligned bases, NaN padding behind the rows that must come back untouched,
in place and out of place, no tokens, tokens outside the vocabulary, a NULL-state row in the middle, rows at unrelated positions on
both sides of their own gen_start; every refusal returns its code with the outputs and the state untouched (the refusals come
before any launch, so the second test of them needs no device)."""
import pytest
import torch

from logits_rows_common import (DTYPES, GEN_STARTS, NAN, OK, PEN_SETTINGS, VS, PenState, RULE_NAMES, _bits, _check_refusals, _rows, con_cases,
                                   con_streams, pen_streams)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("name", list(DTYPES))
def test_penalize_streams_rows_are_the_single_sequence_rows(name, V):
    from cold_compress_amd.harness import glue

    dtype, dev = DTYPES[name], "cuda"
    g = torch.Generator().manual_seed(V * 3 + len(name))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    counted = 0
    for T in (1, 2, 3, 4):
        for stride in (V, V + 3):
            for inplace in (False, True):
                for variant in range(3):
                    states = [PenState(V, dev, g, GEN_STARTS[t], *PEN_SETTINGS[(t + variant) % 4], misaligned=(t + variant) % 2 == 1) for t in range(T)]
                    if T >= 3:
                        states[1] = None  # a NULL-state row in the middle
                    # tokens -1 and V count nothing; positions on both sides of every row's own gen_start
                    tokens = None if variant == 2 else i32([[V - 1, -1, V, 0], [-1, 0, min(3, V - 1), V]][variant][:T])
                    pos = None if variant == 2 else i32([[4, 7, 3, 999], [5, 7, 0, 1000]][variant][:T])
                    x = _rows(T, V, stride, dtype, dev, g)
                    x0 = x.clone()
                    # ---- the single-sequence entry point, row by row at T = 1, on clones of the state
                    want_states = [None if s is None else s.clone() for s in states]
                    want = torch.full((T, stride), NAN, dtype=dtype, device=dev) if not inplace else x.clone()
                    for t, s in enumerate(want_states):
                        if s is None:
                            want[t, :V] = x0[t, :V]
                            continue
                        row = (want if inplace else x0)[t:t + 1, :V]
                        res = glue.logits_penalize(row, s.prompt_count, s.gen_count, s.gen_start, None if tokens is None else tokens[t:t + 1],
                                                   None if pos is None else pos[t:t + 1], s.r, s.f, s.p, s.bias, out=row if inplace else None)
                        if not inplace:
                            want[t, :V] = res[0]
                    # ---- the streams entry point
                    before = [None if s is None else (s.prompt_count.clone(), s.gen_count.clone()) for s in states]
                    out = x if inplace else torch.full((T, stride), NAN, dtype=dtype, device=dev)
                    assert pen_streams(x, out, T, V, stride, dtype, states, tokens, pos) == OK
                    torch.cuda.synchronize()
                    what = (name, V, T, stride, inplace, variant)
                    assert torch.equal(_bits(out), _bits(want)), what  # (the NaN padding included: untouched)
                    if not inplace:
                        assert torch.equal(_bits(x), _bits(x0)), what
                    for t, (s, w) in enumerate(zip(states, want_states)):
                        if s is None:
                            assert torch.equal(_bits(out[t, :V]), _bits(x0[t, :V])), what  # passed through bit for bit
                            continue
                        assert torch.equal(s.prompt_count, w.prompt_count) and torch.equal(s.gen_count, w.gen_count), what
                        moved = int((s.prompt_count != before[t][0]).sum() + (s.gen_count != before[t][1]).sum())
                        valid = tokens is not None and 0 <= int(tokens[t]) < V
                        assert moved == int(valid), what
                        counted += moved
                        if valid:  # on the side of the row's OWN gen_start
                            side = s.gen_count if int(pos[t]) >= GEN_STARTS[t] else s.prompt_count
                            assert int(side[int(tokens[t])]) == int((before[t][1] if side is s.gen_count else before[t][0])[int(tokens[t])]) + 1
    assert counted > 0


@pytest.mark.parametrize("cap", [64, 3000])
@pytest.mark.parametrize("name", list(DTYPES))
def test_constrain_streams_rows_are_the_single_sequence_rows(name, cap):
    from cold_compress_amd.harness import glue

    dtype, dev = DTYPES[name], "cuda"
    g = torch.Generator().manual_seed(cap + len(name))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    hits = {}
    for c in con_cases(cap, dev):
        V, T, stride, inplace, ps, toks, states = (c[k] for k in ("V", "T", "stride", "inplace", "ps", "toks", "states"))
        tokens, pos = (None if toks is None else i32(toks)), i32(ps)
        x = _rows(T, V, stride, dtype, dev, g)
        x0 = x.clone()
        # ---- the single-sequence entry point, row by row at T = 1, on clones of the state
        want_states = [None if s is None else s.clone() for s in states]
        want = x.clone() if inplace else torch.full((T, stride), NAN, dtype=dtype, device=dev)
        for t, s in enumerate(want_states):
            if s is None:
                want[t, :V] = x0[t, :V]
                continue
            row = (want if inplace else x0)[t:t + 1, :V]
            res = glue.logits_constrain(row, s.hist, s.gen_start, None if tokens is None else tokens[t:t + 1], pos[t:t + 1], s.ngram,
                                        s.from_gen, s.m, s.terms, s.bw_tokens, s.bw_offsets, out=row if inplace else None)
            if not inplace:
                want[t, :V] = res[0]
        # ---- the streams entry point
        before = [None if s is None else s.hist.clone() for s in states]
        out = x if inplace else torch.full((T, stride), NAN, dtype=dtype, device=dev)
        assert con_streams(x, out, T, V, stride, dtype, states, tokens, pos) == OK
        torch.cuda.synchronize()
        what = (name, cap, V, T, inplace, toks, ps)
        assert torch.equal(_bits(out), _bits(want)), what  # (the NaN padding included: untouched)
        if not inplace:
            assert torch.equal(_bits(x), _bits(x0)), what
        for t, (s, w) in enumerate(zip(states, want_states)):
            if s is None:
                assert torch.equal(_bits(out[t, :V]), _bits(x0[t, :V])), what  # passed through bit for bit
                continue
            assert torch.equal(s.hist, w.hist), what
            changed = (s.hist != before[t]).nonzero().view(-1).tolist()
            stored = toks is not None and 0 <= ps[t] < cap
            assert changed == ([ps[t]] if stored else []), (what, t, changed)  # exactly pos[t], or nothing
            assert not stored or int(s.hist[ps[t]]) == toks[t]
            ids = s.banned(V)  # the contract itself: these are -inf, every other element keeps its bits (none for a row outside the history)
            keep = torch.ones(V, dtype=torch.bool, device=dev)
            if ids:
                keep[ids] = False
                assert bool(torch.isneginf(out[t, :V][~keep].float()).all()), (what, t)
            assert torch.equal(_bits(out[t, :V])[keep], _bits(x0[t, :V])[keep]), (what, t)
            for rule, n in s.hits(V).items():
                hits[rule] = hits.get(rule, 0) + n
    assert set(hits) == RULE_NAMES and all(n > 0 for n in hits.values()), hits  # every rule banned something somewhere


def test_every_refusal_returns_its_code_with_outputs_and_state_untouched():
    _check_refusals("cuda")
