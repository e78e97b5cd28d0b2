"""Cache-budget arithmetic and the generate loop (the build's counterpart of the reference's
generation_utils.py:224-531), with the decode step optionally captured in a hipGraph instead of being traced
by torch.compile (generation_utils.py:578-594).

Budget helpers are exact-integer restatements checked against tests/golden/f8_budgets.json.
"""
import math
import time
from types import SimpleNamespace
from typing import NamedTuple

import torch

from .model import Transformer, find_multiple
from .constraints import LogitConstraints, active as _active_constraints  # noqa: F401
from .penalties import LogitPenalties, active as _active_penalties  # noqa: F401


# ------------------------------------------------------------------------------ budgets (ref: :224-321)
def normalize_cache_length(max_cache_length: float, max_seq_length: int, multiple_of: int = 8) -> int:
    """ref: generation_utils.py:260-276."""
    if 0 < max_cache_length <= 1:
        n = round(max_seq_length * max_cache_length)
    else:
        assert int(max_cache_length) == max_cache_length
        n = int(max_cache_length)
        if n > max_seq_length:
            print(f"FYI: max_cache_length ({n}) is greater than max_seq_length ({max_seq_length}). Setting to {max_seq_length}")
            n = max_seq_length
    return min(find_multiple(n, multiple_of), max_seq_length)


def apply_pyramid_pattern(max_cache_length, max_seq_length, model_n_layer, decreasing=True, min_cache_length=256):
    """ref: generation_utils.py:279-321 (PyramidKV, beta = 14)."""
    beta = 14
    floor = min(min_cache_length, max_cache_length)
    total = max_cache_length * model_n_layer
    lo, hi = total / (model_n_layer * beta), 2 * total / model_n_layer
    step = (hi - lo) / model_n_layer
    lens = [lo] + [lo + step * i for i in range(1, model_n_layer - 1)] + [hi]
    lens = [normalize_cache_length(int(x), max_seq_length) for x in lens]
    overflow = n_over = 0
    for i, x in enumerate(lens):
        if x < floor:
            overflow += floor - x
            lens[i] = floor
            n_over += 1
    if n_over < len(lens):
        dec = overflow // (len(lens) - n_over)
        lens = [max(floor, x - dec) if x > floor else x for x in lens]
    if decreasing:
        lens = lens[::-1]
        assert lens[-1] < lens[0], "Cache lengths should be decreasing."
    else:
        assert lens[0] < lens[-1], "Cache lengths should be increasing."
    return lens


def apply_pattern(pattern, out_size, extension_strategy="tile", max_seq_length=None):
    """ref: generation_utils.py:224-257."""
    assert extension_strategy in {"tile", "repeat", "pyramid", "funnel"}
    assert out_size % len(pattern) == 0, f"{len(pattern)} must be a divisible factor of the number of layers ({out_size})."
    factor = out_size // len(pattern)
    if extension_strategy in {"funnel", "pyramid"}:
        assert len(pattern) == 1, "Funnel and pyramid patterns must have a single element."
        return apply_pyramid_pattern(pattern[0], max_seq_length, out_size, decreasing=extension_strategy == "pyramid")
    if extension_strategy == "tile":
        return [x for x in pattern for _ in range(factor)]
    return list(pattern) * factor


def setup_caches(model: Transformer, tokenizer, device, max_seq_length: int, cache_kwargs: dict) -> dict:
    """ref: generation_utils.py:324-388."""
    ck = cache_kwargs
    ck["max_seq_length"] = max_seq_length
    ck["max_cache_length"] = [normalize_cache_length(x, max_seq_length) for x in ck["max_cache_length"]]
    ck["max_cache_length"] = apply_pattern(ck["max_cache_length"], model.config.n_layer, ck["cache_length_pattern"],
                                           max_seq_length)
    assert len(ck["cache_strategy"]) == len(ck["prompt_compression_strategy"]), \
        "You must specify a prompt_compression_strategy for each cache_strategy."
    ck["cache_strategy"] = apply_pattern(ck["cache_strategy"], model.config.n_layer, ck["cache_strategy_pattern"])
    ck["prompt_compression_strategy"] = apply_pattern(ck["prompt_compression_strategy"], model.config.n_layer,
                                                      ck["cache_strategy_pattern"])
    if not isinstance(ck["recent_window"], list):
        rw = ck["recent_window"]
        if rw <= 1:
            ck["recent_window"] = [max(1, int(rw * n)) for n in ck["max_cache_length"]]
        else:
            ck["recent_window"] = [max(1, min(rw, n)) for n in ck["max_cache_length"]]
    assert ck["global_tokens"] <= min(ck["max_cache_length"]), "Global tokens must be less than max_cache_length."
    if ck["cache_strategy"][0] == "hybrid":
        ck["token_ids"] = {"special": tokenizer.special_ids(), "punctuation": tokenizer.punctuation_ids()}
    with torch.device(device):
        model.setup_caches(max_batch_size=1, **ck)
    return ck


# ------------------------------------------------------------------------------ sampling / steps
def greedy(logits, next_token):
    """ref: generation_utils.py:136-142."""
    row = logits[0, -1]
    if row.is_cuda and next_token is None:
        from . import glue

        probs, idx_next = glue.softmax_argmax(row)  # one launch instead of softmax + arg-max reduce
        return idx_next, probs
    probs = torch.nn.functional.softmax(row, dim=-1)
    idx_next = torch.argmax(probs, keepdim=True).to(dtype=torch.int) if next_token is None else next_token
    return idx_next, probs


_M64 = (1 << 64) - 1


def _i64(v):
    """The uint64 `v` as the int64 with the same bits (torch has no uint64 arithmetic: int64 wraps the same way)."""
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def _mix64(x):
    """murmur3's finaliser on int64 tensors holding uint64 bit patterns (logical shifts spelled with a mask)."""
    lo31 = (1 << 31) - 1
    x = x ^ ((x >> 33) & lo31)
    x = x * _i64(0xFF51AFD7ED558CCD)
    x = x ^ ((x >> 33) & lo31)
    x = x * _i64(0xC4CEB9FE1A85EC53)
    return x ^ ((x >> 33) & lo31)


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def _sample_host(row, temperature, top_k, seed, pos, top_p=None, min_p=None):
    """cc_sample_topk's contract (include/coldcompress.h) in torch on a CPU tensor: the same six steps, fp32 where the kernel is, and
    cc_sample_nucleus's two filters (steps 2a and 2b) when `top_p` / `min_p` are given.  -> (idx, probs, number of kept elements)."""
    V, dt = row.numel(), row.dtype
    tmax = torch.maximum(torch.tensor(float(temperature), dtype=torch.float32), torch.tensor(1e-5, dtype=torch.float32))
    x = (row.float() / tmax).to(dt).float()  # 1. one fp32 division, rounded to the model dtype
    kept = torch.ones(V, dtype=torch.bool)
    if top_k is not None and top_k > 0:  # 2. ties at the pivot are all kept
        kept = x >= torch.topk(x, min(int(top_k), V)).values[-1]
    m = x[kept].max() if bool(kept.any()) else x.max()
    if top_p is not None and _f32(top_p) < 1:  # 2a. the smallest level set of K whose integer mass reaches ceil(top_p * Z)
        K = kept & ~torch.isnan(x)
        w = torch.where(K, torch.floor(torch.exp(x - m) * 2.0 ** 40), torch.zeros_like(x)).to(torch.int64)
        Z = int(w.sum())
        if Z > 0:
            target = min(Z, math.ceil(_f32(top_p) * float(Z)))
            xs, order = torch.sort(torch.where(K, x, torch.full_like(x, -float("inf"))), descending=True, stable=True)
            j = int(torch.searchsorted(torch.cumsum(w[order], 0), torch.tensor(target, dtype=torch.int64)))
            kept = K & (x >= xs[min(j, V - 1)])  # ties at the level are all kept
    if min_p is not None and _f32(min_p) > 0:  # 2b. p_i >= min_p * p_max in the logit domain
        kept = kept & ((x - m) >= torch.tensor(math.log(_f32(min_p)), dtype=torch.float32))
    e = torch.where(kept, torch.exp(x - m), torch.zeros_like(x))  # 3.
    probs = (e / e.sum()).to(dt)
    i = torch.arange(V, dtype=torch.int64)  # 4. (p and i widened from unsigned 32 bits)
    h = _mix64(_mix64(torch.tensor(_i64((int(seed) ^ 0x53414D504C45) + (int(pos) & 0xFFFFFFFF) * 0x9E3779B97F4A7C15), dtype=torch.int64) + i))
    u = (2 * ((h >> 41) & ((1 << 23) - 1)) + 1).to(torch.float32) * 2.0 ** -24
    ee = torch.where(u > 0.5, -torch.log1p(u - 1.0), -torch.log(u))
    key = (x - m) - torch.log(ee)  # 5. Gumbel-max; argmax returns the first maximal index
    key = torch.where(kept, key, torch.full_like(key, -float("inf")))
    nan = torch.isnan(x)
    idx = torch.argmax(nan.to(torch.int8)) if bool(nan.any()) else torch.argmax(key)  # 6. the first NaN's index
    return idx.view(1).to(torch.int), probs, int((kept & ~nan).sum())


def sample(logits, next_token, temperature, top_k, seed, input_pos, top_p=None, min_p=None, return_n_kept=False):
    """The reference's logits_to_probs (generation_utils.py:125-133) and a stateless draw from it: one token per (logits,
    temperature, top_k, seed, position), whatever launches, replays or ranks computed it (include/coldcompress.h, cc_sample_topk).
    `input_pos`: one element, the position of the step whose logits these are.  Device tensors run the kernel; CPU tensors the same
    contract in torch.  A forced `next_token` is returned as given, with the sampled distribution's probabilities.
    `top_p` (nucleus) and `min_p` (None: off) filter the top-k kept set before the softmax (cc_sample_nucleus); an invalid one raises
    (ValueError here, ColdCompressError on the device path).  `return_n_kept`: the size of the kept set as a third result (a
    one-element int32 tensor on the device path, an int on the CPU path)."""
    row = logits[0, -1]
    if row.is_cuda:
        from . import glue

        pos = input_pos.view(-1)[-1:].to(torch.int32)
        if top_p is None and min_p is None and not return_n_kept:
            probs, idx_next = glue.sample_topk(row, temperature, top_k, seed, pos)
        else:
            probs, idx_next, *n_kept = glue.sample_nucleus(row, temperature, top_k, top_p, min_p, seed, pos, return_n_kept)
    else:
        if not float(temperature) > 0:
            raise ValueError(f"sample: temperature must be > 0, got {temperature}")
        if top_p is not None and not _f32(top_p) > 0:
            raise ValueError(f"sample: top_p must be > 0 (>= 1: off), got {top_p}")
        if min_p is not None and not _f32(min_p) <= 1:
            raise ValueError(f"sample: min_p must be <= 1 (<= 0: off), got {min_p}")
        idx_next, probs, n = _sample_host(row, temperature, top_k, seed, int(input_pos.view(-1)[-1]), top_p, min_p)
        n_kept = [n]
    idx_next = idx_next if next_token is None else next_token
    return (idx_next, probs, n_kept[0]) if return_n_kept else (idx_next, probs)


class TokenScores(NamedTuple):
    """What `generate(..., logprobs=True)` returns in place of the probability rows: the committed tokens' log-probabilities under the
    model's own distribution (fp32) and their ranks (int32: how many logits were strictly larger), in commit order."""

    logprob: torch.Tensor
    rank: torch.Tensor


def token_logprobs(logits, targets, fallback=None):
    """Log-probability and rank of one token per row of logits [1, T, V] (include/coldcompress.h, cc_logprob_rows): row r is scored
    against targets[r] where that is >= 0 and against fallback[r] otherwise (`targets` None: all rows against `fallback`); a token
    outside the vocabulary gives NaN and -1.  -> (logprob [T] fp32, rank [T] int32).  Device tensors run the kernel (T <= 64); CPU tensors
    the same contract in torch: an fp32 log_softmax and a compare-and-sum."""
    rows = logits[0]
    T, V = rows.shape
    if rows.is_cuda:
        from . import glue

        tg = None if targets is None else targets.reshape(-1).to(torch.int32)
        fb = None if fallback is None else fallback.reshape(-1).to(torch.int32)
        logprob, _, rank = glue.logprob_rows(rows, tg, fb)
        return logprob, rank
    t = torch.full((T,), -1, dtype=torch.int64) if targets is None else targets.reshape(-1).to(torch.int64)
    if fallback is not None:
        t = torch.where(t >= 0, t, fallback.reshape(-1).to(torch.int64))
    ok = (t >= 0) & (t < V)
    tc = torch.where(ok, t, torch.zeros_like(t)).view(T, 1)
    x = rows.float()
    xt = x.gather(1, tc)
    nan = torch.full((T,), float("nan"), dtype=torch.float32)
    logprob = torch.where(ok, torch.log_softmax(x, dim=-1).gather(1, tc).view(T), nan)
    rank = torch.where(ok & ~torch.isnan(xt.view(T)), (x > xt).sum(dim=1), torch.full((T,), -1, dtype=torch.int64))
    return logprob, rank.to(torch.int32)


class TokenTopScores(NamedTuple):
    """What `generate(..., logprobs=True, top_logprobs=n)` returns: TokenScores' two vectors, and per committed token the ids of the n
    most likely tokens of the model's own row (int32 [tokens, n]: larger logit first, equal logits by lower id; -1 where the row has
    fewer than n non-NaN logits) with their fp32 log-probabilities ([tokens, n]; NaN behind an id of -1)."""

    logprob: torch.Tensor
    rank: torch.Tensor
    top_ids: torch.Tensor
    top_logprobs: torch.Tensor


MAX_TOP_LOGPROBS = 20  # (CC_LOGPROB_MAX_TOPN)


def token_top_logprobs(logits, n, targets=None, fallback=None):
    """token_logprobs' two results and each row's `n` most likely alternatives (include/coldcompress.h, cc_logprob_topn): the ids of
    the n first elements in the order (larger logit first, equal logits by lower id, NaN never listed) and their log-probabilities,
    padded with -1 / NaN.  `targets` and `fallback` both None: no target (NaN and -1), the alternatives alone.
    -> (logprob [T] fp32, rank [T] int32, top_ids [T, n] int32, top_logprobs [T, n] fp32).  Device tensors run the kernel (T <= 64);
    CPU tensors the same contract in torch: an fp32 log_softmax and a stable descending sort over the non-NaN elements."""
    if not 1 <= int(n) <= MAX_TOP_LOGPROBS:
        raise ValueError(f"token_top_logprobs: n must be in 1..{MAX_TOP_LOGPROBS}, got {n}")
    n = int(n)
    rows = logits[0]
    T, V = rows.shape
    if rows.is_cuda:
        from . import glue

        tg = None if targets is None else targets.reshape(-1).to(torch.int32)
        fb = None if fallback is None else fallback.reshape(-1).to(torch.int32)
        logprob, _, rank, top_ids, top_lp = glue.logprob_topn(rows, n, tg, fb)
        return logprob, rank, top_ids, top_lp
    logprob, rank = token_logprobs(logits, targets, fallback)
    x = rows.float()
    isnan = torch.isnan(x)
    by_value = torch.sort(torch.where(isnan, torch.full_like(x, -float("inf")), x), dim=1, descending=True, stable=True).indices
    nan_last = torch.sort(isnan.gather(1, by_value).to(torch.int8), dim=1, stable=True).indices  # (stable: the value order is kept)
    order = by_value.gather(1, nan_last)
    k = min(n, V)
    listed = torch.arange(k).view(1, k) < (V - isnan.sum(dim=1)).view(T, 1)
    top_ids = torch.full((T, n), -1, dtype=torch.int64)
    top_lp = torch.full((T, n), float("nan"), dtype=torch.float32)
    top_ids[:, :k] = torch.where(listed, order[:, :k], top_ids[:, :k])
    top_lp[:, :k] = torch.where(listed, torch.log_softmax(x, dim=-1).gather(1, order[:, :k]), top_lp[:, :k])
    return logprob, rank, top_ids.to(torch.int32), top_lp


def _check_top_logprobs(kw):
    """-> kw's `top_logprobs` as an int or None; ValueError for one without logprobs=True or outside 1..20."""
    n = kw.get("top_logprobs")
    if n is None:
        return None
    if not kw.get("logprobs", False):
        raise ValueError("top_logprobs needs logprobs=True")
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_TOP_LOGPROBS:
        raise ValueError(f"top_logprobs must be an integer in 1..{MAX_TOP_LOGPROBS}, got {n}")
    return int(n)


def _score_rows(rows, targets, fallback=None, top_logprobs=None):
    """TokenScores of logits rows [1, T, V], or TokenTopScores with `top_logprobs` alternatives per row."""
    if top_logprobs is None:
        return TokenScores(*token_logprobs(rows, targets, fallback))
    return TokenTopScores(*token_top_logprobs(rows, top_logprobs, targets, fallback))


def _clone_scores(s):
    return type(s)(*(t.clone() for t in s))


def _cat_scores(parts, top_logprobs, device):
    """scores of single commits, in order, as one TokenScores / TokenTopScores (empty tensors for no commit at all)."""
    if parts:
        return type(parts[0])(*(torch.cat(ts) for ts in zip(*parts)))
    lp, rk = torch.empty(0, dtype=torch.float32, device=device), torch.empty(0, dtype=torch.int32, device=device)
    if top_logprobs is None:
        return TokenScores(lp, rk)
    return TokenTopScores(lp, rk, torch.empty((0, top_logprobs), dtype=torch.int32, device=device),
                          torch.empty((0, top_logprobs), dtype=torch.float32, device=device))


def perplexity(logprob, every=500):
    """The reference's perplexity arithmetic (eval.py:230-241) on a vector of per-token log-probabilities, in float64:
    {"ppl": exp(mean(-logprob)), "ppl@500": the same over the first 500 tokens, "ppl@1000": ...}; `every` None: "ppl" alone."""
    nll = -logprob.detach().to("cpu", torch.float64).view(-1)
    out = {}
    if every:
        for k in range(int(every), len(nll), int(every)):
            out[f"ppl@{k}"] = float(torch.exp(torch.mean(nll[:k])))
    out["ppl"] = float(torch.exp(torch.mean(nll)))
    return out


def _scored(logits, next_token, temperature, top_k, seed, input_pos, top_p, min_p, score_target=None, chosen_from=None, top_logprobs=None):
    """One step's token and its TokenScores (logprobs=True).  A forced step runs no softmax and keeps no row: it is scored against its
    forced token.  A free step chooses its token exactly as greedy / sample do and scores it through `fallback`; so does a captured
    step (`score_target`: a one-element int32 device tensor the replay reads — the forced token, or -1 for what the step chose).
    `chosen_from`: the penalised logits the token is chosen from (LogitPenalties); the scores stay the model's own row's.
    `top_logprobs`: TokenTopScores with that many alternatives of the same row, from the same call."""
    row = logits[:, -1:]
    if next_token is not None and score_target is None:
        return next_token, _score_rows(row, next_token.view(1), None, top_logprobs)
    pick = row if chosen_from is None else chosen_from[:, -1:]
    if temperature is None:
        idx_next, _ = greedy(pick, None)
    else:
        idx_next, _ = sample(pick, None, temperature, top_k, seed, input_pos, top_p=top_p, min_p=min_p)
    scores = _score_rows(row, score_target, idx_next.view(1), top_logprobs)
    return (idx_next if next_token is None else next_token), scores


def _constrained(constraints, rows, chosen_from, tokens, pos):
    """The rows a token is chosen from behind `constraints` (a LogitConstraints; None or a neutral one: `chosen_from` as it is):
    the penalties' output `chosen_from` constrained in place, or else the model's own `rows` constrained into a new tensor (the scores
    keep reading `rows`).  The two stages commute exactly — every penalty step maps -inf to -inf and a +inf bias is refused — so
    penalties first, constraints second is only the cheaper order."""
    con = _active_constraints(constraints)
    if con is None:
        return chosen_from
    if chosen_from is not None:
        return con.apply(chosen_from, tokens, pos, out=chosen_from)
    return con.apply(rows, tokens, pos)


def prefill(model, x, input_pos, next_token=None, temperature=None, top_k=None, seed=0, top_p=None, min_p=None, logprobs=False,
            penalties=None, top_logprobs=None, constraints=None, **_):
    """ref: generation_utils.py:145-160 — the causal mask is implicit in the HIP prefill kernel.  `temperature` None: greedy;
    otherwise the token is drawn at the last prompt position (sample), behind the top_k / top_p / min_p filters.  `logprobs`: the
    second result is the token's TokenScores, taken from the last row, instead of that row's probabilities.  `penalties` (a
    LogitPenalties whose `reset` has counted this prompt): the token is chosen from the penalised last row and the probabilities are
    that row's; the scores stay the model's own.  `top_logprobs` (with `logprobs`): TokenTopScores with that many alternatives.
    `constraints` (a LogitConstraints whose `reset` has stored this prompt): the token is chosen from the constrained last row,
    behind the penalties."""
    top_logprobs = _check_top_logprobs(dict(logprobs=logprobs, top_logprobs=top_logprobs))
    logits = model(x, input_pos, mask=None, is_prefill=True)
    pen = _active_penalties(penalties)
    chosen_from = None
    if pen is not None:  # (the prompt is already counted: this row adds nothing)
        chosen_from = pen.apply(logits[:, -1:])
    chosen_from = _constrained(constraints, logits[:, -1:], chosen_from, None, input_pos[-1:])  # (the prompt is already in the history)
    if logprobs:
        return _scored(logits, next_token, temperature, top_k, seed, input_pos[-1:], top_p, min_p, chosen_from=chosen_from,
                       top_logprobs=top_logprobs)
    if chosen_from is not None:
        logits = chosen_from
    if temperature is None:
        return greedy(logits, next_token)
    return sample(logits, next_token, temperature, top_k, seed, input_pos[-1:], top_p=top_p, min_p=min_p)


def decode_one_token(model, x, input_pos, next_token=None, attn_top_k=1.0, temperature=None, top_k=None, seed=0, top_p=None, min_p=None,
                     logprobs=False, score_target=None, penalties=None, top_logprobs=None, constraints=None, **_):
    """ref: generation_utils.py:163-178.  `temperature` None: greedy; otherwise the token is drawn at `input_pos` (sample).
    `logprobs`: the second result is the token's TokenScores instead of the row's probabilities (_scored).  `penalties`: the step's
    input `x` at `input_pos` is counted (both read from device memory) and the token is chosen from the penalised row.
    `top_logprobs` (with `logprobs`): TokenTopScores with that many alternatives of the model's own row.  `constraints`: the step's
    input `x` is stored at `input_pos` in the positional history (both read from device memory) and the token is chosen from the
    constrained row, behind the penalties."""
    top_logprobs = _check_top_logprobs(dict(logprobs=logprobs, top_logprobs=top_logprobs))
    logits = model(x, input_pos, is_prefill=False, attn_top_k=attn_top_k)
    pen = _active_penalties(penalties)
    chosen_from = pen.apply(logits[:, -1:], x, input_pos) if pen is not None else None
    chosen_from = _constrained(constraints, logits[:, -1:], chosen_from, x, input_pos)
    if logprobs:
        return _scored(logits, next_token, temperature, top_k, seed, input_pos, top_p, min_p, score_target, chosen_from=chosen_from,
                       top_logprobs=top_logprobs)
    if chosen_from is not None:
        logits = chosen_from
    if temperature is None:
        return greedy(logits, next_token)
    return sample(logits, next_token, temperature, top_k, seed, input_pos, top_p=top_p, min_p=min_p)


class GraphedDecoder:
    """One decode step captured in a hipGraph (HIP-native replacement for the reference's
    `torch.compile(mode="reduce-overhead")`, generation_utils.py:581-587).  The token and position live in
    static device tensors; every HIP entry point reads `input_pos` from device memory, so replays advance.
    The sampling settings (temperature, top_k, seed, top_p, min_p; temperature None: greedy) are carried by the captured step BY
    VALUE — the draw itself reads the position from device memory — so a call with other settings than the step was captured with
    captures again.  `logprobs` is one more such setting: the captured step then ends with cc_logprob_rows on its row, scoring
    `self.target` (the forced token, copied in before the replay; -1 for a free step) or else the token the step just wrote, into
    static tensors that the caller clones as it clones the token.  `penalties` (a LogitPenalties; None or a neutral one: none) is
    one more: the captured step holds the addresses of its buffers and advances its counts from `self.tok` / `self.pos`; objects
    compare by identity, so the same object reused across generations does not capture again.  `top_logprobs` (with `logprobs`) is
    the last: the captured step then ends with cc_logprob_topn in place of cc_logprob_rows and `out_probs` is a TokenTopScores of
    static tensors, `out_top_ids` and `out_top_logprobs` among them; another width captures again.  `constraints` (a LogitConstraints;
    None or a neutral one: none) is compared by identity like `penalties`: the captured step holds the addresses of its positional
    history and stores `self.tok` at `self.pos` in it.  The warm-up steps store positions at and behind the captured one, which the
    replays write again before anything reads them, so capture() has nothing of it to put back."""

    _SETTINGS = ("temperature", "top_k", "seed", "top_p", "min_p", "logprobs", "penalties", "top_logprobs", "constraints")
    _LOGPROBS = 5  # (index of `logprobs` in the settings)
    _PENALTIES = 6  # (index of `penalties`: compared after normalisation)
    _CONSTRAINTS = 8  # (index of `constraints`: likewise)

    def __init__(self, model, warmup=2, temperature=None, top_k=None, seed=0, top_p=None, min_p=None, logprobs=False, penalties=None,
                 top_logprobs=None, constraints=None):
        self.model = model
        top_logprobs = _check_top_logprobs(dict(logprobs=logprobs, top_logprobs=top_logprobs))
        self.sampling = (temperature, top_k, seed, top_p, min_p, logprobs, _active_penalties(penalties), top_logprobs,
                         _active_constraints(constraints))
        dev = model.output.weight.device
        self.tok = torch.zeros((1, 1), dtype=torch.int32, device=dev)
        self.pos = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.target = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.graph = None
        self.out_tok = self.out_probs = None
        self.warmup = warmup

    def capture(self):
        """Capture must start from a state where one extra (discarded) step is harmless: run it on a snapshot."""
        caches = [l.attention.kv_cache for l in self.model.layers]
        for c in caches:  # seed the fused decode-step pipelines BEFORE the snapshot so the restored state is runnable
            if hasattr(c, "prepare_decode") and c.supports_fused_step() and not c._next_valid:
                c.prepare_decode(self.pos)
        snap = [{k: v.clone() for k, v in c._buffers.items()} for c in caches]
        flags = [(getattr(c, "_next_valid", None), getattr(c, "_quant_pending", False)) for c in caches]
        pos0 = self.pos.clone()
        kw = dict(zip(self._SETTINGS, self.sampling))
        pen = kw["penalties"]
        pen_snap = pen.snapshot() if pen is not None else None  # (the warm-up steps and the captured step would be counted)
        if kw["logprobs"]:
            kw["score_target"] = self.target
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(self.warmup):  # positions advance like a real decode (the pipeline assumes +1 steps)
                    decode_one_token(self.model, self.tok, self.pos, **kw)
                    self.pos += 1
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.out_tok, self.out_probs = decode_one_token(self.model, self.tok, self.pos, **kw)
            if kw["logprobs"]:
                self.out_logprob, self.out_rank = self.out_probs[:2]
                self.out_top_ids, self.out_top_logprobs = self.out_probs[2:] if kw["top_logprobs"] is not None else (None, None)
            self.graph = graph
            self._epoch = self._cache_epoch()
            self._w12_epoch = self._weights_epoch()
        finally:  # also when capture is refused (e.g. a collective that cannot be captured): the caller falls back to
            self.pos.copy_(pos0)  # eager launches and must find the state it handed in
            if pen is not None:
                pen.restore(pen_snap)
            for c, sn, fl in zip(caches, snap, flags):
                for k, v in sn.items():
                    c._buffers[k].copy_(v)
                if fl[0] is not None:
                    c._next_valid = fl[0]
                c._quant_pending = fl[1]
                if hasattr(c, "_ring_version"):  # ring and tracked window sums were restored together: still in step
                    c._ring_version = c._ring_tag()

    def _cache_epoch(self):
        """Moves when a cache changed something the captured steps carry by value (KVCacheRandom's per-generation seed)."""
        return sum(int(getattr(l.attention.kv_cache, "_graph_epoch", 0)) for l in self.model.layers)

    def _weights_epoch(self):
        """Moves when a packed copy that the captured step may read is gone or out of date (glue.w12_epoch: a dense weight changed in
        place, or copies were dropped): the copies are rebuilt by an eager step only — so capture again (the warm-up steps run
        eagerly)."""
        from . import glue

        return glue.w12_epoch() if glue.w12_enabled() else None

    def __call__(self, model, x, input_pos, next_token=None, **kw):
        sampling = tuple(kw.get(k, d) for k, d in zip(self._SETTINGS, self.sampling))
        sampling = sampling[:self._PENALTIES] + (_active_penalties(sampling[self._PENALTIES]),) + sampling[self._PENALTIES + 1:]
        sampling = sampling[:self._CONSTRAINTS] + (_active_constraints(sampling[self._CONSTRAINTS]),) + sampling[self._CONSTRAINTS + 1:]
        if sampling != self.sampling:  # (carried by value, like what _cache_epoch watches: capture again)
            self.sampling = sampling
            self.graph = None
        if self.graph is not None:
            # A decoder reused across reset() / generations: prepare_decode sits OUTSIDE the captured step, so EVERY cache whose fused
            # pipeline was invalidated since (reset, a prefill) is re-seeded here, at the position the replay is about to run — the
            # captured step would otherwise evict or insert at the previous generation's `next_key` / `step_commit` (r5
            # did this for KVCacheRandom only, whose per-generation seed also moves the epoch below)
            for l in self.model.layers:
                c = l.attention.kv_cache
                if hasattr(c, "prepare_decode") and c.supports_fused_step() and not c._next_valid:
                    self.pos.copy_(input_pos)
                    c.prepare_decode(self.pos)
            if self._cache_epoch() != self._epoch:  # (something the captured steps carry BY VALUE moved: capture again)
                self.graph = None
            elif self._weights_epoch() != self._w12_epoch:
                self.graph = None
        if self.graph is None:
            self.tok.copy_(x)
            self.pos.copy_(input_pos)
            self.capture()
        self.tok.copy_(x)
        self.pos.copy_(input_pos)
        if self.sampling[self._LOGPROBS]:
            if next_token is None:
                self.target.fill_(-1)
            else:
                self.target.copy_(next_token.view(1))
        self.graph.replay()
        if next_token is not None:
            return next_token, self.out_probs
        return self.out_tok, self.out_probs


def negotiate_graphed_decoder(make, first_step, device, log=None):
    """Capture the decode step in a hipGraph on EVERY rank or on none (ref: generation_utils.py:581-587 compiles the step once per
    process; under tp.py's TP every rank must then run the same thing).  `make()` builds the decoder (GraphedDecoder(model));
    `first_step(dec)` runs its first step, i.e. the capture.  A capture that is refused on ANY rank — the RCCL all-reduce inside the
    step cannot be captured by this runtime, an allocator that balks under capture — sends ALL ranks to eager launches: the verdicts
    are combined with a MIN all-reduce that every rank enters whatever happened locally (a rank that fell back alone would replay
    nothing while its peers wait in the captured collective — or skip a timed comparison whose all-reduces its peers sit in).
    -> the decoder, or None (eager).  (bench.py's logic since r2, moved here in r6 so that it can be exercised: tests/test_tp_gloo.py
    injects the refusal on one rank.)"""
    dec = None
    try:
        dec = make()
        first_step(dec)
    except Exception as e:  # capture refused: fall back — together (below)
        if log is not None:
            log(f"hipGraph capture failed ({type(e).__name__}: {e}); falling back to eager launches")
        dec = None
    if _tp_world() > 1:
        import torch.distributed as dist

        ok = torch.tensor([1 if dec is not None else 0], device=device, dtype=torch.int32)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            if dec is not None and log is not None:
                log("a peer rank's hipGraph capture was refused: this rank falls back to eager launches with it")
            dec = None
    return dec


def _tp_world():
    import torch.distributed as dist

    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _collective_status(dev):
    """The single-launch status of `dev` — under tensor parallelism the MAXIMUM over the ranks (a collective: every rank calls it
    at the same point, so every rank retries, raises or moves on TOGETHER; ADVICE r3: a rank-local verdict lets one rank re-run the
    token's all-reduces while its peers have moved on)."""
    from ..attention_utils import single_launch_status

    st = int(single_launch_status(dev))
    if _tp_world() > 1:
        import torch.distributed as dist

        t = torch.tensor([st], dtype=torch.int32, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        st = int(t.item())
    return st


def _recover_token(model, cur_token, input_pos, decode_fn, nt, npb, forced, attn_top_k, kw, max_retries=6, rebuild=None):
    """In-band recovery from a single-launch hand-off that could not complete (a launch whose workgroups were not all resident: a
    co-tenant kernel on the device; or, with the L2-resident hand-off, a workgroup that found itself on an unexpected XCD).  Called
    when the status word of the decode workspace is known to be set: the failed step committed nothing of its kv head, every later
    launch returned at once (include/coldcompress.h, cc_decode_step_heavy_hitter_rc) — so the word is cleared, the epoch words are
    advanced, and the SAME token runs again: workgroups whose part of the step is committed recompute and store nothing, the others
    step.  From the FOURTH attempt on (three have failed) the L2-resident hand-off is demoted ON THIS DEVICE (memory hand-off; a
    captured graph is dropped and captured again) — until the next generate() call.
    Caches whose step carries no commit words (`recoverable()` False) and a failure that persists raise.  Under tensor parallelism
    the status is the maximum over the ranks, so all ranks take every branch here together.
    `rebuild` (with LogitPenalties): called before every retry — the failed attempt's penalise launch counted its input all the same,
    and it puts the counts back to the histogram of the inputs before this token."""
    from .. import _abi
    from ..attention_utils import raise_single_launch_failure, reset_single_launch_status

    dev = cur_token.device
    tries = 0
    while _collective_status(dev):
        # every layer's step must be of the form that honours the status / commit words (a layer on the two-launch or
        # three-call form — a per-layer budget whose shape the single launch cannot serve, single_launch = False — has stepped on
        # garbage behind the failure and would step again on the retry)
        from ..cache import step_is_recoverable

        ok = all(step_is_recoverable(l.attention.kv_cache, l.attention.n_head, l.attention) for l in model.layers)
        if not ok or tries >= max_retries:
            raise_single_launch_failure(dev)  # (clears the word; on every rank together)
        reset_single_launch_status(dev)
        tries += 1
        with torch.cuda.device(dev):  # (the hand-off's verdict is per device: ask about `dev`, not the current one — ADVICE r5)
            l2_on = bool(_abi.lib()["cc_decode_step_l2_handoff"]())
        if tries >= 3 and l2_on:  # (attempts 1-3 as they are: a co-tenant leaves, a misplaced launch does not)
            import warnings

            warnings.warn("cold_compress_amd: a single-launch decode step failed three times; the L2-resident hand-off is switched off "
                          "on this device for the rest of this generation (memory hand-off); generate() restores it when the next one starts")
            with torch.cuda.device(dev):  # per device (r5): other devices of the process keep the faster hand-off
                _abi.lib()["cc_decode_step_demote_l2_handoff"](1)
            _L2_HANDOFF_DEMOTED.add(dev.index if dev.index is not None else torch.cuda.current_device())
            if hasattr(decode_fn, "graph"):
                decode_fn.graph = None  # captured with the L2-resident form: capture again
        time.sleep(0.05 * tries)  # whatever shared the device gets a moment to leave
        if rebuild is not None:
            rebuild()
        nt, npb = decode_fn(model, cur_token, input_pos, next_token=forced, attn_top_k=attn_top_k, **kw)
    return nt, npb


_MAX_BLOCK = 4  # glue.GEMV_MULTI_MAX_T: the most input vectors cc_gemv_fused_multi takes

_FORCED = object()  # greedy()'s `next_token` for a forced row of a block: anything but None takes its torch.softmax branch


def _block_tail(logits, idx, pos, targets, last_free, kw):
    """Everything of a block of T decode steps behind Transformer.forward_block — the ONE place it lives: decode_n_tokens' eager
    block and GraphedBlockDecoder's captured block both call it, so the two cannot drift.  logits [1, T, V]: forward_block's rows;
    idx [1, T] / pos [T]: the steps' input tokens and positions; targets [T] int32: the forced token of each row, -1 for a free last
    row (read with `logprobs` only: may be None without); last_free: the last row's token is drawn from its own row at its own
    position, every other row is forced; kw: the sampling settings (GraphedDecoder._SETTINGS).
    In order: `penalties.apply` over the T rows, `constraints.apply` (in place on the penalties' output), then per row the
    probability row — greedy / sample, a forced greedy row being torch.softmax — or with `logprobs` one cc_logprob_rows /
    cc_logprob_topn call over the model's own T rows, the free row's token drawn first and scored through `fallback`.
    -> (the free last row's token or None, the T probability rows as a list or the TokenScores / TokenTopScores of T rows)."""
    T = logits.shape[1]
    pen, con = _active_penalties(kw.get("penalties")), _active_constraints(kw.get("constraints"))
    temperature = kw.get("temperature")

    def choose(row, p, forced):
        if temperature is None:
            return greedy(row, _FORCED if forced else None)
        return sample(row, None, temperature, kw.get("top_k"), kw.get("seed", 0), p, top_p=kw.get("top_p"), min_p=kw.get("min_p"))

    own = logits  # (the model's own rows: what logprobs scores)
    if pen is not None:
        logits = pen.apply(logits, idx, pos)
    if con is not None:  # (in place on the penalties' output; the model's own rows stay as they are)
        logits = con.apply(logits, idx, pos, out=logits if pen is not None else None)
    if kw.get("logprobs", False):
        fallback = last = None
        if last_free:
            last, _ = choose(logits[:, T - 1:T], pos[T - 1:T], False)
            fallback = torch.zeros((T,), dtype=torch.int32, device=logits.device)
            fallback[T - 1:] = last.view(1)
        return last, _score_rows(own, targets, fallback, _check_top_logprobs(kw))
    last, rows = None, []
    for t in range(T):
        free = last_free and t == T - 1
        nt, npb = choose(logits[:, t:t + 1], pos[t:t + 1], not free)
        rows.append(npb)
        if free:
            last = nt
    return last, rows


class GraphedBlockDecoder:
    """A forced block — Transformer.forward_block over T = 2..4 known input tokens and the whole per-block tail (_block_tail) —
    captured in a hipGraph, on GraphedDecoder's and GraphedStreamsDecoder's pattern.  One graph per (T, last_free)
    under one set of settings (GraphedDecoder._SETTINGS, carried BY VALUE; `penalties` and `constraints` compare by identity behind
    `active`), captured lazily — at most six — into one shared memory pool.  Each graph reads three static tensors of its own that the
    host fills before a replay: `tok` [1, T], `pos` [T] and `targets` [T] (the forced token of each row; -1 for a free last row);
    nothing else that moves between blocks is carried by value.  The captured work is one linear stream of launches.
    Capture follows GraphedDecoder.capture: unseeded fused pipelines are seeded at pos[0:1], every cache buffer, `_next_valid`,
    `_quant_pending` and the penalties' counts are snapshotted, `warmup` whole blocks run on a side stream with positions advancing by
    T, and whatever happens the state handed in is put back.  All graphs are dropped and captured again when the settings differ,
    when a cache's `_graph_epoch` moved (KVCacheRandom's per-generation seed) or when the model's caches were rebuilt
    (setup_caches).  glue.w12_epoch is not watched: a block launches no packed-copy GEMV (the multi GEMVs stream the dense weights).
    Before every replay a cache whose `_next_valid` is False is seeded again, so one decoder serves consecutive generations.  A capture that raises is logged in one line (`log`, default print) and that block and
    every later one until `begin()` — decode_n_tokens calls it once per call — run as eager blocks.  CPU tensors
    (tests/cpu_twin.py) pass through to the eager block.  `captures`, `replays` and `keys()` tell the routes apart."""

    def __init__(self, model, warmup=1, log=None):
        self.model, self.warmup, self.log = model, int(warmup), log
        self.captures = self.replays = 0
        self.refused = False
        self.reset()

    def reset(self):
        """Drop every captured graph (and the pool they share)."""
        self._graphs, self._pool, self.settings = {}, None, None
        self._epoch = self._cache_set = None

    def begin(self):
        """A new decode_n_tokens call: a capture refused in an earlier call is tried again."""
        self.refused = False

    def keys(self):
        """The captured (T, last_free) pairs."""
        return set(self._graphs)

    def _caches(self):
        return [l.attention.kv_cache for l in self.model.layers]

    _cache_epoch = GraphedDecoder._cache_epoch

    @staticmethod
    def _seed_pipelines(caches, pos):
        """prepare_decode sits OUTSIDE the captured block: every cache whose fused pipeline is not seeded (a prefill, a reset, a
        three-call step) is seeded at the block's first position."""
        for c in caches:
            if hasattr(c, "prepare_decode") and c.supports_fused_step() and not c._next_valid:
                c.prepare_decode(pos[0:1])

    @staticmethod
    def _settings_of(kw):
        s = dict(zip(GraphedDecoder._SETTINGS, (None, None, 0, None, None, False, None, None, None)))
        s.update({k: kw[k] for k in s if k in kw})
        s["logprobs"] = bool(s["logprobs"])
        s["penalties"], s["constraints"] = _active_penalties(s["penalties"]), _active_constraints(s["constraints"])
        s["top_logprobs"] = _check_top_logprobs(s)
        return tuple(s[k] for k in GraphedDecoder._SETTINGS)

    def capture(self, g, T, last_free, kw, attn_top_k=1.0):
        """Capture the block of `g`'s static tensors.  Starts from a state where extra (discarded) blocks are harmless: they run on
        a snapshot."""
        caches = self._caches()
        self._seed_pipelines(caches, g.pos)  # BEFORE the snapshot, so that the restored state is runnable
        snap = [{k: v.clone() for k, v in c._buffers.items() if v is not None} for c in caches]
        flags = [(getattr(c, "_next_valid", None), getattr(c, "_quant_pending", False)) for c in caches]
        pos0 = g.pos.clone()
        pen = _active_penalties(kw.get("penalties"))
        pen_snap = pen.snapshot() if pen is not None else None  # (the warm-up blocks would be counted)

        def block():
            return _block_tail(self.model.forward_block(g.tok, g.pos, attn_top_k=attn_top_k), g.tok, g.pos, g.targets, last_free, kw)

        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(self.warmup):  # positions advance like a real decode (the pipelines assume +1 steps)
                    block()
                    g.pos += T
            torch.cuda.current_stream().wait_stream(s)
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=self._pool):
                g.last, g.outs = block()
            g.graph = graph
        finally:  # also when the capture is refused: the caller falls back to eager blocks and must find the state it handed in
            g.pos.copy_(pos0)
            if pen is not None:
                pen.restore(pen_snap)
            for c, sn, fl in zip(caches, snap, flags):
                for k, v in sn.items():
                    c._buffers[k].copy_(v)
                if fl[0] is not None:
                    c._next_valid = fl[0]
                c._quant_pending = fl[1]
                if hasattr(c, "_ring_version"):  # ring and tracked window sums were restored together: still in step
                    c._ring_version = c._ring_tag()

    def _eager(self, idx, pos, targets, last_free, kw, attn_top_k):
        return _block_tail(self.model.forward_block(idx, pos, attn_top_k=attn_top_k), idx, pos, targets, last_free, kw)

    def __call__(self, idx, pos, targets, last_free, kw, attn_top_k=1.0):
        """One block: idx [1, T], pos [T], targets [T] int32 (-1: the free last row) -> (tokens, rows or scores): T one-element
        token tensors — the forced ones views of the static `targets`, a free last one the graph's own output — and what _block_tail
        returns beside them.  Static tensors all: the caller clones what it keeps before the next call."""
        T, last_free = int(idx.shape[1]), bool(last_free)
        if not idx.is_cuda or self.refused or not 2 <= T <= _MAX_BLOCK:
            last, outs = self._eager(idx, pos, targets, last_free, kw, attn_top_k)
            return [targets[t:t + 1] for t in range(T - 1)] + [last if last_free else targets[T - 1:]], outs
        caches = self._caches()
        settings = self._settings_of(kw)
        if self._graphs:
            self._seed_pipelines(caches, pos)  # (KVCacheRandom's first seeding of a generation moves the epoch)
            same = self._cache_set is not None and len(caches) == len(self._cache_set) and all(a is b for a, b in zip(caches, self._cache_set))
            if settings != self.settings or not same or self._cache_epoch() != self._epoch:
                self.reset()
        g = self._graphs.get((T, last_free))
        if g is None:
            dev = idx.device
            g = SimpleNamespace(tok=torch.zeros((1, T), dtype=torch.int32, device=dev), pos=torch.zeros((T,), dtype=torch.int32, device=dev),
                                targets=torch.full((T,), -1, dtype=torch.int32, device=dev), graph=None, last=None, outs=None)
            g.tok.copy_(idx)
            g.pos.copy_(pos)
            g.targets.copy_(targets)
            try:
                self.capture(g, T, last_free, kw, attn_top_k)
            except Exception as e:  # capture refused: the state is as it was handed in (capture's finally)
                (print if self.log is None else self.log)(f"hipGraph capture of a forced block of {T} failed ({type(e).__name__}: {e}); "
                                                          "falling back to eager blocks")
                self.refused = True
                return self(idx, pos, targets, last_free, kw, attn_top_k)
            if not self._graphs:
                self.settings, self._cache_set = settings, caches
            self._epoch = self._cache_epoch()
            self._graphs[(T, last_free)] = g
            self.captures += 1
        g.tok.copy_(idx)
        g.pos.copy_(pos)
        g.targets.copy_(targets)
        self._seed_pipelines(caches, g.pos)
        g.graph.replay()
        self.replays += 1
        return [g.targets[t:t + 1] for t in range(T - 1)] + [g.last if last_free else g.targets[T - 1:]], g.outs

_L2_HANDOFF_DEMOTED = set()  # device indices on which the recovery path demoted the L2-resident hand-off: generate() restores them


def _restore_l2_handoff():
    """A transient co-tenant must not cost every later generation of the process the faster hand-off: what
    _recover_token demoted (per device) is restored when the next generation starts (steps captured in a hipGraph keep the form
    they were captured with)."""
    if _L2_HANDOFF_DEMOTED:
        from .. import _abi

        for idx in sorted(_L2_HANDOFF_DEMOTED):
            with torch.cuda.device(idx):
                _abi.lib()["cc_decode_step_demote_l2_handoff"](0)
        _L2_HANDOFF_DEMOTED.clear()


class _StatusWatch:
    """One asynchronous 4-byte copy of every decode workspace's status word per token, inspected when its event has completed —
    no device synchronisation in the decode loop while fewer than `depth` tokens are in flight (a blocking read per token
    serialises the host's launches with the GPU's work).  Late detection is safe: launches behind a set status word do nothing, so
    the caches stay where the failed token found them; the loop rewinds to that token.  The device side sits in four small methods
    (_open / _start / _is_done / _wait_done / _status) so that the host logic — the ring, its overflow, the order of verdicts — can be
    tested with a stand-in device (tests/test_host_logic.py)."""

    def __init__(self, dev, depth=16):
        self.dev = dev
        self.depth = depth
        self.index = [None] * depth
        self.pending = []   # slots in posting order
        self.overflow = []  # verdicts taken early to free a slot (the host ran `depth` tokens ahead): handed out first, in order
        self._open(dev)

    # ---- device side
    def _open(self, dev):
        from .. import _abi
        from ..attention_utils import _decode_workspaces

        self.off = int(_abi.lib()["cc_decode_step_status_offset"]())
        self.slots = torch.zeros((self.depth, 8), dtype=torch.int32).pin_memory()
        self.events = [None] * self.depth
        self._ws = _decode_workspaces

    def _start(self, slot):
        wss = [w for w in self._ws(self.dev) if self.off + 4 <= w.numel()][:8]
        self.slots[slot].zero_()
        for k, w in enumerate(wss):
            self.slots[slot, k:k + 1].copy_(w[self.off:self.off + 4].view(torch.int32), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[slot] = ev

    def _is_done(self, slot):
        return self.events[slot].query()

    def _wait_done(self, slot):
        self.events[slot].synchronize()

    def _status(self, slot):
        return int(self.slots[slot].max().item())

    # ---- host logic
    def post(self, token_index):
        if len(self.pending) >= self.depth:
            # the ring is full — the normal case under graph replay without terminators: the oldest verdict is WAITED for and KEPT
            # (it used to be dropped here; had it been the failed token's, the rewind would have started one token late and
            # the failed token's garbage would have been committed)
            slot = self.pending[0]
            self._wait_done(slot)
            self.overflow.append(self._take())
        slot = next(k for k in range(self.depth) if k not in self.pending)
        self._start(slot)
        self.index[slot] = token_index
        self.pending.append(slot)

    def _take(self):
        slot = self.pending.pop(0)
        return self.index[slot], self._status(slot)

    def ready(self):
        """-> (token_index, status) of the oldest posted token whose copy has completed, or None."""
        if self.overflow:
            return self.overflow.pop(0)
        if self.pending and self._is_done(self.pending[0]):
            return self._take()
        return None

    def wait_oldest(self):
        if self.overflow:
            return self.overflow.pop(0)
        self._wait_done(self.pending[0])
        return self._take()

    def outstanding(self):
        return bool(self.pending or self.overflow)

    def clear(self):
        self.pending.clear()
        self.overflow.clear()


def decode_n_tokens(model, cur_token, input_pos, decode_one_token, num_new_tokens, terminator_ids=None, attn_top_k=1.0,
                    prefix=None, **kw):
    """ref: generation_utils.py:181-217.  `recover` (ours; default: on with one GPU, off under tensor parallelism — there every
    check is a collective plus a device synchronisation per token, so it is opt-in): watch the single-launch status word and run a
    failed token again in band (_recover_token).  With one GPU the word is read through an asynchronous copy per token and looked
    at when that copy has completed — possibly a few tokens late: the loop then rewinds to the failed token (everything launched
    behind it did nothing).  The loop itself never synchronises the device ONLY without `terminator_ids`: with them, `nt in
    terminator_ids` reads the sampled token on the host every step (the reference's loop does the same, generation_utils.py:207-210),
    and the status copy is then always complete one token later.
    `forced_block` (ours; default 1: this loop as it was): with B > 1 on a model whose `block_eligible(attn_top_k)` holds, steps whose
    INPUT tokens are known run in blocks of up to min(B, 4): steps i .. i+T-1 go through `model.forward_block` when steps i .. i+T-2
    are forced (their outputs, the inputs of i+1 .. i+T-1, are then known) — every dense product of a layer is one pass over its
    weights for the T tokens, the layer's T cache steps run in order, and the T results are committed in order exactly as the single
    steps commit them (the last step of a block may be a free one: its token is drawn from its own row at its own position).
    Blocks are eager launches, or with `block_decoder` (ours; default None: this loop as it was; a GraphedBlockDecoder built for this
    model, else ValueError) replays of a captured hipGraph per (T, last step free); everything else — free steps, fewer than two
    known inputs, an ineligible model — runs through `decode_one_token` as before, and the decoder captures nothing.  A single-launch step that fails INSIDE a block cannot be rewound token-wise (earlier layers have
    committed all T tokens): with `recover` the status word is read once behind each block, and a set word raises.
    `logprobs` (ours; default False: this loop as it was): the second result is not the list of V-sized probability rows but
    TokenScores(logprob, rank), one element per committed token in commit order (trimmed with the tokens when the loop rewinds).  A
    forced step runs no softmax and is scored against its forced token; a free step draws its token as before and scores it; a block
    scores its T rows in one call.
    `top_logprobs` (ours, with `logprobs`; default None: as above): TokenTopScores in place of TokenScores — every element also has
    the n most likely tokens of the model's own row and their log-probabilities (no temperature, filters or penalties), from the same
    call that scores it.
    `penalties` (ours; default None: this loop as it was): a LogitPenalties whose counts hold the prompt; every step counts its input
    token and chooses from the penalised row (a block in one call over its T rows).  Launches behind a set status word do nothing to
    the caches but their penalise launches still count their garbage inputs: a rewind rebuilds the counts from the inputs of the
    steps that stay committed before the failed token runs again, and so does every retry.
    `constraints` (ours; default None: this loop as it was): a LogitConstraints whose history holds the prompt; every step stores its
    input token at its position and chooses from the constrained row, behind the penalties (a block in one call over its T rows).  A
    rewind needs nothing here: the garbage launches stored positions past the failed token's, and those are stored again, in order,
    before any step reads them."""
    new_tokens, new_probs, incs = [], [], []
    pen = _active_penalties(kw.get("penalties"))
    con = _active_constraints(kw.get("constraints"))
    logprobs = bool(kw.get("logprobs", False))
    top_n = _check_top_logprobs(kw)
    recover = kw.pop("recover", None)
    block = kw.pop("forced_block", 1)
    block_decoder = kw.pop("block_decoder", None)
    if block_decoder is not None and block_decoder.model is not model:
        raise ValueError("decode_n_tokens: block_decoder was built for another model")
    block = 1 if block is None else max(1, min(int(block), _MAX_BLOCK))
    use_blocks = block > 1 and prefix is not None and len(prefix) > 0 and bool(getattr(model, "block_eligible", lambda *_: False)(attn_top_k))
    if block_decoder is not None:
        block_decoder.begin()
    tp = _tp_world() > 1
    recover = (cur_token.is_cuda and not tp) if recover is None else bool(recover)
    watch = _StatusWatch(cur_token.device) if recover and not tp else None
    tok0, cur, stopped, i = cur_token, cur_token, False, 0

    def forced_at(k):
        return prefix[k].view(1) if (prefix is not None and k < len(prefix)) else None

    def commit(k, nt, npb):
        nonlocal cur, stopped
        new_tokens.append(nt.clone())
        new_probs.append(_clone_scores(npb) if logprobs else npb.clone())
        teacher_force = prefix is not None and k < len(prefix)
        if terminator_ids and nt in terminator_ids and not teacher_force:
            stopped = True
            incs.append(0)
            return
        input_pos.add_(1)  # (in place, like the reference's `input_pos += 1`)
        incs.append(1)
        cur = nt.view(1, -1)

    def rebuild_before(k):
        """the counts as step k must find them: prompt ‖ inputs of steps < k (tok0 and new_tokens[:k-1]); `input_pos` is step k's."""
        inputs = torch.cat([tok0.view(-1)] + [t.view(-1) for t in new_tokens[:k - 1]]) if k > 0 else tok0.view(-1)[:0]
        pen.rebuild(inputs, int(input_pos.view(-1)[0]) - k)

    def recover_kw(k):
        return {"rebuild": lambda: rebuild_before(k)} if pen is not None else {}

    def block_len(k):
        """how many steps from k on run as one block: all but the last must be forced; 0: step k runs on its own."""
        if not use_blocks:
            return 0
        T = min(block, num_new_tokens - k, len(prefix) - k + 1)
        return T if T >= 2 else 0

    def check_block_status(T, pos):
        if recover and cur_token.is_cuda and _collective_status(cur_token.device):
            from ..attention_utils import raise_single_launch_failure

            try:
                raise_single_launch_failure(cur_token.device)  # (clears the word)
            except Exception as e:
                raise type(e)(f"in the block of {T} forced decode steps starting at position {int(pos[0])}: {e}") from None

    def run_block(k, T):
        """steps k .. k+T-1 through model.forward_block (eager launches, or `block_decoder`'s captured block); commits T results
        in order."""
        idx = torch.cat([cur.view(1, 1), prefix[k:k + T - 1].view(1, -1).to(cur.dtype)], 1)
        pos = input_pos + torch.arange(T, device=input_pos.device, dtype=input_pos.dtype)
        n_forced = min(T, len(prefix) - k)  # T or T - 1: only the last step of a block may be a free one
        targets = None
        if logprobs or block_decoder is not None:
            targets = torch.full((T,), -1, dtype=torch.int32, device=idx.device)
            targets[:n_forced] = prefix[k:k + n_forced]
        if block_decoder is not None:
            toks, outs = block_decoder(idx, pos, targets, n_forced < T, kw, attn_top_k=attn_top_k)
            last = toks[T - 1]
            check_block_status(T, pos)
        else:
            logits = model.forward_block(idx, pos, attn_top_k=attn_top_k)
            check_block_status(T, pos)
            last, outs = _block_tail(logits, idx, pos, targets, n_forced < T, kw)
        for t in range(T):
            commit(k + t, forced_at(k + t) if t < n_forced else last, type(outs)(*(s[t:t + 1] for s in outs)) if logprobs else outs[t])

    while True:
        running = i < num_new_tokens and not stopped
        T = block_len(i) if running else 0
        drain = T > 0 and watch is not None and watch.outstanding()  # (single steps still unjudged: their verdicts first)
        if T > 0 and not drain:
            run_block(i, T)
            i += T
            running = i < num_new_tokens and not stopped
        elif running and not drain:
            nt, npb = decode_one_token(model, cur, input_pos, next_token=forced_at(i), attn_top_k=attn_top_k, **kw)
            if recover and tp:  # collective and synchronous (opt-in): every rank takes the same branch
                nt, npb = _recover_token(model, cur, input_pos, decode_one_token, nt, npb, forced_at(i), attn_top_k, kw, **recover_kw(i))
            if watch is not None:
                watch.post(i)
            commit(i, nt, npb)
            i += 1
            running = i < num_new_tokens and not stopped
        if watch is None:
            if not running:
                break
            continue
        while watch.outstanding():
            r = watch.ready() if (running and not drain) else watch.wait_oldest()
            if r is None:
                break
            f, st = r
            if st:  # token f left the status word set: it, and everything launched behind it, did nothing
                input_pos.sub_(sum(incs[f:]))
                del new_tokens[f:], new_probs[f:], incs[f:]
                cur = new_tokens[f - 1].view(1, -1) if f > 0 else tok0
                stopped = False
                watch.clear()
                if pen is not None:
                    rebuild_before(f)
                nt, npb = _recover_token(model, cur, input_pos, decode_one_token, None, None, forced_at(f), attn_top_k, kw, **recover_kw(f))
                commit(f, nt, npb)
                i = f + 1
                running = i < num_new_tokens and not stopped
                break
        if not running and not watch.outstanding():
            break
    if logprobs:
        return new_tokens, _cat_scores(new_probs, top_n, cur_token.device)
    return new_tokens, new_probs


@torch.no_grad()
def generate(model, prompt, prefill, decode_one_token, max_new_tokens, next_tokens=None, terminator_ids=None,
             feed_long_prompts=False, decode_first_token=False, attn_top_k=1.0, **kw):
    """ref: generation_utils.py:399-531 (prompt-splitting rules, teacher forcing, perf stats).  Unlike the
    reference, the prefill timer is closed after a device sync (SURVEY §5 note).  `logprobs=True` (ours): the second result is
    TokenScores(logprob, rank) of `decode_tokens` elements — the committed tokens' fp32 log-probabilities and ranks — instead of the
    list of probability rows (perplexity() turns the first into the reference's ppl figures).
    `penalties=LogitPenalties(...)` (ours): repetition / frequency / presence penalties and a logit bias on every row a token is
    chosen from, with the token history on the device; the object is reset with the tokens that are prefilled, and positions from the
    ORIGINAL prompt length on count as generated (a teacher-forced continuation included).  The returned probability rows are the
    penalised distribution's; `logprobs` keeps scoring under the model's own.  `top_logprobs=n` (ours, with `logprobs=True`, 1..20):
    the second result is TokenTopScores — the two vectors, and per token the n most likely tokens of the model's own row with their
    log-probabilities; a ValueError before anything runs for an n outside 1..20 or without `logprobs=True`.
    `constraints=LogitConstraints(...)` (ours): n-gram blocking, banned sequences and a minimum number of new tokens on every row a
    token is chosen from, behind the penalties, with the token history on the device by position; the object is reset with the tokens
    that are prefilled and the same `gen_start` as the penalties.  A ValueError before the prefill when the prompt and the new tokens
    do not fit its `max_positions`.
    `block_decoder=GraphedBlockDecoder(model)` (ours, with `forced_block` > 1): the blocks are replayed from captured hipGraphs; a
    decoder built for another model is a ValueError before anything runs."""
    _check_top_logprobs(kw)
    if kw.get("block_decoder") is not None and kw["block_decoder"].model is not model:
        raise ValueError("generate: block_decoder was built for another model")
    prompt_length = prompt.size(0)
    device, dtype = prompt.device, prompt.dtype
    gen_start = prompt_length  # (penalties: a prompt tail that is fed through decode steps below still counts as prompt)
    _restore_l2_handoff()
    min_cache_length = model.min_cache_length()
    max_prompt_len = min_cache_length - 1
    prefix = None
    if (feed_long_prompts and prompt_length > max_prompt_len) or prompt_length == min_cache_length:
        prompt, prefix = prompt[:max_prompt_len], prompt[max_prompt_len:]
        max_new_tokens += len(prefix)
        prompt_length = max_prompt_len
    if decode_first_token:
        prompt, prefix = prompt[:-1], prompt[-1:]
        max_new_tokens += 1
        prompt_length -= 1
    if next_tokens is not None:
        max_new_tokens = len(next_tokens)
        next_token, prefix = next_tokens[0].view(1), next_tokens[1:]
    elif prefix is not None:
        next_token, prefix = prefix[0].view(1), prefix[1:]
    else:
        next_token = prefix = None
    seq = torch.full((prompt_length + max_new_tokens,), -1, dtype=dtype, device=device)
    seq[:prompt_length] = prompt
    input_pos = torch.arange(0, prompt_length, device=device)

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    pen = _active_penalties(kw.get("penalties"))
    if pen is not None:
        pen.reset(prompt, gen_start)
    con = _active_constraints(kw.get("constraints"))
    if con is not None:
        if prompt_length + max_new_tokens > con.max_positions:
            raise ValueError(f"generate: {prompt_length} prompt tokens and {max_new_tokens} new ones do not fit the constraints' "
                             f"max_positions = {con.max_positions}")
        con.reset(prompt, gen_start)
    sync()
    t0 = time.perf_counter()
    ret = prefill(model, prompt.view(1, -1), input_pos, next_token=next_token, **kw)
    sync()
    t1 = time.perf_counter()
    logprobs = bool(kw.get("logprobs", False))
    next_token = ret[0].clone()
    next_tok_probs = _clone_scores(ret[1]) if logprobs else ret[1].clone()
    seq[prompt_length] = next_token
    input_pos = torch.tensor([prompt_length], device=device, dtype=torch.int)
    toks, tok_probs = decode_n_tokens(model, next_token.view(1, -1), input_pos, decode_one_token, max_new_tokens - 1,
                                      terminator_ids=terminator_ids, prefix=prefix, attn_top_k=attn_top_k, **kw)
    sync()
    t2 = time.perf_counter()
    if device.type == "cuda":  # fail loudly: a single-launch step that timed out leaves a word in the decode workspace
        from ..attention_utils import raise_single_launch_failure
        from ..tp import check_oneshot_allreduce_status

        # both verdicts are collectives under tensor parallelism (every rank passes here and raises or not TOGETHER): the transport's
        # first — a rank that raised on its own single-launch word before it would leave its peers waiting in this one
        check_oneshot_allreduce_status()
        if _collective_status(device):
            raise_single_launch_failure(device)
    decode_tokens = len(toks) + 1
    stats = {
        "prefill_tokens": prompt_length, "decode_tokens": decode_tokens,
        "prefill_toks_per_sec": prompt_length / (t1 - t0), "decode_toks_per_sec": decode_tokens / (t2 - t1),
        "total_toks_per_sec": decode_tokens / (t2 - t0), "total_seconds": t2 - t0, "prefill_seconds": t1 - t0,
        "decode_seconds": t2 - t1, "decode_seconds_frac_of_total": (t2 - t1) / (t2 - t0),
        "memory_used_gb": (torch.cuda.max_memory_reserved() / 1e9) if device.type == "cuda" else 0.0,
    }
    if toks:
        seq[prompt_length + 1: prompt_length + 1 + len(toks)] = torch.cat(toks)
    if -1 in seq:
        seq = seq[: torch.where(seq == -1)[0][0]]
    if logprobs:  # (element 0: the token behind the prefill, scored from the prefill's last row)
        return seq, type(tok_probs)(*(torch.cat(ts) for ts in zip(next_tok_probs, tok_probs))), stats
    return seq, [next_tok_probs] + tok_probs, stats


def load_model(checkpoint_path, device, precision, use_tp):
    """ref: generation_utils.py:534-566.  The shape is the CONFIGS entry named by the checkpoint's directory; a path naming int8
    is a weight-only int8 checkpoint (harness/quantize.py), whose int8 buffers stay int8 through `.to(device, precision)`.  A path
    naming int4 is a weight-only int4 checkpoint, DIR/model_int4.gG.pth, G parsed from the name as the reference does; bf16 only.
    Its codes stay uint8, and its (scale, zero) pairs are held per row from the load on.  Any failure to read, validate or shard
    an int4 checkpoint raises ColdCompressError naming the path.  A path naming mxfp4 is a weight-only MXFP4 checkpoint
    (DIR/model_mxfp4.pth): bf16 only, its codes and e8m0 scale bytes stay uint8, and any failure raises ColdCompressError naming the
    path likewise."""
    from pathlib import Path

    from .. import _abi
    from .quantize import (WeightOnlyInt4QuantHandler, WeightOnlyInt8QuantHandler, WeightOnlyMxfp4QuantHandler, check_int4_state_dict,
                           check_mxfp4_state_dict)

    checkpoint_path = Path(checkpoint_path)
    if "mxfp4" in str(checkpoint_path):
        if precision != torch.bfloat16:
            raise _abi.ColdCompressError(f"{checkpoint_path}: MXFP4 weight-only models run in bfloat16 only, not {precision}")
        try:
            with torch.device("meta"):
                model = WeightOnlyMxfp4QuantHandler(Transformer.from_name(checkpoint_path.parent.name)).convert_for_runtime()
            checkpoint = torch.load(str(checkpoint_path), mmap=True, weights_only=True)
            check_mxfp4_state_dict(model, checkpoint)
            model.load_state_dict(checkpoint, assign=True)
            if use_tp:
                from ..tp import apply_tp

                apply_tp(model)
        except Exception as e:
            raise _abi.ColdCompressError(f"{checkpoint_path}: cannot load this mxfp4 weight-only checkpoint: {e}") from e
        return model.to(device=device, dtype=precision).eval()
    int4 = "int4" in str(checkpoint_path)
    if int4:
        try:
            groupsize = int(checkpoint_path.name.split(".")[-2][1:])
        except (IndexError, ValueError):
            raise _abi.ColdCompressError(f"{checkpoint_path}: an int4 checkpoint is named model_int4.gG.pth (G the groupsize)") from None
        if precision != torch.bfloat16:
            raise _abi.ColdCompressError(f"{checkpoint_path}: int4 weight-only models run in bfloat16 only, not {precision}")
    with torch.device("meta"):
        model = Transformer.from_name(checkpoint_path.parent.name)
    if int4:
        try:
            model = WeightOnlyInt4QuantHandler(model, groupsize).convert_for_runtime()
            checkpoint = torch.load(str(checkpoint_path), mmap=True, weights_only=True)
            check_int4_state_dict(model, checkpoint)
            model.load_state_dict(checkpoint, assign=True)
            if use_tp:
                from ..tp import apply_tp

                apply_tp(model)
        except Exception as e:
            raise _abi.ColdCompressError(f"{checkpoint_path}: cannot load this int4 weight-only checkpoint: {e}") from e
        return model.to(device=device, dtype=precision).eval()
    if "int8" in str(checkpoint_path):
        model = WeightOnlyInt8QuantHandler(model).convert_for_runtime()
    checkpoint = torch.load(str(checkpoint_path), mmap=True, weights_only=True)
    if "model" in checkpoint and "stories" in str(checkpoint_path):
        checkpoint = checkpoint["model"]
    model.load_state_dict(checkpoint, assign=True)
    if use_tp:
        from ..tp import apply_tp

        apply_tp(model)
    model = model.to(device=device, dtype=precision)
    return model.eval()
