"""Sequence rules in front of the sampling tail: no_repeat_ngram_size, bad_words_ids and min_new_tokens (Hugging Face's
NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor and MinNewTokensLengthLogitsProcessor), with the token history kept on the
device BY POSITION (include/coldcompress.h, cc_token_history_write / cc_logits_constrain) so that a captured decode step advances
through it.

The invariant: `hist[q]` is the input token at position q.  A step at position p writes hist[p] and reads hist only in front of p, so
a launch that ran behind a failed step — it wrote positions past the failed one — leaves nothing to put back: those positions are
written again, in order, before any step reads them."""
import torch

MAX_NGRAM, MAX_TERMINATORS, MAX_BAD_WORDS, MAX_BAD_WORDS_TOKENS = 32, 64, 1024, 4096  # (CC_CONSTRAIN_MAX_*)


def _banned(s, p, gen_start, n, from_gen, m, terms, bad_words):
    """The ids the rules ban for the row at position p whose history is the list s = s[0 .. p]."""
    ban = set()
    if n > 0:
        tail = s[p - n + 2:p + 1] if n > 1 else []
        for i in range(max(gen_start, 0) if from_gen else 0, p - n + 2):
            if s[i:i + n - 1] == tail:
                ban.add(s[i + n - 1])
    if p + 1 - gen_start < m:
        ban.update(terms)
    for w in bad_words:
        k = len(w) - 1
        if k == 0 or (k <= p + 1 and s[p - k + 1:p + 1] == w[:k]):
            ban.add(w[k])
    return ban


def _constrain_host(rows, out, hist, tokens, pos0, gen_start, n, from_gen, m, terms, bad_words):
    """cc_logits_constrain's contract on CPU tensors: rows [T, V] -> out (rows itself: in place); hist advances in place."""
    T, V = rows.shape
    cap = hist.numel()
    if out is not rows:
        out.copy_(rows)
    toks = None if tokens is None else [int(x) for x in tokens]
    for t in range(T):
        p = pos0 + t
        if not 0 <= p < cap:
            continue
        if toks is None:
            s = hist[:p + 1].tolist()
        else:
            s = hist[:max(pos0, 0)].tolist() + [toks[j - pos0] for j in range(max(pos0, 0), p + 1)]
        ids = sorted(w for w in _banned(s, p, gen_start, n, from_gen, m, terms, bad_words) if 0 <= w < V)
        if ids:
            out[t, ids] = -float("inf")
    if toks is not None:
        for t in range(T):
            if 0 <= pos0 + t < cap:
                hist[pos0 + t] = toks[t]
    return out


class LogitConstraints:
    """The settings and the device-resident state of the sequence rules for ONE sequence.  A row computed at position p (its input
    token sits at p) predicts the token at p + 1; its history is s[0 .. p], the prompt followed by the decode inputs.  A banned element
    becomes -inf of the row's dtype whatever it held; every other element keeps its bits; an id outside the vocabulary bans nothing.
      no_repeat_ngram_size = n (1 .. 32; 0: off): for every i0 <= i <= p - n + 1 with s[i .. i+n-2] == s[p-n+2 .. p], s[i+n-1] is
        banned (HF's NoRepeatNGramLogitsProcessor; n = 1 bans every token seen).  ngram_scope "all": i0 = 0, the prompt takes part as
        in HF; "generated": i0 = gen_start, only n-grams that lie wholly in the generated part block (a model may copy from its prompt).
      min_new_tokens = m with terminator_ids (at most 64): while p + 1 - gen_start < m every terminator is banned (HF's
        MinNewTokensLengthLogitsProcessor).
      bad_words_ids: token sequences (1 .. 32 long, at most 1024 of them and 4096 tokens in all); a sequence w of length k + 1 bans
        w[k] when k == 0, or when k <= p + 1 and s[p-k+1 .. p] == w[0 .. k-1].  The rule is PER SEQUENCE: HF's NoBadWordsLogitsProcessor
        applies none of its sequences while the history is shorter than the longest of them; that quirk is not followed, so the two
        agree wherever the history is at least as long as the longest sequence.
    Invalid settings raise ValueError.  An object with every rule off (`neutral`) behaves exactly as `constraints=None`: nothing is
    launched and `apply` returns its argument.
    The state is `hist` (int32 [max_positions]: hist[q] = the input token at position q) and `gen_start` (int32 [1]); both live as
    long as the object, so a captured graph can hold their addresses.  There is nothing to snapshot, restore or rebuild: a step never
    reads a position that it, or a launch behind it, wrote.  CPU tensors run the same contract in plain Python (as `LogitPenalties`
    and `sample` do)."""

    def __init__(self, vocab_size, device, max_positions, no_repeat_ngram_size=0, ngram_scope="all", min_new_tokens=0,
                 terminator_ids=None, bad_words_ids=None):
        V = int(vocab_size)
        if V <= 0:
            raise ValueError(f"LogitConstraints: vocab_size must be > 0, got {vocab_size}")

        def integer(v, what):
            try:
                ok = not isinstance(v, bool) and int(v) == v
            except (TypeError, ValueError, OverflowError):  # (None, a string, a list, inf, nan)
                ok = False
            if not ok:
                raise ValueError(f"LogitConstraints: {what} must be an integer, got {v!r}")
            return int(v)

        def token(v, what):
            v = integer(v, what)
            if not 0 <= v < V:
                raise ValueError(f"LogitConstraints: {what} {v} is outside the vocabulary [0, {V})")
            return v

        if integer(max_positions, "max_positions") <= 0:
            raise ValueError(f"LogitConstraints: max_positions must be > 0, got {max_positions}")
        n = integer(no_repeat_ngram_size, "no_repeat_ngram_size")
        if not 0 <= n <= MAX_NGRAM:
            raise ValueError(f"LogitConstraints: no_repeat_ngram_size must be in 0..{MAX_NGRAM}, got {n}")
        if ngram_scope not in ("all", "generated"):
            raise ValueError(f"LogitConstraints: ngram_scope must be 'all' or 'generated', got {ngram_scope!r}")
        m = integer(min_new_tokens, "min_new_tokens")
        if m < 0:
            raise ValueError(f"LogitConstraints: min_new_tokens must be >= 0, got {m}")
        terms = [token(v, "terminator id") for v in (terminator_ids or [])]
        if len(terms) > MAX_TERMINATORS:
            raise ValueError(f"LogitConstraints: at most {MAX_TERMINATORS} terminator ids, got {len(terms)}")
        if m > 0 and not terms:
            raise ValueError("LogitConstraints: min_new_tokens needs terminator_ids")
        words = []
        for w in (bad_words_ids or []):
            w = [token(v, "bad_words_ids token") for v in w]
            if not 1 <= len(w) <= MAX_NGRAM:
                raise ValueError(f"LogitConstraints: a banned sequence has 1..{MAX_NGRAM} tokens, got {len(w)}")
            words.append(w)
        if len(words) > MAX_BAD_WORDS or sum(len(w) for w in words) > MAX_BAD_WORDS_TOKENS:
            raise ValueError(f"LogitConstraints: at most {MAX_BAD_WORDS} banned sequences and {MAX_BAD_WORDS_TOKENS} tokens in all")
        self.vocab_size, self.device, self.max_positions = V, torch.device(device), int(max_positions)
        self.no_repeat_ngram_size, self.ngram_scope, self.min_new_tokens = n, ngram_scope, m
        self.terminator_ids, self.bad_words_ids = terms, words
        self.neutral = n == 0 and m == 0 and not words
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)  # noqa: E731
        self._terms = i32(terms) if m > 0 else None
        self._bw_tokens = i32([v for w in words for v in w]) if words else None
        offs = [0]
        for w in words:
            offs.append(offs[-1] + len(w))
        self._bw_offsets = i32(offs) if words else None
        self.hist = torch.zeros(self.max_positions, dtype=torch.int32, device=self.device)
        self.gen_start = torch.zeros(1, dtype=torch.int32, device=self.device)

    def reset(self, prompt_tokens, gen_start):
        """A new sequence: the prefilled tokens (the inputs at positions 0 .. len - 1) go to hist[0 .. len-1] in one launch; positions
        from `gen_start` on count as generated.  What hist holds behind them is never read before it is written."""
        if self.neutral:
            return
        tokens = prompt_tokens.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        if tokens.numel() > self.max_positions:
            raise ValueError(f"LogitConstraints: {tokens.numel()} prompt tokens do not fit max_positions = {self.max_positions}")
        self.gen_start.fill_(int(gen_start))
        if tokens.numel() == 0:
            return
        if tokens.is_cuda:
            from . import glue

            glue.token_history_write(self.hist, tokens, 0)
        else:
            self.hist[:tokens.numel()] = tokens

    def record(self):
        """This sequence's row of glue.logits_constrain_streams: the state's tensors and the settings as the kernel receives them."""
        return (self.hist, self.gen_start, self.no_repeat_ngram_size, self.ngram_scope == "generated", self.min_new_tokens, self._terms,
                self._bw_tokens, self._bw_offsets)

    def apply(self, logits, tokens=None, pos=None, out=None):
        """logits [1, T, V], T <= 4: the rows of T steps at the consecutive positions pos[0] .. pos[0] + T - 1 (`pos`: at least one
        element, on the logits' device); tokens: those steps' input tokens (T elements), or None for the prefill's row, whose history
        is already in `hist` up to pos[0].  -> the constrained logits: a new tensor, or `logits` itself with out=logits (in place);
        hist[pos[0] + t] = tokens[t].  A row at a position outside [0, max_positions) is returned as it is and stores nothing."""
        if self.neutral:
            return logits
        if out is not None and out is not logits:
            raise ValueError("LogitConstraints: out must be None or the logits tensor itself")
        rows = logits[0]
        T = rows.shape[0]
        if rows.shape[1] != self.vocab_size:
            raise ValueError(f"LogitConstraints: logits have {rows.shape[1]} columns, the vocabulary has {self.vocab_size}")
        if pos is None or pos.numel() < 1:
            raise ValueError("LogitConstraints: apply needs the position of its first row")
        pos = pos.reshape(-1).to(torch.int32).contiguous()
        if tokens is not None:
            tokens = tokens.reshape(-1).to(torch.int32).contiguous()
            if tokens.numel() != T:
                raise ValueError(f"LogitConstraints: {T} rows need {T} tokens, got {tokens.numel()}")
        n, from_gen, m = self.no_repeat_ngram_size, self.ngram_scope == "generated", self.min_new_tokens
        if rows.is_cuda:
            from . import glue

            res = glue.logits_constrain(rows, self.hist, self.gen_start, tokens, pos, n, from_gen, m, self._terms, self._bw_tokens,
                                        self._bw_offsets, out=rows if out is not None else None)
        else:
            res = _constrain_host(rows, rows if out is not None else torch.empty_like(rows), self.hist, tokens, int(pos[0]),
                                  int(self.gen_start[0]), n, from_gen, m, self.terminator_ids if m > 0 else [], self.bad_words_ids)
        return logits if out is not None else res.unsqueeze(0)


def active(constraints):
    """`constraints` where it changes anything, None otherwise (None, or an object whose rules are all off)."""
    return None if constraints is None or constraints.neutral else constraints
