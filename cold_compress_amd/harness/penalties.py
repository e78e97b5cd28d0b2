"""Token-history penalties in front of the sampling tail: repetition_penalty (HF / vLLM: prompt and generated tokens),
frequency_penalty / presence_penalty (OpenAI / vLLM: generated tokens only) and logit_bias, with the history kept on the device
(include/coldcompress.h, cc_token_counts_add / cc_logits_penalize) so that a captured decode step advances through it.

The invariant every caller keeps: before step i runs, the counts are the histogram of prompt ‖ inputs of steps < i; step i's `apply`
adds its own input (the previously committed token, forced or free), which is always in device memory."""
import math

import torch


def _penalize_host(rows, prompt_count, gen_count, gen_start, tokens, pos, r, f, p, bias):
    """cc_logits_penalize's contract in torch fp32 on CPU tensors: rows [T, V] -> penalised rows; the counts advance in place."""
    T, V = rows.shape
    out = torch.empty_like(rows)
    for t in range(T):
        if tokens is not None:
            tok = int(tokens[t])
            if 0 <= tok < V:
                (gen_count if int(pos[t]) >= int(gen_start[0]) else prompt_count)[tok] += 1
        x = rows[t].float()
        if r != 1.0:
            seen = (prompt_count + gen_count) > 0
            rr = torch.tensor(r, dtype=torch.float32)
            x = torch.where(seen, torch.where(x > 0, x / rr, x * rr), x)
        if f != 0.0:
            x = x - torch.tensor(f, dtype=torch.float32) * gen_count.float()
        if p != 0.0:
            x = torch.where(gen_count > 0, x - torch.tensor(p, dtype=torch.float32), x)
        if bias is not None:
            x = x + bias
        out[t] = x.to(rows.dtype)
    return out


class LogitPenalties:
    """The settings and the device-resident state of the penalties for ONE sequence.  `logit_bias`: {token: float}, made into a dense
    fp32 [V] tensor once; -inf bans a token.  Invalid settings raise ValueError: a penalty that is not finite, repetition_penalty <= 0,
    a bias of +inf or NaN, a token outside the vocabulary.  An object whose settings are all neutral (`neutral`) behaves exactly as
    `penalties=None`: nothing is launched and nothing is counted.
    The three buffers (prompt_count, gen_count, gen_start) live as long as the object, so a captured graph can hold their addresses.
    CPU tensors run the same contract in torch fp32 (as `sample` does)."""

    def __init__(self, vocab_size, device, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None):
        V = int(vocab_size)
        if V <= 0:
            raise ValueError(f"LogitPenalties: vocab_size must be > 0, got {vocab_size}")
        f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))  # noqa: E731  (what the kernel receives)
        r, f, p = f32(repetition_penalty), f32(frequency_penalty), f32(presence_penalty)
        if not (math.isfinite(r) and r > 0):
            raise ValueError(f"LogitPenalties: repetition_penalty must be finite and > 0, got {repetition_penalty}")
        if not math.isfinite(f):
            raise ValueError(f"LogitPenalties: frequency_penalty must be finite, got {frequency_penalty}")
        if not math.isfinite(p):
            raise ValueError(f"LogitPenalties: presence_penalty must be finite, got {presence_penalty}")
        self.vocab_size, self.device = V, torch.device(device)
        self.repetition_penalty, self.frequency_penalty, self.presence_penalty = r, f, p
        self.bias = None
        if logit_bias:
            b = torch.zeros(V, dtype=torch.float32)
            for tok, val in logit_bias.items():
                if isinstance(tok, bool) or int(tok) != tok or not 0 <= int(tok) < V:
                    raise ValueError(f"LogitPenalties: logit_bias token {tok!r} is outside the vocabulary [0, {V})")
                val = float(val)
                if math.isnan(val) or val == math.inf:
                    raise ValueError(f"LogitPenalties: logit_bias[{tok}] must be finite or -inf, got {val}")
                b[int(tok)] = val
            if bool((b != 0).any()):
                self.bias = b.to(self.device)
        self.neutral = r == 1.0 and f == 0.0 and p == 0.0 and self.bias is None
        self.prompt_count = torch.zeros(V, dtype=torch.int32, device=self.device)
        self.gen_count = torch.zeros(V, dtype=torch.int32, device=self.device)
        self.gen_start = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._prompt = torch.zeros(0, dtype=torch.int32, device=self.device)

    # ---- state
    def _add(self, tokens, first_pos):
        tokens = tokens.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        if tokens.numel() == 0:
            return
        if tokens.is_cuda:
            from . import glue

            glue.token_counts_add(self.prompt_count, self.gen_count, tokens, first_pos, self.gen_start)
            return
        t = tokens.to(torch.int64)
        posn = int(first_pos) + torch.arange(t.numel())
        ok = (t >= 0) & (t < self.vocab_size)
        gen = posn >= int(self.gen_start[0])
        self.gen_count += torch.bincount(t[ok & gen], minlength=self.vocab_size).to(torch.int32)
        self.prompt_count += torch.bincount(t[ok & ~gen], minlength=self.vocab_size).to(torch.int32)

    def reset(self, prompt_tokens, gen_start):
        """A new sequence: zero counts, then the prompt (the inputs at positions 0 .. len - 1) in one launch.  Positions from
        `gen_start` on count as generated."""
        if self.neutral:
            return
        self._prompt = prompt_tokens.reshape(-1).to(device=self.device, dtype=torch.int32).clone()
        self.prompt_count.zero_()
        self.gen_count.zero_()
        self.gen_start.fill_(int(gen_start))
        self._add(self._prompt, 0)

    def rebuild(self, inputs, first_pos):
        """After a rewind: zero counts, the prompt kept at `reset` time, then `inputs` (the decode steps' inputs that stay committed,
        at positions first_pos ..)."""
        if self.neutral:
            return
        self.prompt_count.zero_()
        self.gen_count.zero_()
        self._add(self._prompt, 0)
        self._add(inputs, first_pos)

    def snapshot(self):
        return self.prompt_count.clone(), self.gen_count.clone(), self.gen_start.clone(), self._prompt

    def restore(self, snap):
        self.prompt_count.copy_(snap[0])
        self.gen_count.copy_(snap[1])
        self.gen_start.copy_(snap[2])
        self._prompt = snap[3]

    def record(self):
        """This sequence's row of glue.logits_penalize_streams: the state's tensors and the settings as the kernel receives them."""
        return (self.prompt_count, self.gen_count, self.gen_start, self.repetition_penalty, self.frequency_penalty, self.presence_penalty,
                self.bias)

    # ---- the step
    def apply(self, logits, tokens=None, pos=None):
        """logits [1, T, V], T <= 4: the rows of T steps; tokens / pos: those steps' input tokens and positions (T elements each, on the
        logits' device), or None for the prefill's row.  -> the penalised logits, a new tensor; the counts advance by `tokens`."""
        if self.neutral:
            return logits
        rows = logits[0]
        T = rows.shape[0]
        if rows.shape[1] != self.vocab_size:
            raise ValueError(f"LogitPenalties: logits have {rows.shape[1]} columns, the vocabulary has {self.vocab_size}")
        if tokens is not None:
            tokens = tokens.reshape(-1).to(torch.int32).contiguous()
            pos = pos.reshape(-1).to(torch.int32).contiguous()
            if tokens.numel() != T or pos.numel() != T:
                raise ValueError(f"LogitPenalties: {T} rows need {T} tokens and positions, got {tokens.numel()} and {pos.numel()}")
        if rows.is_cuda:
            from . import glue

            out = glue.logits_penalize(rows, self.prompt_count, self.gen_count, self.gen_start, tokens, pos, self.repetition_penalty,
                                       self.frequency_penalty, self.presence_penalty, self.bias)
        else:
            out = _penalize_host(rows, self.prompt_count, self.gen_count, self.gen_start, tokens, pos, self.repetition_penalty,
                                 self.frequency_penalty, self.presence_penalty, self.bias)
        return out.unsqueeze(0)


def active(penalties):
    """`penalties` where it changes anything, None otherwise (None, or an object whose settings are all neutral)."""
    return None if penalties is None or penalties.neutral else penalties
