"""Up to four sequences decoded in lock-step from ONE pass over the weights per step.

`DecodeStreams(model, n)` holds n cache sets for one model: stream 0 is the model's own per-layer caches, streams 1 .. n-1 are
further caches of the same classes and arguments.  `generate_streams` decodes n continuations of one prompt (fork: prefilled once)
or n different prompts (batch) through `Transformer.forward_streams` — every dense product one `cc_gemv_fused_multi` pass for the n
rows, every stream's cache step the existing launch on that stream's own cache — and one `cc_sample_rows` call per step.  Every
stream ends exactly where a lone `generate()` run of it ends: tokens, per-step probability rows or scores, and every cache buffer of
every layer, bit for bit."""
import collections
import time

import torch

from .. import _abi
from . import glue
from .constraints import LogitConstraints, active as _active_constraints
from .generation import (TokenScores, _clone_scores, _collective_status, _restore_l2_handoff, decode_one_token, greedy, sample,
                         token_logprobs)
from .penalties import LogitPenalties, active as _active_penalties

MAX_STREAMS = glue.GEMV_MULTI_MAX_T

# The logit processors of n streams: per stream a LogitPenalties / LogitConstraints or None (a neutral object is None
# here), and `key`, every object's settings as the kernels receive them — a captured step carries them by value, so two of these
# compare equal exactly where one captured step serves both (the objects themselves compare by identity).
Processors = collections.namedtuple("Processors", "pens cons key")


def processors(pens, cons):
    """-> the Processors of these per-stream objects (two sequences of n entries), or None where no stream has any."""
    pens, cons = tuple(_active_penalties(p) for p in pens), tuple(_active_constraints(c) for c in cons)
    if all(o is None for o in pens + cons):
        return None
    key = tuple(None if o is None else tuple(x.data_ptr() if torch.is_tensor(x) else x for x in o.record()) for o in pens + cons)
    return Processors(pens, cons, key)


def _per_stream(name, v, n, cls, vocab_size):
    """generate_streams' `penalties` / `constraints` -> n entries (an object of `cls` or None each), or ValueError."""
    if v is None:
        return (None,) * n
    if isinstance(v, cls):
        raise ValueError(f"generate_streams: {name} takes a list of {n} entries, one {cls.__name__} (or None) per stream — one object is "
                         f"one sequence's state; got a single {cls.__name__}")
    if not isinstance(v, (list, tuple)) or any(o is not None and not isinstance(o, cls) for o in v):
        raise ValueError(f"generate_streams: {name} must be a list or tuple of {cls.__name__} objects or None, one per stream")
    if len(v) != n:
        raise ValueError(f"generate_streams: {n} streams need {n} entries of {name}, got {len(v)}")
    given = [o for o in v if o is not None]
    if len({id(o) for o in given}) != len(given):
        raise ValueError(f"generate_streams: one {cls.__name__} appears twice in {name}: one object is one sequence's state")
    for o in given:
        if o.vocab_size != vocab_size:
            raise ValueError(f"generate_streams: {name} for a vocabulary of {o.vocab_size}, the model's has {vocab_size}")
    return tuple(v)


def _processed(logits, tok, pos, proc):
    """The rows the tokens are chosen from behind the streams' processors: row t of logits [1, n, V] penalised against stream t's
    counts and constrained over stream t's history, as decode_one_token does it for that stream alone (penalties first, constraints
    in place behind them; without penalties the constraints write a new tensor).  tok: the rows' input tokens [1, n], counted and
    stored at pos [n] — or None for the prefill's row, whose prompt the objects hold already.  -> [1, n, V], or None without `proc`.
    Device tensors: one launch per stage whatever n is (and the copy when constraints run alone); CPU tensors: the objects' own host
    contract, row by row."""
    if proc is None:
        return None
    pens, cons = proc.pens, proc.cons
    n = logits.shape[1]
    tokens = None if tok is None else tok.reshape(-1).to(torch.int32).contiguous()
    pos = pos.reshape(-1).to(torch.int32).contiguous()
    has_pen, has_con = any(p is not None for p in pens), any(c is not None for c in cons)
    if logits.is_cuda:
        out = logits[0]
        if has_pen:
            out = glue.logits_penalize_streams(out, [None if p is None else p.record() for p in pens], tokens, None if tokens is None else pos)
        if has_con:
            out = glue.logits_constrain_streams(out, [None if c is None else c.record() for c in cons], tokens, pos, out=out if has_pen else None)
        return out.unsqueeze(0)
    rows = []
    for t in range(n):
        row = logits[:, t:t + 1]
        tk, ps = None if tokens is None else tokens[t:t + 1], pos[t:t + 1]
        chosen = pens[t].apply(row, tk, ps) if pens[t] is not None else None
        if cons[t] is not None:
            chosen = cons[t].apply(chosen, tk, ps, out=chosen) if chosen is not None else cons[t].apply(row, tk, ps)
        rows.append(row if chosen is None else chosen)
    return torch.cat(rows, dim=1)


# host-side step state that reset() and the fused pipelines maintain beside the registered buffers
_HOST_STATE = ("_next_valid", "_quant_pending", "_state_fused")
_HYBRID_STATE = ("requires_heavy_hitter", "requires_punc", "requires_special")


class DecodeStreams:
    """n cache sets of one model (1 <= n <= glue.GEMV_MULTI_MAX_T), built after setup_caches: `sets[s][l]` is stream s's cache of
    layer l, `sets[0]` the model's own.  The further sets are built from what Transformer.setup_caches recorded for each layer
    (constructor, shape arguments, keyword arguments) on the device of the layer's own cache; a later setup_caches call needs a new
    DecodeStreams.  One cache set is 0.54 GB at the 8B shape with a cache of 4096 (32 layers x 2 x 8 heads x 4096 x 128 bf16)."""

    def __init__(self, model, n):
        if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_STREAMS:
            raise ValueError(f"DecodeStreams: n must be in 1..{MAX_STREAMS} (glue.GEMV_MULTI_MAX_T), got {n}")
        self.model, self.n, self.active = model, int(n), 0
        own = [layer.attention.kv_cache for layer in model.layers]
        if any(c is None for c in own) or not all(hasattr(layer.attention, "kv_cache_spec") for layer in model.layers):
            raise _abi.ColdCompressError("DecodeStreams is built after setup_caches")
        self.sets = [own] + [[self._build(layer.attention) for layer in model.layers] for _ in range(self.n - 1)]

    @staticmethod
    def _build(att):
        ctor, args, kw = att.kv_cache_spec
        src = att.kv_cache
        with torch.device(src.pos.device):
            cache = ctor(*args, **kw)
        for name, b in src._buffers.items():
            o = cache._buffers.get(name)
            if (b is None) != (o is None) or (b is not None and (b.shape != o.shape or b.dtype != o.dtype)):
                raise _abi.ColdCompressError(f"DecodeStreams: the layer's cache was changed after setup_caches (buffer {name}); call "
                                             "setup_caches again, then build the streams")
        return cache.train(src.training)

    def first(self, n):
        """The streams 0 .. n-1 as a DecodeStreams of their own that shares their caches (no new memory)."""
        if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= self.n:
            raise ValueError(f"DecodeStreams.first: n must be in 1..{self.n}, got {n}")
        view = object.__new__(DecodeStreams)
        view.model, view.n, view.active, view.sets = self.model, int(n), self.active, self.sets[:int(n)]
        return view

    def activate(self, s):
        """Make stream s's caches the layers' `attention.kv_cache` (and nothing else): prefill, the single-token step, statistics and
        GraphedDecoder then run on that stream untouched.  activate(0) restores the model."""
        if not 0 <= int(s) < self.n:
            raise ValueError(f"DecodeStreams.activate: stream {s} of {self.n}")
        for layer, cache in zip(self.model.layers, self.sets[int(s)]):
            layer.attention.kv_cache = cache
        self.active = int(s)

    def fork(self, src=0):
        """Copy stream `src`'s state to every other stream: every registered buffer (persistent or not) and the host-side step state
        beside them.  KVCacheRandom's per-generation seed is NOT copied: each stream draws its own when its pipeline is first seeded,
        as a fresh generation does, and evicts independently from there."""
        if not 0 <= int(src) < self.n:
            raise ValueError(f"DecodeStreams.fork: stream {src} of {self.n}")
        for s in range(self.n):
            if s != int(src):
                for a, b in zip(self.sets[int(src)], self.sets[s]):
                    _copy_cache_state(a, b)

    def reset(self):
        for caches in self.sets:
            for c in caches:
                c.reset()


def _copy_cache_state(a, b):
    for name, buf in a._buffers.items():
        if buf is not None:
            b._buffers[name].copy_(buf)
    for name in _HOST_STATE + _HYBRID_STATE:
        if hasattr(a, name):
            setattr(b, name, getattr(a, name))
    if hasattr(a, "cache_strategies"):  # hybrid: the per-head policies the prefill profiled
        cs = a.cache_strategies
        b.cache_strategies = cs.clone() if torch.is_tensor(cs) else cs
    if hasattr(a, "_ring_version"):  # the ring and its tracked window sums were copied together: in step where the source was
        b._ring_version = b._ring_tag() if a._ring_version == a._ring_tag() else None
    if hasattr(b, "_rng_seed"):  # random: keys scored under the source's seed are not this stream's; its pipeline is seeded again
        b._next_valid = False


def _choose(logits, pos, seeds, temperature, top_k, top_p, min_p, logprobs, chosen_from=None):
    """Row t of logits [1, n, V] -> its token, drawn as the lone step draws it (greedy, or seeded at pos[t] under seeds[t]), and what
    the lone step returns beside it.  -> (tokens [n] int32, probs [n, V]) or, with `logprobs`, (tokens, TokenScores of n).
    `chosen_from` (_processed): the rows behind the streams' logit processors — the tokens and the probability rows are theirs, the
    scores stay the model's own rows' (generation._scored)."""
    n = logits.shape[1]
    pick = logits if chosen_from is None else chosen_from
    if temperature is None:  # (softmax_argmax once per row: a rows form of that kernel is not part of this)
        picks = [greedy(pick[:, t:t + 1], None) for t in range(n)]
        tokens, probs = torch.cat([p[0].view(1) for p in picks]), torch.stack([p[1] for p in picks])
    elif logits.is_cuda:
        probs, tokens = glue.sample_rows(pick[0], temperature, top_k, top_p, min_p, seeds, pos.to(torch.int32).contiguous())
    else:
        picks = [sample(pick[:, t:t + 1], None, temperature, top_k, seeds[t], pos[t:t + 1], top_p=top_p, min_p=min_p) for t in range(n)]
        tokens, probs = torch.cat([p[0].view(1) for p in picks]), torch.stack([p[1] for p in picks])
    if logprobs:
        return tokens, TokenScores(*token_logprobs(logits, None, tokens))
    return tokens, probs


def _joint_step(model, streams, tok, pos, settings, attn_top_k=1.0):
    logits = model.forward_streams(tok, pos, streams, attn_top_k=attn_top_k)
    proc = settings[6] if len(settings) > 6 else None
    return _choose(logits, pos, *settings[:6], chosen_from=_processed(logits, tok, pos, proc))


class GraphedStreamsDecoder:
    """ONE joint step (Transformer.forward_streams + the sampling tail) of n streams captured in a hipGraph, on GraphedDecoder's
    pattern: the tokens `tok` [1, n] and positions `pos` [n] live in static device tensors that every kernel reads, the seeds and
    sampling settings are carried by value (other settings: capture again).  The warm-up steps run on a snapshot of all n cache sets;
    the state handed in is restored whether or not the capture succeeds.  The captured work is one linear stream of launches.
    `penalties` / `constraints`: per stream an object or None (`processors`).  The captured tail then holds the two streams launches
    with the addresses of the objects' buffers and their settings by value, all part of `settings`: other objects, or the same ones
    with other settings, capture again.  The warm-up steps count their inputs into the penalties' tables, so every stream's object
    is snapshotted beside the caches and restored with them; the constraints' histories need nothing (§2.21: the warm-up steps store
    positions at and behind the captured one, which the replays write again before anything reads them)."""

    def __init__(self, model, streams, seeds, temperature=None, top_k=None, top_p=None, min_p=None, logprobs=False, warmup=2,
                 penalties=None, constraints=None):
        self.model, self.streams, self.warmup = model, streams, warmup
        self.settings = (tuple(int(s) for s in seeds), temperature, top_k, top_p, min_p, bool(logprobs))
        none = (None,) * streams.n
        proc = processors(none if penalties is None else penalties, none if constraints is None else constraints)
        if proc is not None:  # (a seventh element only where a stream has a processor: six-element settings stay what they were)
            self.settings += (proc,)
        dev = model.output.weight.device
        self.tok = torch.zeros((1, streams.n), dtype=torch.int32, device=dev)
        self.pos = torch.zeros((streams.n,), dtype=torch.int32, device=dev)
        self.graph = None
        self.out_tok = self.out_probs = None
        self.replays = self.captures = 0

    def _caches(self):
        return [(t, c) for t, caches in enumerate(self.streams.sets) for c in caches]

    def _seed_pipelines(self):
        """prepare_decode sits OUTSIDE the captured step: every cache whose fused pipeline is not seeded (a prefill, a reset, a fork
        of such a cache) is seeded here, at its own stream's position."""
        for t, c in self._caches():
            if hasattr(c, "prepare_decode") and c.supports_fused_step() and not c._next_valid:
                c.prepare_decode(self.pos[t:t + 1])

    def _cache_epoch(self):
        return sum(int(getattr(c, "_graph_epoch", 0)) for _, c in self._caches())

    @staticmethod
    def _weights_epoch():
        return glue.w12_epoch() if glue.w12_enabled() else None

    def stale(self, settings):
        return (self.graph is None or settings != self.settings or self._cache_epoch() != self._epoch
                or self._weights_epoch() != self._w12_epoch)

    def capture(self):
        self._seed_pipelines()
        caches = [c for _, c in self._caches()]
        snap = [{k: v.clone() for k, v in c._buffers.items() if v is not None} for c in caches]
        flags = [(getattr(c, "_next_valid", None), getattr(c, "_quant_pending", False)) for c in caches]
        pos0 = self.pos.clone()
        proc = self.settings[6] if len(self.settings) > 6 else None
        pens = [p for p in proc.pens if p is not None] if proc is not None else []
        pen_snaps = [p.snapshot() for p in pens]  # (the warm-up steps and the captured step would be counted)
        self.captures += 1
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(self.warmup):  # positions advance like a real decode (the pipelines assume +1 steps)
                    _joint_step(self.model, self.streams, self.tok, self.pos, self.settings)
                    self.pos += 1
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.out_tok, self.out_probs = _joint_step(self.model, self.streams, self.tok, self.pos, self.settings)
            self.graph = graph
            self._epoch = self._cache_epoch()
            self._w12_epoch = self._weights_epoch()
        finally:  # also when the capture is refused: the caller falls back to eager joint steps and must find the state it handed in
            self.pos.copy_(pos0)
            for p, sn in zip(pens, pen_snaps):
                p.restore(sn)
            for c, sn, fl in zip(caches, snap, flags):
                for k, v in sn.items():
                    c._buffers[k].copy_(v)
                if fl[0] is not None:
                    c._next_valid = fl[0]
                c._quant_pending = fl[1]
                if hasattr(c, "_ring_version"):  # ring and tracked window sums were restored together: still in step
                    c._ring_version = c._ring_tag()

    def prepare(self, tok, pos, settings=None):
        """Capture (again) if there is no graph for these settings, or if something a captured step carries by value has moved."""
        settings = self.settings if settings is None else settings
        self.tok.copy_(tok)
        self.pos.copy_(pos)
        if self.graph is not None:
            self._seed_pipelines()  # (KVCacheRandom's first seeding moves the epoch)
        if self.stale(settings):
            self.settings, self.graph = settings, None
            self.capture()

    def __call__(self, tok, pos):
        self.prepare(tok, pos)
        self.tok.copy_(tok)
        self.pos.copy_(pos)
        self._seed_pipelines()
        self.graph.replay()
        self.replays += 1
        return self.out_tok, self.out_probs


def decode_streams(model, streams, tok, pos, num_steps, settings, terminator_ids=None, dec=None, joint=True, attn_top_k=1.0, log=print):
    """Up to `num_steps` lock-step decode steps of streams.n streams from the tokens `tok` [1, n] at the positions `pos` [n]
    (generate_streams' loop; tools/bench_streams.py times it).  settings: (seeds, temperature, top_k, top_p, min_p, logprobs) and,
    where a stream has logit processors, `processors(...)` as a seventh element (the objects hold their sequences' state already).
    `dec`: a GraphedStreamsDecoder whose captured step is replayed (a refused capture: eager joint steps from there on, a line through
    `log`); `joint` False: one stream at a time through activate(s) + decode_one_token.
    -> (per step the tokens [n], per step the rows [n, V] or TokenScores of n, per stream the number of steps it keeps or None while
    it has not emitted a terminator, the decoder or None)."""
    n = streams.n
    seeds, temperature, top_k, top_p, min_p, logprobs = settings[:6]
    proc = settings[6] if len(settings) > 6 else None  # (a seventh element: the streams' logit processors, `processors`)
    pens, cons = (proc.pens, proc.cons) if proc is not None else ((None,) * n, (None,) * n)
    skw = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, logprobs=logprobs)
    device = tok.device
    on_device = device.type == "cuda"
    step_toks, step_probs = [], []
    kept = [None] * n
    terminators = set(int(t) for t in terminator_ids) if terminator_ids else None
    for i in range(num_steps):
        if joint:
            if dec is not None and dec.stale(settings):
                try:
                    dec.prepare(tok, pos, settings)
                except Exception as e:  # capture refused: the state is as it was handed in (capture's finally)
                    if log is not None:
                        log(f"hipGraph capture of the joint step failed ({type(e).__name__}: {e}); falling back to eager joint steps")
                    dec = None
            nt, npb = dec(tok, pos) if dec is not None else _joint_step(model, streams, tok, pos, settings, attn_top_k)
            if on_device and _collective_status(device):
                from ..attention_utils import raise_single_launch_failure

                try:
                    raise_single_launch_failure(device)  # (clears the word)
                except Exception as e:
                    raise type(e)(f"in the joint decode step of {n} streams at positions {pos.tolist()}: {e}") from None
        else:  # one stream at a time: the existing single-token step on that stream's caches
            outs = []
            try:
                for s in range(n):
                    streams.activate(s)
                    outs.append(decode_one_token(model, tok[:, s:s + 1], pos[s:s + 1], attn_top_k=attn_top_k, seed=seeds[s],
                                                 penalties=pens[s], constraints=cons[s], **skw))
            finally:
                streams.activate(0)
            nt = torch.cat([o[0].view(1) for o in outs])
            npb = TokenScores(*(torch.cat(ts) for ts in zip(*(o[1] for o in outs)))) if logprobs else torch.stack([o[1] for o in outs])
        nt = nt.clone()
        step_toks.append(nt)
        step_probs.append(_clone_scores(npb) if logprobs else npb.clone())
        if terminators:
            for s, t in enumerate(nt.tolist()):
                if kept[s] is None and t in terminators:
                    kept[s] = i + 1  # (the terminator itself is committed, as the lone loop commits it)
            if all(k is not None for k in kept):
                break
        tok = nt.view(1, n).to(torch.int32)
        pos = pos + 1
    return step_toks, step_probs, kept, dec


_NOT_SERVED = ("top_logprobs", "next_tokens", "feed_long_prompts", "decode_first_token")


@torch.no_grad()
def generate_streams(model, prompts, prefill, max_new_tokens, n_streams=None, seeds=None, terminator_ids=None, temperature=None,
                     top_k=None, top_p=None, min_p=None, logprobs=False, graph=True, streams=None, log=print, **kw):
    """n sequences decoded in lock-step -> (seqs: n 1-D tensors, probs: per stream the list of probability rows or, with `logprobs`,
    a TokenScores, stats).  Stream s equals generate(model, prompt_s, prefill, decode_one_token, max_new_tokens, seed=seeds[s], ...)
    on a fresh model: tokens, rows or scores and every cache buffer of every layer, bit for bit.
    `prompts`: ONE 1-D tensor with `n_streams` — fork: n continuations of the prompt, prefilled once into stream 0 and copied
    (DecodeStreams.fork), the n first tokens drawn from the prefill's last row under the n seeds — or a LIST of 1-D tensors — batch:
    stream s is prefilled with prompt s and its first token drawn as `prefill` draws it.  `seeds`: n integers (default 0 .. n-1);
    `temperature` None: greedy.  `prefill`: the caller's callable, as generate() takes it.  A stream that has emitted a terminator is
    finished: it keeps stepping, its results are discarded, and what it returns ends where the lone run stops; the loop ends when all
    streams are finished or after `max_new_tokens`.  `graph` (device tensors): one joint step is captured (GraphedStreamsDecoder); a
    refused capture falls back to eager joint steps with a line through `log`.  The single-launch status word is read once behind
    every joint step and a set word raises, with the step's positions: a joint step cannot be rewound token-wise.
    A model that is not `streams_eligible` (int4 weights without `model.block_int4`, a cache quantising in reference mode, attn_top_k < 1, more than one rank)
    runs its streams one at a time per step through activate(s) + decode_one_token: the same results, no speed-up.
    `penalties` / `constraints`: a LIST or TUPLE of n entries, each a LogitPenalties / LogitConstraints or None, one
    per stream — one object is one sequence's state, so a single object, a wrong length, one object twice, a vocabulary that is not
    the model's or constraints whose `max_positions` is below the stream's prompt length + max_new_tokens raise ValueError before the
    prefill.  Every object is reset with its stream's prompt (gen_start = the prompt's length), as generate() resets it; stream s then
    equals generate(..., penalties=<its object>, constraints=<its object>).  A joint step puts its n rows through ONE
    cc_logits_penalize_streams and ONE cc_logits_constrain_streams launch, both captured with the step; a neutral object is None.
    A finished stream keeps stepping, so its objects' state runs on past its terminator: afterwards it is NOT the lone run's.
    Not served (ValueError before any launch): top_logprobs, next_tokens, feed_long_prompts, decode_first_token — their state is per
    sequence — and a prompt exactly as long as the smallest cache, which generate() splits into a prefill and a forced step.  On
    return stream 0 is active: the model is as a plain generate() leaves it.
    `streams`: a DecodeStreams to use (default: one built for this call).  `decoder`: a GraphedStreamsDecoder built for `streams` to
    use instead of a new one — its captured step is replayed where the settings are the ones it was captured with, the processors'
    among them, and captured again where they are not."""
    attn_top_k = kw.pop("attn_top_k", 1.0)
    penalties, constraints, decoder = kw.pop("penalties", None), kw.pop("constraints", None), kw.pop("decoder", None)
    for name in _NOT_SERVED:
        v = kw.pop(name, None)
        if v is not None and v is not False:
            raise ValueError(f"generate_streams does not serve {name}: its state is per sequence (run generate() per sequence)")
    if kw:
        raise TypeError(f"generate_streams: unexpected arguments {sorted(kw)}")
    fork = torch.is_tensor(prompts)
    if fork:
        n = n_streams if n_streams is not None else (streams.n if streams is not None else None)
        if n is None:
            raise ValueError("generate_streams: one prompt (fork) needs n_streams")
        plist = [prompts]
    else:
        plist = list(prompts)
        n = len(plist)
        if n_streams is not None and int(n_streams) != n:
            raise ValueError(f"generate_streams: {n} prompts but n_streams = {n_streams}")
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_STREAMS:
        raise ValueError(f"generate_streams: 1..{MAX_STREAMS} streams, got {n}")
    n = int(n)
    seeds = list(range(n)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != n:
        raise ValueError(f"generate_streams: {n} streams need {n} seeds, got {len(seeds)}")
    if streams is not None and streams.n != n:
        raise ValueError(f"generate_streams: the DecodeStreams holds {streams.n} streams, the call asks for {n}")
    if int(max_new_tokens) < 1:
        raise ValueError(f"generate_streams: max_new_tokens must be >= 1, got {max_new_tokens}")
    min_cache_length = model.min_cache_length()
    for p in plist:
        if not (torch.is_tensor(p) and p.dim() == 1 and p.numel() >= 1):
            raise ValueError("generate_streams: every prompt is a non-empty 1-D tensor")
        if p.numel() == min_cache_length:
            raise ValueError(f"generate_streams: a prompt of {p.numel()} tokens is as long as the smallest cache ({min_cache_length}): "
                             "generate() splits it and forces its last token through a decode step, which is not served here")
    device, dtype = plist[0].device, plist[0].dtype
    vocab_size = model.output.weight.shape[0]
    pens = _per_stream("penalties", penalties, n, LogitPenalties, vocab_size)
    cons = _per_stream("constraints", constraints, n, LogitConstraints, vocab_size)
    for s, c in enumerate(cons):
        L = int(plist[0 if fork else s].numel())
        if _active_constraints(c) is not None and L + int(max_new_tokens) > c.max_positions:
            raise ValueError(f"generate_streams: stream {s}: {L} prompt tokens and {max_new_tokens} new ones do not fit the constraints' "
                             f"max_positions = {c.max_positions}")
    if decoder is not None and (decoder.model is not model or (streams is not None and decoder.streams is not streams)):
        raise ValueError("generate_streams: decoder was built for another model or another DecodeStreams")
    proc = processors(pens, cons)
    if streams is None:
        streams = decoder.streams if decoder is not None else DecodeStreams(model, n)
        if streams.n != n:
            raise ValueError(f"generate_streams: the decoder's DecodeStreams holds {streams.n} streams, the call asks for {n}")
    settings = (tuple(seeds), temperature, top_k, top_p, min_p, bool(logprobs)) + (() if proc is None else (proc,))
    skw = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, logprobs=bool(logprobs))
    on_device = device.type == "cuda"
    joint = bool(model.streams_eligible(streams, attn_top_k))
    _restore_l2_handoff()

    def sync():
        if on_device:
            torch.cuda.synchronize(device)

    try:
        # ---- prefill and the n first tokens
        lengths = [int(p.numel()) for p in plist] * (n if fork else 1)
        if proc is not None:  # every stream's objects hold its prompt; positions from its length on count as generated (generate())
            for s, objs in enumerate(zip(proc.pens, proc.cons)):
                for o in objs:
                    if o is not None:
                        o.reset(plist[0 if fork else s], lengths[s])
        sync()
        t0 = time.perf_counter()
        if fork:
            L = lengths[0]
            streams.activate(0)
            last = []
            hook = model.register_forward_hook(lambda m, a, out: last.append(out[:, -1:]))
            try:
                prefill(model, plist[0].view(1, -1), torch.arange(0, L, device=device), seed=seeds[0], **skw)
            finally:
                hook.remove()
            streams.fork(0)
            row = last[-1]
            pos = torch.full((n,), L - 1, dtype=torch.int32, device=device)
            rows = row.expand(1, n, row.shape[-1]).contiguous()  # (the prompt is counted and stored already: tok None)
            first_tok, first_probs = _choose(rows, pos, *settings[:6], chosen_from=_processed(rows, None, pos, proc))
            first_tok = first_tok.clone()
            first_probs = _clone_scores(first_probs) if logprobs else first_probs.clone()
        else:
            toks, rows = [], []
            for s, p in enumerate(plist):
                streams.activate(s)
                pkw = dict(penalties=proc.pens[s], constraints=proc.cons[s]) if proc is not None else {}
                ret = prefill(model, p.view(1, -1), torch.arange(0, p.numel(), device=device), seed=seeds[s], **pkw, **skw)
                toks.append(ret[0].clone().view(1))
                rows.append(_clone_scores(ret[1]) if logprobs else ret[1].clone())
            streams.activate(0)
            first_tok = torch.cat(toks)
            first_probs = TokenScores(*(torch.cat(ts) for ts in zip(*rows))) if logprobs else torch.stack(rows)
        sync()
        t1 = time.perf_counter()

        # ---- joint steps
        tok = first_tok.view(1, n).to(torch.int32)
        pos = torch.tensor(lengths, dtype=torch.int32, device=device)
        dec = None
        if graph and on_device and joint:
            dec = decoder if decoder is not None else GraphedStreamsDecoder(model, streams, seeds, temperature, top_k, top_p, min_p, logprobs,
                                                                            penalties=pens, constraints=cons)
        step_toks, step_probs, kept, dec = decode_streams(model, streams, tok, pos, int(max_new_tokens) - 1, settings, terminator_ids, dec,
                                                          joint, attn_top_k, log)
        sync()
        t2 = time.perf_counter()
        if on_device:  # fail loudly, as generate() does
            from ..attention_utils import raise_single_launch_failure

            if _collective_status(device):
                raise_single_launch_failure(device)
    finally:
        streams.activate(0)

    # ---- per-stream results, trimmed where the lone run stops
    seqs, probs, counts = [], [], []
    for s in range(n):
        k = len(step_toks) if kept[s] is None else kept[s]
        prompt = plist[0] if fork else plist[s]
        seqs.append(torch.cat([prompt, first_tok[s:s + 1].to(dtype)] + [t[s:s + 1].to(dtype) for t in step_toks[:k]]))
        if logprobs:
            parts = [type(first_probs)(*(x[s:s + 1] for x in first_probs))] + [type(p)(*(x[s:s + 1] for x in p)) for p in step_probs[:k]]
            probs.append(type(first_probs)(*(torch.cat(ts) for ts in zip(*parts))))
        else:
            probs.append([first_probs[s]] + [p[s] for p in step_probs[:k]])
        counts.append(k + 1)
    total, prefilled = sum(counts), sum(int(p.numel()) for p in plist)
    stats = {
        "prefill_tokens": prefilled, "decode_tokens": counts, "streams": n, "joint_steps": bool(joint),
        "graphed": dec is not None and dec.graph is not None, "captures": dec.captures if dec is not None else 0,
        "decode_tokens_total": total,
        "prefill_toks_per_sec": prefilled / (t1 - t0), "decode_toks_per_sec": total / (t2 - t1),
        "total_toks_per_sec": total / (t2 - t0), "total_seconds": t2 - t0, "prefill_seconds": t1 - t0,
        "decode_seconds": t2 - t1, "decode_seconds_frac_of_total": (t2 - t1) / (t2 - t0),
        "memory_used_gb": (torch.cuda.max_memory_reserved() / 1e9) if on_device else 0.0,
    }
    return seqs, probs, stats
