"""The contract of cc_logits_penalize / cc_token_counts_add (include/coldcompress.h) in torch fp32 on CPU tensors, an independent
scalar restatement of it in numpy.float32 with integer counts, the input families and the cases both test files walk.

Everything is compared BIT FOR BIT (NaNs as a class): every fp32 operation of the contract is a single IEEE operation rounded to
nearest, and the result is rounded once to the model dtype, so there is no tolerance to choose."""
import functools

import numpy as np
import torch

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
FAMILIES = ("normal", "peaked", "equal", "zeros", "subnormal", "inf", "nan")
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
# (repetition, frequency, presence): each on alone, then all together
SETTINGS = ((1.3, 0.0, 0.0), (0.7, 0.0, 0.0), (1.0, 0.4, 0.0), (1.0, -0.25, 0.0), (1.0, 0.0, 0.6), (1.2, 0.3, 0.5))
ALL_ON = SETTINGS[-1]


@functools.lru_cache(maxsize=None)
def family(name, dtype, V, T=4):
    """-> rows [T, V] of `dtype` (CPU)."""
    g = torch.Generator().manual_seed(7919 * FAMILIES.index(name) + 13 * V + DTYPES.index(dtype))
    base = torch.randn(T, V, generator=g)
    if name == "normal":
        x = base * 4
    elif name == "peaked":
        x = base.clone()
        x[torch.arange(T), torch.randint(0, V, (T,), generator=g)] += 20
    elif name == "equal":
        x = torch.full((T, V), 1.5)
    elif name == "zeros":  # exact zeros of both signs: x > 0 is false for both, the product branch is taken (and keeps the sign)
        x = torch.where(torch.arange(T * V).view(T, V) % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0))
    elif name == "subnormal":  # the dtype's own subnormals, both signs: k * (smallest subnormal), k up to the mantissa's width
        iv = _INT[dtype]
        mag = torch.randint(1, {torch.float32: 1 << 23, torch.bfloat16: 1 << 7, torch.float16: 1 << 10}[dtype], (T, V), generator=g).to(iv)
        neg = torch.randint(0, 2, (T, V), generator=g).bool()
        sign = torch.full((T, V), torch.iinfo(iv).min, dtype=iv)  # (the sign bit alone)
        return torch.where(neg, mag | sign, mag).view(dtype)
    elif name == "inf":
        x = base * 3
        x[:, 0::5] = float("inf")
        x[:, 2::5] = -float("inf")
    elif name == "nan":
        x = base * 3
        x[torch.arange(T), torch.randint(0, V, (T,), generator=g)] = float("nan")
    else:
        raise KeyError(name)
    return x.to(dtype)


def counts(V, seed=0):
    """-> (prompt_count, gen_count) int32 [V]: about half the elements zero in each, so that all four seen / generated cases occur."""
    g = torch.Generator().manual_seed(101 * V + seed)
    pc = torch.randint(0, 4, (V,), generator=g, dtype=torch.int32) * torch.randint(0, 2, (V,), generator=g, dtype=torch.int32)
    gc = torch.randint(0, 5, (V,), generator=g, dtype=torch.int32) * torch.randint(0, 2, (V,), generator=g, dtype=torch.int32)
    return pc, gc


GEN_START = 100


def block_inputs(V, T):
    """-> (tokens, pos) python lists of T elements: a duplicate inside the block, 0 and V - 1, -1 and V (which count nothing), and
    positions on both sides of GEN_START."""
    toks = {1: [V - 1], 2: [0, 0], 3: [V - 1, -1, V - 1], 4: [0, V, V - 1, 0]}[T]
    pos = [GEN_START - 2 + t for t in range(T)]  # the first two are prompt, the rest generated
    return toks, pos


def bias_vec(V, seed=0):
    g = torch.Generator().manual_seed(977 * V + seed)
    b = torch.randn(V, generator=g) * 2
    b[torch.rand(V, generator=g) < 0.5] = 0.0
    b[V // 2] = -float("inf")
    return b


def twin(rows, prompt_count, gen_count, gen_start, tokens, pos, r, f, p, bias):
    """The contract in torch fp32.  rows [T, V]; counts int32 [V] (not modified); tokens / pos: T ints each or None.
    -> (out [T, V] of rows' dtype, prompt_count', gen_count')."""
    T, V = rows.shape
    cp, cg = prompt_count.clone(), gen_count.clone()
    out = torch.empty_like(rows)
    r32, f32, p32 = (torch.tensor(v, dtype=torch.float32) for v in (r, f, p))
    for t in range(T):
        if tokens is not None and 0 <= int(tokens[t]) < V:
            (cg if int(pos[t]) >= int(gen_start) else cp)[int(tokens[t])] += 1
        x = rows[t].float()
        if float(r32) != 1.0:
            x = torch.where((cp + cg) > 0, torch.where(x > 0, x / r32, x * r32), x)
        if float(f32) != 0.0:
            x = x - (f32 * cg.float())
        if float(p32) != 0.0:
            x = torch.where(cg > 0, x - p32, x)
        if bias is not None:
            x = x + bias
        out[t] = x.to(rows.dtype)
    return out, cp, cg


def _round_to(v, dtype):
    """one round-to-nearest-even of the np.float32 `v` to `dtype`, returned as np.float32 (restated on the bits for bf16)."""
    if dtype == torch.float32:
        return v
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            return np.float32(np.float16(v))
    if v != v:
        return v
    u = int(np.array(v, dtype=np.float32).view(np.uint32))
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return np.array(u, dtype=np.uint32).view(np.float32)[()]


def scalar_restatement(rows, prompt_count, gen_count, gen_start, tokens, pos, r, f, p, bias):
    """The issue's pseudo-code, element by element, in numpy.float32 scalars and python integers.  -> (out fp32 [T, V] holding the
    rounded values, prompt_count', gen_count' as lists)."""
    T, V = rows.shape
    x_in = rows.float().numpy()
    out = np.empty((T, V), dtype=np.float32)
    cps, cgs = [int(c) for c in prompt_count], [int(c) for c in gen_count]
    r, f, p = np.float32(r), np.float32(f), np.float32(p)
    b = None if bias is None else bias.numpy()
    with np.errstate(all="ignore"):
        for v in range(V):
            cp, cg = cps[v], cgs[v]
            for t in range(T):
                if tokens is not None and tokens[t] == v:
                    if pos[t] >= gen_start:
                        cg += 1
                    else:
                        cp += 1
                x = x_in[t, v]
                if r != 1 and cp + cg > 0:
                    x = np.float32(x / r) if x > 0 else np.float32(x * r)
                if f != 0:
                    x = np.float32(x - np.float32(f * np.float32(cg)))
                if p != 0 and cg > 0:
                    x = np.float32(x - p)
                if b is not None:
                    x = np.float32(x + b[v])
                out[t, v] = _round_to(x, rows.dtype)
            cps[v], cgs[v] = cp, cg
    return out, cps, cgs


def same_bits(a, b):
    """a, b of one dtype and shape: equal bit for bit, NaNs compared as a class."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    iv = _INT[a.dtype]
    za, zb = torch.zeros_like(a), torch.zeros_like(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(torch.where(na, za, a).view(iv), torch.where(nb, zb, b).view(iv)))
