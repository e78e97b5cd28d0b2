"""A plain float64 reference of the attention the kernels compute, with the reference's rounding points
(attention_utils.py:36-54 and model.py:413-418 of the original project; include/coldcompress.h, cc_decode_attn_gqa and
cc_prefill_attn_bands):

  score = dtype(dtype(q . k) * scale)          (q . k exact in float64 from the dtype operands)
  P     = dtype(softmax_float64(score))        (masked slots: -inf -> probability 0)
  y     = dtype(sum_s P[s] * v[s])             (accumulated in float64)
  gm    = dtype(mean over the R query heads of the group of P)

Group-query attention without repeating K / V: query head h * R + r reads kv head h.  Prefill side outputs (float64, what the
kernels return as f32): colsum[h, k] = sum over queries of gm; obs[h, k] = the mean of gm over the last obs_len query rows;
band[b, h, k] = sum over queries q in [k, k + bands[b]) of gm.  Every tensor stays on the device it came from; the queries of a
prefill are processed in chunks so that 8192 tokens with 28 query heads fit in GPU memory."""
import math

import torch


def rnd(x, dtype):
    """Round float64 values to `dtype` and back (the reference's rounding points)."""
    return x.to(dtype).to(torch.float64)


def _scale(D, scale):
    return 1.0 / math.sqrt(D) if scale is None else float(scale)


def decode_ref(q, k, v, mask=None, scale=None, dtype=None):
    """q [1, HQ, 1, D] (or [HQ, D]); k, v [1, H, S, D]; mask bool [1, H or HQ, 1, S] or None (a pre-repeated mask is read
    every R-th row, as attention_utils.decode_attention does).  -> (y [HQ, D], probs [HQ, S], gm [H, S]), float64 values that
    are exact in `dtype` (default: q's dtype)."""
    dtype = dtype or q.dtype
    H, S, D = k.shape[-3], k.shape[-2], k.shape[-1]
    HQ = q.numel() // D
    R = HQ // H
    assert R * H == HQ, (HQ, H)
    qd = q.reshape(H, R, D).to(torch.float64)
    kd = k.reshape(H, S, D).to(torch.float64)
    vd = v.reshape(H, S, D).to(torch.float64)
    sc = rnd(rnd(torch.einsum("hrd,hsd->hrs", qd, kd), dtype) * _scale(D, scale), dtype)
    if mask is not None:
        m = mask.reshape(-1, S)
        if m.shape[0] == HQ and R > 1:
            m = m[::R]
        sc = sc.masked_fill(~m.reshape(H, 1, S).to(sc.device), float("-inf"))
    p = rnd(torch.softmax(sc, dim=-1), dtype)
    y = rnd(torch.einsum("hrs,hsd->hrd", p, vd), dtype)
    gm = rnd(p.mean(dim=1), dtype)
    return y.reshape(HQ, D), p.reshape(HQ, S), gm


def prefill_ref(q, k, v, scale=None, dtype=None, obs_len=16, bands=(), chunk=None, need_side=True):
    """Causal prefill.  q [1, HQ, L, D]; k, v [1, H, L, D].  -> dict(y [HQ, L, D], and with need_side: colsum [H, L],
    obs [H, L], bands {width: [H, L]}), float64."""
    dtype = dtype or q.dtype
    H, L, D = k.shape[-3], k.shape[-2], k.shape[-1]
    HQ = q.shape[-3]
    R = HQ // H
    assert R * H == HQ, (HQ, H)
    qd = q.reshape(H, R, L, D).to(torch.float64)
    kd = k.reshape(H, L, D).to(torch.float64)
    vd = v.reshape(H, L, D).to(torch.float64)
    sc_f = _scale(D, scale)
    ol = min(obs_len, L)
    if chunk is None:  # about 64 MiB of float64 scores per chunk
        chunk = max(1, min(L, (8 << 20) // max(1, HQ * L)))
    dev = q.device
    y = torch.empty((H, R, L, D), dtype=torch.float64, device=dev)
    colsum = torch.zeros((H, L), dtype=torch.float64, device=dev)
    obs = torch.zeros((H, L), dtype=torch.float64, device=dev)
    band = {int(b): torch.zeros((H, L), dtype=torch.float64, device=dev) for b in bands}
    cols = torch.arange(L, device=dev)
    for i0 in range(0, L, chunk):
        i1 = min(L, i0 + chunk)
        rows = torch.arange(i0, i1, device=dev)
        sc = rnd(rnd(torch.einsum("hrid,hsd->hris", qd[:, :, i0:i1], kd[:, :i1]), dtype) * sc_f, dtype)
        live = cols[:i1].view(1, -1) <= rows.view(-1, 1)  # [c, i1] causal
        sc = sc.masked_fill(~live, float("-inf"))
        p = rnd(torch.softmax(sc, dim=-1), dtype)
        y[:, :, i0:i1] = rnd(torch.einsum("hris,hsd->hrid", p, vd[:, :i1]), dtype)
        if not need_side:
            continue
        gm = rnd(p.mean(dim=1), dtype)  # [H, c, i1], zero above the diagonal
        colsum[:, :i1] += gm.sum(dim=1)
        in_obs = rows >= L - ol
        if bool(in_obs.any()):
            obs[:, :i1] += gm[:, in_obs].sum(dim=1)
        for b, acc in band.items():
            near = (rows.view(-1, 1) - cols[:i1].view(1, -1)) < b
            acc[:, :i1] += (gm * near).sum(dim=1)
        del sc, p, gm
    out = dict(y=y.reshape(HQ, L, D))
    if need_side:
        out.update(colsum=colsum, obs=obs / ol if ol > 0 else obs, bands=band)
    return out


def ulp_of(dtype):
    """Unit roundoff scale used by the suite's tolerances: one rounding of the dtype at |x| ~ 1."""
    return {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
