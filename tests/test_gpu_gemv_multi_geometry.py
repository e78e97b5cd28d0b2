"""The launch geometries pick_multi_cfg adopted for 16-bit rows at T = 3 and 4 (csrc/cc_gemv.hip, profiles/gemv_multi_geometry.md):
results do not depend on the geometry, so at every adopted (shape class, T) the multi launch must equal T single launches bit for bit.
The class is picked by K — 4096 (XS = 2) or 14336 (XS = 8), the 8B model's — on a 64-row bf16 matrix, and the rules that hang on the
number of row groups are also run at the smallest odd row counts that reach them:
  * long plain rows (w2's class) at T = 4 run at 2 x 4 instead of 4 x 4: 64 rows, and 1091 (more than one round of 512 workgroups);
  * the SwiGLU pair at K = 4096, T = 3 and 4, runs under at most 1024 workgroups instead of 2048: 64 rows, and 2307 (a second round);
  * short plain rows whose groups of 4 rows are no whole number of rounds of 1024 workgroups (wqkv: 6144 rows, with the norm
    prologue and the RoPE epilogue) run under 512 at T = 3 and 4; 4096 rows (wo) keep 1024.
T = 2 rides along at every shape: it keeps pick_cfg's choice."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
D = 128


def _inputs(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.05).to(BF).to(DEV)
    x = torch.randn(4, K, generator=g).to(BF).to(DEV)
    return g, W, x


def _same(what, multi, singles):
    for t, s in enumerate(singles):
        assert torch.equal(multi[t].view(torch.int16), s.view(-1).view(torch.int16)), f"{what}: row {t} differs from the single launch"


@pytest.mark.parametrize("T", [2, 3, 4])
@pytest.mark.parametrize("N", [64, 1091])
def test_long_plain_rows(N, T):
    from cold_compress_amd.harness import glue

    _, W, x = _inputs(N, 14336, 1)
    _same(f"w2 class N={N} T={T}", glue.gemv_fused_multi(W, x[:T]), [glue.gemv_fused(W, x[t]) for t in range(T)])


@pytest.mark.parametrize("T", [2, 3, 4])
@pytest.mark.parametrize("N", [64, 2307])
def test_swiglu_pair(N, T):
    from cold_compress_amd.harness import glue

    g, W, x = _inputs(N, 4096, 2)
    W3 = (torch.randn(N, 4096, generator=g) * 0.05).to(BF).to(DEV)
    delta = torch.randn(4, 4096, generator=g).to(BF).to(DEV)
    nw = (1 + 0.1 * torch.randn(4096, generator=g)).to(BF).to(DEV)
    hm, hs = torch.empty_like(x[:T]), [torch.empty_like(x[0]) for _ in range(T)]
    multi = glue.gemv_fused_multi(W, x[:T], w3=W3, delta=delta[:T], norm_weight=nw, h_out=hm)
    singles = [glue.gemv_fused(W, x[t], w3=W3, delta=delta[t], norm_weight=nw, h_out=hs[t]) for t in range(T)]
    _same(f"pair N={N} T={T}", multi, singles)
    _same(f"pair N={N} T={T}, h_out", hm, hs)


@pytest.mark.parametrize("T", [2, 3, 4])
@pytest.mark.parametrize("N", [64, 4096, 6144])
def test_short_plain_rows(N, T):
    """wqkv's form: norm prologue, RoPE on all but the last 1024 rows (64 rows: on the first 48 with 16-wide heads)."""
    from cold_compress_amd.harness import glue

    g, W, x = _inputs(N, 4096, 3)
    hd = D if N > 64 else 16
    rope = N - 1024 if N > 64 else 48
    delta = torch.randn(4, 4096, generator=g).to(BF).to(DEV)
    nw = (1 + 0.1 * torch.randn(4096, generator=g)).to(BF).to(DEV)
    freqs = torch.randn(4, hd // 2, 2, generator=g).to(BF).to(DEV)
    hm, hs = torch.empty_like(x[:T]), [torch.empty_like(x[0]) for _ in range(T)]
    multi = glue.gemv_fused_multi(W, x[:T], delta=delta[:T], norm_weight=nw, h_out=hm, freqs=freqs[:T], rope_rows=rope, head_dim=hd)
    singles = [glue.gemv_fused(W, x[t], delta=delta[t], norm_weight=nw, h_out=hs[t], freqs=freqs[t], rope_rows=rope, head_dim=hd) for t in range(T)]
    _same(f"wqkv class N={N} T={T}", multi, singles)
    _same(f"wqkv class N={N} T={T}, h_out", hm, hs)
