#!/usr/bin/env python3
"""The tensor-parallel PRODUCT path (cache + attention kernels under cold_compress_amd.tp) at TP = N against the unsharded
model on the same weights: tokens equal, layer-0 evictions identical.

  --backend nccl  : one GPU per rank, RCCL all-reduces over xGMI (what tp.py:41-56, 124-176 does with NCCL); with --graph
                    the sharded decode step, collectives included, is replayed from a hipGraph
  --backend gloo  : every rank drives cuda:0 and the collectives are staged over the host — no RCCL, but every kernel of
                    the sharded decode path runs for real (what a 1-GPU box can check); with --oneshot the decode-size
                    all-reduces go through cc_allreduce_sum (IPC-mapped buffers of the two ranks on the one GPU) and --graph
                    replays the sharded decode step, those collectives included, from a hipGraph
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29541 \
        tools/tp2_check.py [--backend nccl --graph]"""
import argparse
import copy
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from cold_compress_amd import tp  # noqa: E402
from cold_compress_amd.harness import CONFIGS, ModelArgs, Transformer, decode_one_token, prefill, setup_caches  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["gloo", "nccl"], default="gloo")
    ap.add_argument("--graph", action="store_true", help="replay the sharded decode step from a hipGraph (collectives captured)")
    ap.add_argument("--oneshot", action="store_true", help="decode-size all-reduces over the one-shot transport (cc_allreduce_sum), after its self-test")
    ap.add_argument("--model", default="Meta-Llama-3.1-8B-Instruct", help="harness.CONFIGS key; Llama-3-70B-shape = BASELINE C5 (two layers of it)")
    ap.add_argument("--no_fuse_gemv", action="store_true", help="debugging: the sharded model's dense layers through torch (hipBLASLt)")
    ap.add_argument("--no_fuse_step", action="store_true", help="debugging: the sharded model's caches through the three-call path")
    ap.add_argument("--one_rank_per_gpu", action="store_true", help="gloo: rank r drives GPU r instead of every rank driving cuda:0")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=0, help="override the vocabulary size (0: the config's) — keeps eight ranks' host copies small")
    ap.add_argument("--cache", type=int, default=128, help="cache slots per layer (C5: 3488)")
    ap.add_argument("--prompt", type=int, default=300, help="prompt tokens (> --cache: the prompt is compacted)")
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if args.backend == "nccl":
        assert torch.cuda.device_count() >= world, f"{world} ranks need {world} GPUs (found {torch.cuda.device_count()})"
        torch.cuda.set_device(rank)
        dev = torch.device("cuda", rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        assert dist.get_backend() == "nccl" and dist.get_world_size() == world
    else:
        d = rank if args.one_rank_per_gpu else 0
        torch.cuda.set_device(d)
        dev = torch.device("cuda", d)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        orig = dist.all_reduce

        def staged(t, op=dist.ReduceOp.SUM, **kw):  # gloo without device support: sum on the host in fp32, round once
            if t.is_cuda:
                c = t.float().cpu()
                orig(c, op=op)
                t.copy_(c.to(t.dtype))
                return None
            return orig(t, op=op, **kw)

        dist.all_reduce = staged
    if args.backend == "gloo" and args.cache >= 1024:
        # every rank shares cuda:0 and runs its kernels CONCURRENTLY with the others': a single-launch step needs all of its workgroups
        # resident at once, which eight processes streaming full-size caches do not grant each other (measured, r5: hand-off timeouts,
        # different garbage in every run — this harness drives decode_one_token without the recovery loop).  The documented switch for
        # shared devices: the two-launch forms (same arithmetic, bit-identical cache state).
        from cold_compress_amd.attention_utils import set_device_single_launch

        set_device_single_launch(torch.device("cuda", torch.cuda.current_device()), False)  # (r6: the per-device knob of the boundary header)
    if args.oneshot:
        assert tp.enable_oneshot_allreduce() is not None, "the one-shot all-reduce did not pass its self-test"
    cfg = dict(CONFIGS[args.model])
    cfg["n_layer"] = args.layers
    cfg["block_size"] = max(1024, args.prompt + 128)
    if args.vocab:
        cfg["vocab_size"] = args.vocab
    torch.manual_seed(77)
    ref = Transformer(ModelArgs(**cfg)).to(torch.bfloat16).eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(77)
        for n, p in ref.named_parameters():
            p.fill_(1.0) if "norm" in n else p.normal_(0.0, 0.02, generator=g)
    sharded = copy.deepcopy(ref)
    ref = ref.to(dev)
    tp.apply_tp(sharded)
    sharded = sharded.to(dev)
    for l in sharded.layers:
        l.fuse_gemv = not args.no_fuse_gemv
        l.attention.fuse_decode_step = not args.no_fuse_step
    kw = dict(max_cache_length=[float(args.cache)], cache_bits=None, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
              cache_strategy_pattern="tile", feed_long_prompts=False, prompt_compression_strategy=["heavy_hitter"], global_tokens=4,
              recent_window=10, history_window_size=1, attn_thresholding=False, min_recovery_frac=0.9)
    outs = []
    L = args.prompt
    prompt = torch.randint(0, cfg["vocab_size"], (L,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(dev)
    for name, model in (("tp1", ref), ("tp2", sharded)):
        setup_caches(model, None, dev, L + 100, dict(kw))
        with torch.no_grad():
            tok, probs = prefill(model, prompt.view(1, -1), torch.arange(L, device=dev))
            pos = torch.tensor([L], dtype=torch.int32, device=dev)
            toks, plist = [int(tok)], [probs.float().clone()]
            cur = tok.view(1, 1).to(torch.int32)
            step = decode_one_token
            if args.graph and name == "tp2":
                from cold_compress_amd.harness import GraphedDecoder

                step = GraphedDecoder(model)  # capture fails loudly if a collective cannot be captured
            for _ in range(12):
                # teacher-force the unsharded model's tokens so that both runs see the same inputs
                nt, pr = step(model, cur, pos)
                plist.append(pr.float().clone())
                toks.append(int(nt))
                cur = (nt if name == "tp1" else torch.tensor(outs[0][0][len(toks) - 1], device=dev)).view(1, 1).to(torch.int32)
                pos += 1
        torch.cuda.synchronize()
        outs.append((toks, plist, [l.attention.kv_cache.pos.clone() for l in model.layers]))
    ok = True
    H = cfg["n_local_heads"] // world
    for i, (a, b) in enumerate(zip(outs[0][1], outs[1][1])):
        rel = float((a - b).abs().max() / a.abs().max())
        if rel > 0.25:  # random weights: near-uniform probabilities, the all-reduce rounds the residual stream differently
            ok = False
        if rank == 0:
            print(f"step {i}: token tp1 {outs[0][0][i]} tp2 {outs[1][0][i]}  max|dp|/max p = {rel:.4f}", flush=True)
    agree, differ = [], []
    for l, (pa, pb) in enumerate(zip(outs[0][2], outs[1][2])):
        mine = pa[:, rank * H:(rank + 1) * H]
        differ.append(int((mine != pb).sum()))
        agree.append(1.0 if differ[-1] == 0 else 1.0 - differ[-1] / mine.numel())
    print(f"rank {rank}: cache slots holding a different position than in the unsharded run, per layer: {differ}", flush=True)
    same_tokens = sum(int(x == y) for x, y in zip(outs[0][0], outs[1][0]))
    # a differing greedy token must be a near-tie of the UNSHARDED model's own distribution (random weights: near-uniform
    # probabilities; the all-reduce sums `world` partial residuals in another order — the more ranks, the more often the arg-max of
    # two almost equal probabilities flips): the sharded run's token must carry, in the unsharded distribution, the maximum minus at
    # most twice the largest difference between the two distributions at that step.  Inputs are teacher-forced: no drift.
    near_tie = 0
    for i, (ta, tb) in enumerate(zip(outs[0][0], outs[1][0])):
        if ta != tb:
            a, b = outs[0][1][i].view(-1), outs[1][1][i].view(-1)
            gap = float(a.max() - a[tb])
            if gap <= 2.0 * float((a - b).abs().max()):
                near_tie += 1
            else:
                ok = False
    # layer 0 sees identical inputs on both runs: its evictions must agree exactly; deeper layers see a residual stream
    # rounded differently by the all-reduce, and heavy-hitter scores of random data sit in near-ties
    # (long caches: the unsharded step and a rank's step split the cache differently — 32 x 8 waves against 55 x 4 at C5 — so the last
    #  bit of (M, L), hence of a bf16 probability, hence a near-tie eviction may differ: at most one slot per 2048 and rank, counted)
    ok = ok and differ[0] <= args.cache // 2048 and same_tokens + near_tie == len(outs[0][0]) and near_tie <= max(1, world // 2)
    if rank == 0:
        print(f"backend {dist.get_backend()} world {world} graph {bool(args.graph)} oneshot {bool(args.oneshot)}: tokens equal: {same_tokens}/{len(outs[0][0])} (+ {near_tie} arg-max near-ties); "
              f"TP{world} CHECK {'OK' if ok else 'FAIL'}", flush=True)
    from cold_compress_amd.attention_utils import single_launch_status

    st = int(single_launch_status(dev))
    if st:
        print(f"rank {rank}: a single-launch step reported a hand-off timeout (status word {st}): the comparison above is void", flush=True)
        ok = False
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
