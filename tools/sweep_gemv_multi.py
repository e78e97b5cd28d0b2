#!/usr/bin/env python
"""Launch geometries of cc_gemv_fused_multi at T = 2, 3, 4 over the four dense decode shapes of the 8B model (bf16): wqkv
[6144, 4096] with its norm prologue and RoPE epilogue, wo [4096, 4096], the w1/w3 pair [14336, 4096] x 2 with its norm prologue,
w2 [4096, 14336].  The geometry comes from the CC_GEMV_CFG="RB,CU,max workgroups" hook, which the library reads once per process:
the driver starts one worker process per geometry, one after the other, and a worker without the hook (pick_multi_cfg's own choice)
first and last.  A worker times every (shape, T) it can launch `--runs` times with HIP events over `--mats` distinct weight matrices
per shape in turn (more bytes than the 256 MiB Infinity Cache, so every launch streams its weights from HBM); a geometry that is not
built for a shape is recorded as null.  Prints one JSON object; profiles/gemv_multi_geometry.md is written from it.

    python tools/sweep_gemv_multi.py [--runs 5] [--reps 6] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (RB, CU) of the table in DESIGN §2.11 that are built without scratch for bf16: XS = 2 (K = 4096) and XS = 8 (K = 14336)
GEOMETRIES = [(2, 2), (4, 2), (8, 2), (2, 4), (4, 4), (2, 8), (4, 8)]
CAPS = [512, 1024, 2048]
DIM, INTER, HQ, H, D = 4096, 14336, 32, 8, 128


def worker(args):
    import torch

    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    bf = torch.bfloat16

    def mats(n, k, count):
        return [torch.randn(n, k, device=dev, generator=g, dtype=torch.float32).mul_(0.02).to(bf) for _ in range(count)]

    x4 = torch.randn(4, DIM, device=dev, generator=g).to(bf)
    d4 = torch.randn(4, DIM, device=dev, generator=g).to(bf)
    g4 = torch.randn(4, INTER, device=dev, generator=g).to(bf)
    nw = torch.ones(DIM, device=dev, dtype=bf)
    fr4 = torch.randn(4, D // 2, 2, device=dev, generator=g).to(bf)
    h4 = torch.empty_like(x4)
    M = args.mats
    wqkv, wo, w2 = mats((HQ + 2 * H) * D, DIM, M), mats(DIM, DIM, M), mats(DIM, INTER, max(2, M // 2))
    w1, w3 = mats(INTER, DIM, max(2, M // 2)), mats(INTER, DIM, max(2, M // 2))
    shapes = {
        "wqkv": (len(wqkv), lambda i, T: glue.gemv_fused_multi(wqkv[i], x4[:T], delta=d4[:T], norm_weight=nw, h_out=h4[:T], freqs=fr4[:T],
                                                               rope_rows=(HQ + H) * D, head_dim=D)),
        "wo": (len(wo), lambda i, T: glue.gemv_fused_multi(wo[i], x4[:T])),
        "w1/w3": (len(w1), lambda i, T: glue.gemv_fused_multi(w1[i], x4[:T], w3=w3[i], delta=d4[:T], norm_weight=nw, h_out=h4[:T])),
        "w2": (len(w2), lambda i, T: glue.gemv_fused_multi(w2[i], g4[:T])),
    }
    out = {}
    for name, (n, fn) in shapes.items():
        for T in (2, 3, 4):
            key = f"{name} T={T}"
            try:
                fn(0, T)
            except _abi.ColdCompressError:  # this geometry is not built for this shape
                out[key] = None
                continue
            for i in range(n):
                fn(i, T)
            us = []
            for _ in range(args.runs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    for i in range(n):
                        fn(i, T)
                b.record()
                b.synchronize()
                us.append(a.elapsed_time(b) * 1e3 / (args.reps * n))
            out[key] = {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--mats", type=int, default=8, help="distinct weight matrices per shape (half as many for the 14336-wide ones)")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cfgs = [None] + [f"{rb},{cu},{cap}" for rb, cu in GEOMETRIES for cap in CAPS] + [None]
    results = []
    for cfg in cfgs:
        env = dict(os.environ)
        env.pop("CC_GEMV_CFG", None)
        if cfg is not None:
            env["CC_GEMV_CFG"] = cfg
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--runs", str(args.runs), "--reps", str(args.reps), "--mats", str(args.mats)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
        if p.returncode != 0:  # a worker that died ends the sweep: nothing more is started on the device
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"worker for CC_GEMV_CFG={cfg} ended with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        results.append({"cfg": cfg or "default", "us": json.loads(line[7:])})
        print(f"{cfg or 'default'}: done", file=sys.stderr, flush=True)
        if args.out:  # (after every worker: a partial sweep is kept)
            with open(args.out, "w") as f:
                f.write(json.dumps({"runs": args.runs, "reps": args.reps, "mats": args.mats, "results": results}, indent=1) + "\n")
    print(json.dumps({"runs": args.runs, "reps": args.reps, "mats": args.mats, "results": results}, indent=1))


if __name__ == "__main__":
    main()
