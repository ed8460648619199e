"""Time the blockwise-FP8 kernels on one GPU (block size [128, 128], bf16) and write profiles/blockwise_fp8.md.

    python scripts/bench_blockwise_fp8.py [--out profiles/blockwise_fp8.md] [--iters 200]

Steps, each in a child process of its own under `timeout` (one process on the GPU at a time; a step that fails or hangs ends the run):
  dense:N:K  at M = 1, 8, 512, in the same process: `fused` launch_fp8_matmul_bf16; `yardstick` dequantize_w() followed by the library bf16 matmul (what a user
             must do without the fused route, and the reference's fallback, blockwise_fp8/mod.rs:282-289); `ceiling` the library matmul alone on the
             pre-dequantized bf16 weight
  moe        launch_fp8_indexed_moe_gemm_bf16, E = 32, topk = 4, N = K = 2880, T = 1 and T = 64; its yardstick is the dequantize_w() of the expert stack alone,
             which the fallback pays before it multiplies anything
HIP events around `iters` back-to-back launches after a warm-up of the same length (a tenth of that for the yardstick), median of 5 rounds; weights rotate over
enough copies to exceed the 256 MiB Infinity Cache for M <= 8 (a decode step streams its weights from HBM).  bytes = weight bytes + scales read once.
The one condition: at M = 1 and M = 8 `fused` is faster than `yardstick` at every shape.  M = 512 is reported, not gated.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]
MS = [1, 8, 512]
BS = (128, 128)
MOE = dict(e=32, topk=4, n=2880, k=2880, tokens=(1, 64))
HBM_BYTES_PER_US = 8e6  # 8 TB/s


def _time(fn_of_i, iters, copies):
    import torch
    for i in range(iters):
        fn_of_i(i % copies)
    torch.cuda.synchronize()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn_of_i(i % copies)
        b.record()
        torch.cuda.synchronize()
        rounds.append(a.elapsed_time(b) * 1e3 / iters)
    return sorted(rounds)[2]


def _copies(nbytes, m):
    return max(1, min(64, (320 << 20) // nbytes + 1)) if m <= 8 else 1


def step(name, iters):
    import torch
    import mistralrs_amd  # noqa: F401
    from mistralrs_amd import blockwise_fp8 as bf8
    dev, out = "cuda:0", []
    g = torch.Generator(device="cpu").manual_seed(0)

    def layer(*shape):
        w = torch.randint(0, 0x7F, shape, dtype=torch.uint8, generator=g) | (torch.randint(0, 2, shape, dtype=torch.uint8, generator=g) << 7)  # no NaN bytes
        s = torch.rand(*shape[:-2], -(-shape[-2] // BS[0]), -(-shape[-1] // BS[1]), generator=g) * 0.01 + 0.001
        return bf8.BlockwiseFP8Linear(w.to(dev), s.to(dev), None, torch.bfloat16, BS)

    if name.startswith("dense:"):
        n, k = (int(v) for v in name.split(":")[1:])
        nbytes = n * k + 4 * (-(-n // BS[0])) * (-(-k // BS[1]))
        for m in MS:
            c = _copies(nbytes, m)
            ls = [layer(n, k) for _ in range(c)]
            x = (torch.rand(m, k, generator=g) * 4 - 2).to(torch.bfloat16).to(dev)
            us = _time(lambda i: ls[i].forward(x), iters, c)
            out.append(dict(step="fused", n=n, k=k, m=m, us=us, bytes=nbytes, route=bf8.last_route(), copies=c))
            us = _time(lambda i: x @ ls[i].dequantize_w().t(), max(10, iters // 10), c)
            out.append(dict(step="yardstick", n=n, k=k, m=m, us=us, bytes=nbytes, route=0, copies=c))
            dense = [l.dequantize_w() for l in ls]
            us = _time(lambda i: x @ dense[i].t(), iters, c)
            out.append(dict(step="ceiling", n=n, k=k, m=m, us=us, bytes=2 * n * k, route=0, copies=c))
            del dense, ls
    elif name == "moe":
        e, topk, n, k = MOE["e"], MOE["topk"], MOE["n"], MOE["k"]
        experts = layer(e, n, k)
        per_expert = n * k + 4 * (-(-n // BS[0])) * (-(-k // BS[1]))
        for t in MOE["tokens"]:
            x = (torch.rand(t, k, generator=g) * 4 - 2).to(torch.bfloat16).to(dev)
            idxs = [torch.stack([torch.randperm(e, generator=g)[:topk] for _ in range(t)]).to(torch.int32).to(dev) for _ in range(8)]
            touched = sum(len(set(i.reshape(-1).tolist())) for i in idxs) / len(idxs)
            us = _time(lambda i: experts.gather_forward(x, idxs[i]), iters, 8)
            out.append(dict(step="moe", n=n, k=k, m=t, us=us, bytes=int(touched * per_expert), route=bf8.last_route(), copies=8))
        us = _time(lambda i: experts.dequantize_w(), 10, 1)
        out.append(dict(step="moe_yardstick", n=n, k=k, m=0, us=us, bytes=e * per_expert, route=0, copies=1))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blockwise_fp8.md"))
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.iters)
    rows = []
    for name in [f"dense:{n}:{k}" for n, k in SHAPES] + ["moe"]:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(a.iters)], capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            sys.exit(f"step {name} failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
        rows += json.loads(line[7:])
        print(f"step {name} done", flush=True)
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = os.environ.get("MRS_COMMIT", "unknown (no git metadata next to the run)")
    label = {"fused": "launch_fp8_matmul_bf16", "yardstick": "dequantize_w() + library bf16 matmul", "ceiling": "library bf16 matmul, weight already dense",
             "moe": "launch_fp8_indexed_moe_gemm_bf16 (E 32, topk 4; M column = tokens)", "moe_yardstick": "dequantize_w() of the 32-expert stack alone"}
    key = lambda r: (r["n"], r["k"], r["m"])
    yard = {key(r): r["us"] for r in rows if r["step"] == "yardstick"}
    gated = [(key(r), r["us"], yard[key(r)]) for r in rows if r["step"] == "fused" and r["m"] <= 8]
    lost = [g for g in gated if not g[1] < g[2]]
    md = ["# Blockwise FP8 kernels on one MI355X", "",
          f"Written by `scripts/bench_blockwise_fp8.py` (block size [128, 128], bf16; HIP events, {a.iters} launches per round after an equal warm-up, a tenth of that for",
          "the yardstick, median of 5 rounds, weights rotated through > 256 MiB for M <= 8).  The three rows of one (N, K, M) come from one process.",
          f"Parent commit of the measured tree: `{commit}`.  bytes = weight bytes + scales read once (the ceiling row: the dense bf16 weight); the fraction is of 8 TB/s",
          "and is given for M <= 8 only.", "",
          "| what | N | K | M | route | us | bytes / us | of 8 TB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        rate = r["bytes"] / r["us"]
        frac = f"{rate / HBM_BYTES_PER_US:.1%}" if r["m"] <= 8 and r["step"] in ("fused", "moe", "ceiling") else ""
        md.append(f"| {label[r['step']]} | {r['n']} | {r['k']} | {r['m'] or ''} | {r['route'] or ''} | {r['us']:.1f} | {rate:,.0f} | {frac} |")
    md += ["", "Condition (fused faster than the yardstick at M = 1 and M = 8, every shape): "
           + ("**met** at all %d points; the smallest margin is %.1fx." % (len(gated), min(y / f for _, f, y in gated)) if not lost else
              "**NOT met** at " + ", ".join(f"(N {k[0]}, K {k[1]}, M {k[2]}): fused {f:.1f} us, yardstick {y:.1f} us" for k, f, y in lost) + "."),
           "M = 512 is reported, not gated.  Untuned: see DESIGN 4.15."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))
    print(json.dumps(dict(rows=rows, commit=commit)))


if __name__ == "__main__":
    main()
