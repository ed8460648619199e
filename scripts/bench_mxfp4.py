"""Time the MXFP4 kernels on one GPU (GPT-OSS shapes) and write profiles/mxfp4.md.

    python scripts/bench_mxfp4.py [--out profiles/mxfp4.md] [--iters 200]

Steps, each in a child process of its own under `timeout` (one process on the GPU at a time; a step that fails or hangs ends the run):
  dense     launch_mxfp4_matmul_bf16 at (N, K) = (5760, 2880), (2880, 2880), M in 1, 4, 8, 64, 512
  moe       the indexed MoE launch, E = 32, topk = 4, one token, same (N, K)
  dequant   dequantize_w() followed by a torch bf16 matmul on the dense shapes
  q4k       the Q4_K MMVQ launch at the nearest legal (N, K) (K % 256 == 0): the in-repo yardstick for a 4-bit streaming GEMV
HIP events around `iters` back-to-back launches after a warm-up of the same length, median of 5 rounds; weights rotate over enough copies to exceed the 256 MiB
Infinity Cache for M <= 8 (a decode step streams its weights from HBM).  bytes = packed weights + scales streamed once.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(5760, 2880), (2880, 2880)]
MS = [1, 4, 8, 64, 512]
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
    from mistralrs_amd import mxfp4
    dev, out = "cuda:0", []
    g = torch.Generator(device="cpu").manual_seed(0)

    def weights(*lead, k):
        return (torch.randint(0, 256, (*lead, k // 2), dtype=torch.uint8, generator=g).to(dev),
                torch.randint(107, 138, (*lead, k // 32), dtype=torch.uint8, generator=g).to(dev))

    if name in ("dense", "dequant"):
        for n, k in SHAPES:
            nbytes = n * (k // 2 + k // 32)
            for m in MS:
                c = _copies(nbytes, m)
                ws = [weights(n, k=k) for _ in range(c)]
                x = (torch.rand(m, k, generator=g) * 4 - 2).to(torch.bfloat16).to(dev)
                if name == "dense":
                    us = _time(lambda i: mxfp4.matmul(x, ws[i][0], ws[i][1]), iters, c)
                    route = mxfp4.last_route()
                else:
                    layers = [mxfp4.MXFP4Layer.from_parts(b, s) for b, s in ws]
                    us = _time(lambda i: x @ layers[i].dequantize_w().t(), max(10, iters // 10), c)
                    route = 0
                out.append(dict(step=name, n=n, k=k, m=m, us=us, bytes=nbytes, route=route, copies=c))
    elif name == "moe":
        e, topk = 32, 4
        for n, k in SHAPES:
            b, s = weights(e, n, k=k)
            x = (torch.rand(1, k, generator=g) * 4 - 2).to(torch.bfloat16).to(dev)
            idxs = [torch.randperm(e, generator=g)[:topk].reshape(1, topk).to(torch.int32).to(dev) for _ in range(8)]  # 8 x 4 distinct experts: rotates over the stack
            us = _time(lambda i: mxfp4.indexed_moe_gemm(x, b, s, None, idxs[i], entry="indexed"), iters, 8)
            out.append(dict(step=name, n=n, k=k, m=1, us=us, bytes=topk * n * (k // 2 + k // 32), route=mxfp4.last_route(), copies=8))
    elif name == "q4k":
        from mistralrs_amd.gguf import GgmlDType, QTensor, fast_mmvq
        import numpy as np
        rng = np.random.default_rng(0)
        for n, k0 in SHAPES:
            k = (k0 // 256) * 256
            nbytes = n * k // 256 * 144
            for m in (1, 4, 8):
                c = _copies(nbytes, m)
                packed = rng.integers(0, 256, (n, k // 256, 144), dtype=np.uint8)
                packed[:, :, 1] &= 0x3B  # keep the two f16 block scales finite
                packed[:, :, 3] &= 0x3B
                ws = [QTensor.from_numpy(GgmlDType.Q4K, (n, k), packed.reshape(n, -1), dev) for _ in range(c)]
                x = (torch.rand(m, k, generator=g) * 4 - 2).to(dev)
                us = _time(lambda i: fast_mmvq.plain(ws[i], x), iters, c)
                out.append(dict(step=name, n=n, k=k, m=m, us=us, bytes=nbytes, route=0, copies=c))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4.md"))
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.iters)
    rows = []
    for name in ("dense", "moe", "dequant", "q4k"):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(a.iters)], capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            sys.exit(f"step {name} failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
        rows += json.loads(line[7:])
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = os.environ.get("MRS_COMMIT", "unknown (no git metadata next to the run)")
    label = {"dense": "launch_mxfp4_matmul_bf16", "moe": "launch_mxfp4_indexed_moe_gemm_bf16 (E 32, topk 4)", "dequant": "dequantize_w() + torch bf16 matmul",
             "q4k": "Q4_K MMVQ (launch_mmvq_gguf_q4_k_f32_plain)"}
    md = ["# MXFP4 kernels on one MI355X", "",
          f"Written by `scripts/bench_mxfp4.py` (HIP events, {a.iters} launches per round after an equal warm-up, median of 5 rounds, weights rotated through > 256 MiB for M <= 8).",
          f"Parent commit of the measured tree: `{commit}`.  bytes = packed weights + scales read once; the fraction is of 8 TB/s and is given for M <= 8 only.", "",
          "| what | N | K | M | route | us | bytes / us | of 8 TB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        rate = r["bytes"] / r["us"]
        frac = f"{rate / HBM_BYTES_PER_US:.1%}" if r["m"] <= 8 and r["step"] != "dequant" else ""
        md.append(f"| {label[r['step']]} | {r['n']} | {r['k']} | {r['m']} | {r['route'] or ''} | {r['us']:.1f} | {rate:,.0f} | {frac} |")
    md += ["", "Untuned: see DESIGN 4.14."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))
    print(json.dumps(dict(rows=rows, commit=commit)))


if __name__ == "__main__":
    main()
