"""Time the bitsandbytes kernels on one GPU and write profiles/bnb.md.

    python scripts/bench_bnb.py [--out profiles/bnb.md] [--iters 100]

NF4, blocksize 64, double-quantized absmax (nested blocksize 256), bf16; (N, K) = (4096, 4096), (14336, 4096), (4096, 14336), (28672, 4096); M in 1, 8, 64, 512.
Per shape and M, in ONE process and alternating round by round on the same data:
  fused    BnbLinear.forward (route 1 for M <= 8, route 2 above)
  deq_mm   dequantize_w() + the library matmul in the same forward (what the reference does per call)
  dense    the library matmul on an already dense bf16 weight
and per shape the dequantize kernel alone.  The measuring process runs under a time limit; if it fails nothing more is started on the GPU.
Timing: HIP events around `iters` launches after an equal warm-up (a tenth for M > 8, deq_mm and dequantize), 5 rounds per side, the sides interleaved; the
median is reported and the spread is (max - min) / median over a side's rounds.  For M <= 8 the weights rotate through > 256 MiB so that no launch finds its
bytes in the last-level cache.  packed bytes = weight + u8 absmax + nested tensors, read once.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336), (28672, 4096)]
MS = [1, 8, 64, 512]
BLOCK, NESTED = 64, 256
HBM_BYTES_PER_US = 8e6  # 8 TB/s


def _round(fn_of_i, iters, copies):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn_of_i(i % copies)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _time_sides(sides, copies):
    """sides: {name: (fn_of_i, iters)} -> {name: (median us, spread)}; warm-up, then 5 rounds with the sides alternating"""
    for fn, iters in sides.values():
        _round(fn, iters, copies)
    rounds = {name: [] for name in sides}
    for _ in range(5):
        for name, (fn, iters) in sides.items():
            rounds[name].append(_round(fn, iters, copies))
    return {name: (sorted(r)[2], (max(r) - min(r)) / sorted(r)[2]) for name, r in rounds.items()}


def nbytes_of(n, k):
    blocks = n * k // BLOCK
    return n * k // 2 + blocks + 4 * (-(-blocks // NESTED)) + 1024


def run(iters):
    import torch
    import mistralrs_amd  # noqa: F401
    from mistralrs_amd import bnb
    dev, out = "cuda:0", []
    g = torch.Generator(device="cpu").manual_seed(0)

    def layer(n, k):
        blocks = n * k // BLOCK
        return bnb.BnbLinear.from_parts(torch.randint(0, 256, (n * k // 2,), dtype=torch.uint8, generator=g).to(dev),
                                        torch.randint(0, 256, (blocks,), dtype=torch.uint8, generator=g).to(dev), "nf4", BLOCK, (n, k), torch.bfloat16, None,
                                        (torch.rand(-(-blocks // NESTED), generator=g) * 0.01 + 0.005).to(dev), torch.linspace(-1, 1, 256).to(dev), NESTED, 0.02)

    for n, k in SHAPES:
        nbytes = nbytes_of(n, k)
        c = max(1, min(64, (320 << 20) // nbytes + 1))
        layers = [layer(n, k) for _ in range(c)]
        dense = layers[0].dequantize_w()
        us, spread = _time_sides({"dequantize": (lambda i: layers[i].dequantize_w(), max(10, iters // 10))}, c)["dequantize"]
        out.append(dict(step="dequantize", n=n, k=k, m=0, us=us, spread=spread, bytes=nbytes + 2 * n * k, route=0))
        for m in MS:
            cm = c if m <= 8 else 1
            it = iters if m <= 8 else max(10, iters // 10)
            x = (torch.rand(m, k, generator=g) * 4 - 2).to(torch.bfloat16).to(dev)
            res = _time_sides({"fused": (lambda i: layers[i].forward(x), it),
                               "deq_mm": (lambda i: torch.nn.functional.linear(x, layers[i].dequantize_w()), max(10, iters // 10)),
                               "dense": (lambda i: torch.nn.functional.linear(x, dense), it)}, cm)
            route = 1 if m <= 8 else 2
            layers[0].forward(x)
            assert bnb.last_route() == route
            for step, (us, spread) in res.items():
                out.append(dict(step=step, n=n, k=k, m=m, us=us, spread=spread, bytes=nbytes, route=route if step == "fused" else 0))
        del layers, dense
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bnb.md"))
    a = ap.parse_args()
    if a.run:
        return run(a.iters)
    r = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--run", "--iters", str(a.iters)], capture_output=True, text=True)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        sys.exit(f"the measuring process failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
    rows = json.loads(line[7:])
    label = {"fused": "BnbLinear.forward", "deq_mm": "dequantize_w + library matmul", "dense": "library matmul, dense bf16 weight", "dequantize": "dequantize_w alone"}
    md = ["# bitsandbytes NF4 kernels on one MI355X", "",
          f"Written by `python scripts/bench_bnb.py --iters {a.iters}` (one process; HIP events, {a.iters} launches per round after an equal warm-up, a tenth of that "
          "for M > 8, for the dequantize lines and for dequantize_w + library matmul; 5 rounds per side with the sides alternating, median; weights rotated through "
          "> 256 MiB for M <= 8).",
          "NF4, blocksize 64, double-quantized absmax (nested blocksize 256), bf16.  spread = (max - min) / median over a line's 5 rounds.  packed bytes = weight + "
          "u8 absmax + nested tensors read once (the dequantize line adds the bf16 bytes written); the fraction is of 8 TB/s.", "",
          "| what | N | K | M | route | us | spread | bytes / us | of 8 TB/s |", "|---|---|---|---|---|---|---|---|---|"]
    for r_ in rows:
        rate = r_["bytes"] / r_["us"]
        frac = f"{rate / HBM_BYTES_PER_US:.1%}" if (r_["step"] == "fused" and r_["m"] <= 8) or r_["step"] == "dequantize" else ""
        md.append(f"| {label[r_['step']]} | {r_['n']} | {r_['k']} | {r_['m'] or ''} | {r_['route'] or ''} | {r_['us']:.1f} | {r_['spread']:.1%} | {rate:,.0f} | {frac} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))
    print(json.dumps(dict(rows=rows)))


if __name__ == "__main__":
    main()
