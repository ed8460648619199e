"""Time the per-tensor FP8 W8A8 forward on one GPU (bf16 activations) and write profiles/fp8.md.

    python scripts/bench_fp8.py [--out profiles/fp8.md] [--iters 100]

One child process per (N, K) shape under `timeout` (one process on the GPU at a time; a step that fails or hangs ends the run).  In that process, for each M, four
sides are timed in turn, round after round (so that drift hits all of them alike):
  w8a8       FP8Linear.forward: the dynamic quantizer's launches plus launch_fp8_pertensor_matmul_bf16
  dequant    dequantize_w() followed by the library bf16 matmul: yardstick (a)
  blockwise  launch_fp8_matmul_bf16 on the same bytes with a 1 x 1 scale grid (PerTensorFP8Linear, act_quant "none"), how the parent commit serves this weight:
             yardstick (b)
  library    the library bf16 matmul alone on the pre-dequantized weight
  w8a8 graph / blockwise graph   the same two forwards over all weight copies captured once into a graph and replayed: the device side alone, without the host's
             work per call (allocations, argument checks, the ctypes calls).  A replay is checked against the eager result before it is timed.
HIP events around `iters` back-to-back launches (a tenth for `dequant`) after a warm-up round; 5 rounds, the median is reported and max - min is the run-to-run
spread.  Weights rotate over enough copies to exceed the 256 MiB Infinity Cache for M <= 16 (a decode step streams its weights from HBM).
The one condition: at M = 1 and M = 8, `w8a8` is not slower than `dequant` or `blockwise` by more than the larger of the two spreads involved.  It is evaluated on
the eager calls, and again on the graph pair, which says whether a miss is the kernels' or the host's.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_blockwise_fp8 import HBM_BYTES_PER_US, SHAPES  # noqa: E402

MS = [1, 8, 16, 64, 512]
SIDES = ["w8a8", "dequant", "blockwise", "library", "w8a8_graph", "blockwise_graph"]
ROUNDS = 5


def step(n, k, iters):
    import torch
    import mistralrs_amd  # noqa: F401
    from mistralrs_amd import fp8
    dev, out = "cuda:0", []
    g = torch.Generator(device="cpu").manual_seed(0)
    ws = []
    for _ in range(max(1, min(64, (320 << 20) // (n * k) + 1))):
        w = torch.randint(0, 0x7F, (n, k), dtype=torch.uint8, generator=g) | (torch.randint(0, 2, (n, k), dtype=torch.uint8, generator=g) << 7)  # no NaN bytes
        ws.append(w.to(dev))
    scale = torch.tensor(0.004, device=dev)
    w8 = [fp8.FP8Linear.from_parts(w, None, scale, scale, scale) for w in ws]
    bw = [fp8.PerTensorFP8Linear(w, scale) for w in ws]
    for m in MS:
        copies = len(ws) if m <= 16 else 1
        dense = [l.dequantize_w() for l in bw] if m > 16 else None  # bf16; at M <= 16 the copies of it would not fit next to the rest
        x = (torch.rand(m, k, generator=g) * 4 - 2).to(torch.bfloat16).to(dev)
        fns = {"w8a8": lambda i: w8[i].forward(x), "dequant": lambda i: x @ bw[i].dequantize_w().t(), "blockwise": lambda i: bw[i].forward(x)}
        if dense is not None:
            fns["library"] = lambda i: x @ dense[i].t()
        graphs = {}
        for side in ("w8a8", "blockwise"):
            want = fns[side](0).clone()  # also the first call of this shape: one-time kernel attributes are set outside the capture
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                outs = [fns[side](i) for i in range(copies)]
            for _ in range(3):
                gr.replay()
                torch.cuda.synchronize()
                assert torch.equal(outs[0], want), f"{side}: a graph replay differs from the eager result"
            graphs[side + "_graph"] = (gr, outs)
        times, routes = {s: [] for s in list(fns) + list(graphs)}, {}
        for rnd in range(ROUNDS + 1):  # round 0 is the warm-up
            for side in times:
                fn = fns.get(side)
                it = max(5, iters // 10) if side == "dequant" else iters if fn else max(1, iters // copies) * copies
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if fn is None:
                    for _ in range(it // copies):
                        graphs[side][0].replay()
                else:
                    for i in range(it):
                        fn(i % copies)
                b.record()
                torch.cuda.synchronize()
                if rnd:
                    times[side].append(a.elapsed_time(b) * 1e3 / it)
                if side == "w8a8":
                    routes[side] = fp8.fp8_pertensor_last_route()
        for side, ts in times.items():
            ts = sorted(ts)
            out.append(dict(side=side, n=n, k=k, m=m, us=ts[len(ts) // 2], spread=ts[-1] - ts[0], route=routes.get(side, 0), copies=copies))
        del dense, graphs
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8.md"))
    ap.add_argument("--errors", default=None, help="a text file of `worst error / bound` lines (the GPU test's output) to append")
    a = ap.parse_args()
    if a.step:
        return step(*(int(v) for v in a.step.split(":")), a.iters)
    rows = []
    for n, k in SHAPES:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--step", f"{n}:{k}", "--iters", str(a.iters)], capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            sys.exit(f"step {n}:{k} failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
        rows += json.loads(line[7:])
        print(f"step {n}:{k} done", flush=True)
    at = {(r["n"], r["k"], r["m"], r["side"]): r for r in rows}
    md = ["# Per-tensor FP8 (W8A8) on one MI355X", "",
          f"Written by `scripts/bench_fp8.py` (bf16 activations; HIP events, {a.iters} launches per round, a tenth for `dequant`; a warm-up round, then {ROUNDS} rounds with",
          "the sides taken in turn; median, and max - min as the spread; weights rotated through > 256 MiB for M <= 16).  All sides of one (N, K) come from one process.",
          "`w8a8` = FP8Linear.forward, the dynamic quantizer's launches included; `dequant` = dequantize_w() + library bf16 matmul; `blockwise` = the blockwise route",
          "on the same bytes with a 1 x 1 scale grid; `library` = the library bf16 matmul on a pre-dequantized weight; `graph` = the forward captured once and replayed (the device side alone).  The share of",
          "8 TB/s counts the weight bytes (N K).", "",
          "| N | K | M | route | w8a8 us (spread) | dequant us (spread) | blockwise us (spread) | library us | w8a8 graph us (spread) | blockwise graph us (spread) | w8a8 graph of 8 TB/s | graph M / M=1 |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    lost, lost_dev = [], []
    for n, k in SHAPES:
        for m in MS:
            w, d, b, lib, wg, bg = (at.get((n, k, m, s)) for s in SIDES)
            md.append(f"| {n} | {k} | {m} | {w['route']} | {w['us']:.1f} ({w['spread']:.1f}) | {d['us']:.1f} ({d['spread']:.1f}) | {b['us']:.1f} ({b['spread']:.1f}) | "
                      f"{'%.1f' % lib['us'] if lib else ''} | {wg['us']:.1f} ({wg['spread']:.1f}) | {bg['us']:.1f} ({bg['spread']:.1f}) | "
                      f"{n * k / wg['us'] / HBM_BYTES_PER_US:.1%} | {wg['us'] / at[(n, k, 1, 'w8a8_graph')]['us']:.2f} |")
            if m in (1, 8):
                lost += [f"(N {n}, K {k}, M {m}): w8a8 {w['us']:.1f} us, {y['side']} {y['us']:.1f} us, spread {max(w['spread'], y['spread']):.1f} us"
                         for y in (d, b) if w["us"] > y["us"] + max(w["spread"], y["spread"])]
                if wg["us"] > bg["us"] + max(wg["spread"], bg["spread"]):
                    lost_dev.append(f"(N {n}, K {k}, M {m}): {wg['us']:.1f} us against {bg['us']:.1f} us")
    md += ["", "Condition (w8a8 not slower than `dequant` or `blockwise` by more than the spread, at M = 1 and M = 8, every shape): "
           + ("**met** at all points." if not lost else "**NOT met** at " + "; ".join(lost) + "."),
           "The same on the device side alone (w8a8 graph against blockwise graph): " + ("**met** at all points." if not lost_dev else "**NOT met** at " + "; ".join(lost_dev) + "."),
           "M = 16, 64 and 512 are reported, not gated.  Untuned: see DESIGN 4.18."]
    if a.errors and os.path.exists(a.errors):
        md += ["", "## Worst error / bound of the random cases (tests/test_zz_fp8_gpu.py)", "", "```"] + [ln.rstrip() for ln in open(a.errors) if "worst error / bound" in ln] + ["```"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))
    print(json.dumps(dict(rows=rows)))


if __name__ == "__main__":
    main()
