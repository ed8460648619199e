"""Time the AFQ kernels on one GPU and write profiles/afq.md.

    python scripts/bench_afq.py [--out profiles/afq.md] [--iters 200]

Steps (each in a process of its own, under a time limit; a failed step ends the run):
  dense     mrs_afq_matmul, bf16, AFQ4 and AFQ8 at group 64, (N, K) = (4096, 4096), (14336, 4096), M in 1, 8, 512
  dequant   the same problems as dequantize_w() + the library matmul (the baseline of the same run)
  moe       one token, E 32, topk 4: mrs_afq_indexed_moe_gemm
  q4k       the Q4_K MMVQ launches at M = 1 on the same shapes
Timing: HIP events around `iters` launches after an equal warm-up, median of 5 rounds; for M <= 8 the weights rotate through > 256 MiB so that no
launch finds its bytes in the 256 MiB last-level cache.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4096, 4096), (14336, 4096)]
MS = [1, 8, 512]
BITS, GROUP = [4, 8], 64
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
    from mistralrs_amd import afq
    dev, out = "cuda:0", []
    g = torch.Generator(device="cpu").manual_seed(0)

    def weights(*lead, k, bits):
        w_q = torch.randint(-2 ** 31, 2 ** 31 - 1, (*lead, k * bits // 32), dtype=torch.int32, generator=g).to(dev).view(torch.uint32)
        s = (torch.rand(*lead, k // GROUP, generator=g) * 0.01 + 0.001).to(torch.bfloat16).to(dev)
        return w_q, s, (-s.float() * (1 << (bits - 1))).to(torch.bfloat16)

    def nbytes_of(n, k, bits):
        return n * (k * bits // 8 + 2 * 2 * (k // GROUP))

    if name in ("dense", "dequant"):
        for bits in BITS:
            for n, k in SHAPES:
                nbytes = nbytes_of(n, k, bits)
                for m in MS:
                    c = _copies(nbytes, m)
                    ws = [weights(n, k=k, bits=bits) for _ in range(c)]
                    x = (torch.rand(m, k, generator=g) * 4 - 2).to(torch.bfloat16).to(dev)
                    if name == "dense":
                        us = _time(lambda i: afq.matmul(x, *ws[i], bits, GROUP), iters if m <= 8 else max(10, iters // 10), c)
                        route = afq.last_route()
                    else:
                        layers = [afq.AfqLayer.from_parts(*w, None, bits, GROUP) for w in ws]
                        us = _time(lambda i: x @ layers[i].dequantize_w().t(), max(10, iters // 10), c)
                        route = 0
                    out.append(dict(step=name, bits=bits, n=n, k=k, m=m, us=us, bytes=nbytes, route=route, copies=c))
    elif name == "moe":
        e, topk = 32, 4
        for bits in BITS:
            for n, k in SHAPES[:1]:
                w_q, s, b = weights(e, n, k=k, bits=bits)
                x = (torch.rand(1, k, generator=g) * 4 - 2).to(torch.bfloat16).to(dev)
                idxs = [torch.randperm(e, generator=g)[:topk].reshape(1, topk).to(torch.int32).to(dev) for _ in range(8)]  # 8 x 4 distinct experts: rotates over the stack
                us = _time(lambda i: afq.indexed_moe_gemm(x, w_q, s, b, bits, GROUP, idxs[i]), iters, 8)
                out.append(dict(step=name, bits=bits, n=n, k=k, m=1, us=us, bytes=topk * nbytes_of(n, k, bits), route=afq.last_route(), copies=8))
    elif name == "q4k":
        from mistralrs_amd.gguf import GgmlDType, QTensor, fast_mmvq
        import numpy as np
        rng = np.random.default_rng(0)
        for n, k in SHAPES:
            nbytes = n * k // 256 * 144
            c = _copies(nbytes, 1)
            packed = rng.integers(0, 256, (n, k // 256, 144), dtype=np.uint8)
            packed[:, :, 1] &= 0x3B  # keep the two f16 block scales finite
            packed[:, :, 3] &= 0x3B
            ws = [QTensor.from_numpy(GgmlDType.Q4K, (n, k), packed.reshape(n, -1), dev) for _ in range(c)]
            x = (torch.rand(1, k, generator=g) * 4 - 2).to(dev)
            us = _time(lambda i: fast_mmvq.plain(ws[i], x), iters, c)
            out.append(dict(step=name, bits=4, n=n, k=k, m=1, us=us, bytes=nbytes, route=0, copies=c))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afq.md"))
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.iters)
    rows = []
    for name in ("dense", "moe", "dequant", "q4k"):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(a.iters)], capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            sys.exit(f"step {name} failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
        rows += json.loads(line[7:])
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = os.environ.get("MRS_COMMIT", "unknown (no git metadata next to the run)")
    label = {"dense": "mrs_afq_matmul bf16", "moe": "mrs_afq_indexed_moe_gemm bf16 (E 32, topk 4, one token)", "dequant": "dequantize_w() + torch bf16 matmul",
             "q4k": "Q4_K MMVQ (launch_mmvq_gguf_q4_k_f32_plain)"}
    md = ["# AFQ kernels on one MI355X", "",
          f"Written by `scripts/bench_afq.py` (HIP events, {a.iters} launches per round after an equal warm-up, median of 5 rounds, weights rotated through > 256 MiB for M <= 8).",
          f"Parent commit of the measured tree: `{commit}`.  bytes = packed weights + scales read once; the fraction is of 8 TB/s and is given for M <= 8 only.", "",
          "| what | bits | N | K | M | route | us | bytes / us | of 8 TB/s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        rate = r["bytes"] / r["us"]
        frac = f"{rate / HBM_BYTES_PER_US:.1%}" if r["m"] <= 8 and r["step"] != "dequant" else ""
        md.append(f"| {label[r['step']]} | {r['bits']} | {r['n']} | {r['k']} | {r['m']} | {r['route'] or ''} | {r['us']:.1f} | {rate:,.0f} | {frac} |")
    md += ["", "Group size 64.  Route 2 (the MFMA tile) is untuned, see DESIGN 4.16."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))
    print(json.dumps(dict(rows=rows, commit=commit)))


if __name__ == "__main__":
    main()
