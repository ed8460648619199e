"""Time the GPTQ kernels on one GPU and write profiles/gptq.md.

    python scripts/bench_gptq.py [--out profiles/gptq.md] [--iters 200]

4-bit, group 128, sequential g_idx (and one act-order line), (N, K) = (4096, 4096), (14336, 4096), (28672, 4096), (4096, 14336), M in 1, 8, 64, 512.
Per shape and M, in ONE process and alternating on the same data:
  fused     mrs_gptq_matmul (route 1 for M <= 8, route 2 above)
  recon     mrs_gptq_reconstruct + the library f16 matmul (what the reference does for M > 8 and for every 2/3-bit layer)
  q4k       the Q4_K MMVQ pair (activation quantizer + MMVQ launch) at the same shape, M <= 8 only
The measuring process runs under a time limit; if it fails nothing more is started on the GPU.
Timing: HIP events around `iters` launches after an equal warm-up, median of 5 rounds; for M <= 8 the weights rotate through > 256 MiB so that no launch
finds its bytes in the 256 MiB last-level cache.  bytes = qweight + qzeros + scales + g_idx, read once.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4096, 4096), (14336, 4096), (28672, 4096), (4096, 14336)]
MS = [1, 8, 64, 512]
BITS, GROUP = 4, 128
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


def nbytes_of(n, k):
    g = k // GROUP
    return k * BITS // 8 * n + g * n * BITS // 8 + 2 * g * n + 4 * k


def run(iters):
    import numpy as np
    import torch
    import mistralrs_amd  # noqa: F401
    from mistralrs_amd import gptq
    from mistralrs_amd.gguf import GgmlDType, QTensor, fast_mmvq
    dev, out = "cuda:0", []
    g = torch.Generator(device="cpu").manual_seed(0)
    rng = np.random.default_rng(0)

    def layer(n, k, act_order=False):
        qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (k * BITS // 32, n), dtype=torch.int32, generator=g).to(dev)
        qz = torch.randint(-2 ** 31, 2 ** 31 - 1, (k // GROUP, n * BITS // 32), dtype=torch.int32, generator=g).to(dev)
        sc = (torch.rand(k // GROUP, n, generator=g) * 0.01 + 0.001).to(torch.float16).to(dev)
        gi = torch.arange(k, dtype=torch.int32) // GROUP
        if act_order:
            gi = gi[torch.randperm(k, generator=g)]
        return gptq.GptqLayer.from_parts(qw, qz, sc, gi.to(dev), None, BITS)

    for n, k in SHAPES:
        nbytes = nbytes_of(n, k)
        c = _copies(nbytes, 1)
        layers = [layer(n, k) for _ in range(c)]
        dense = torch.empty(k, n, dtype=torch.float16, device=dev)
        for m in MS:
            cm = c if m <= 8 else 1
            it = iters if m <= 8 else max(10, iters // 10)
            x = (torch.rand(m, k, generator=g) * 4 - 2).to(torch.float16).to(dev)
            us = _time(lambda i: layers[i].forward_raw(x), it, cm)
            out.append(dict(step="fused", n=n, k=k, m=m, us=us, bytes=nbytes, route=gptq.last_route(), copies=cm))

            def recon(i):
                L = layers[i]
                gptq.reconstruct(L.qweight, L.qzeros, L.scales, L.g_idx, BITS, 1, out=dense, validate=False)
                return x @ dense
            us = _time(recon, max(10, iters // 10), cm)
            out.append(dict(step="recon", n=n, k=k, m=m, us=us, bytes=nbytes, route=0, copies=cm))
        if (n, k) == SHAPES[0]:
            ao = [layer(n, k, act_order=True) for _ in range(c)]
            for m in (1, 8):
                x = (torch.rand(m, k, generator=g) * 4 - 2).to(torch.float16).to(dev)
                us = _time(lambda i: ao[i].forward_raw(x), iters, c)
                out.append(dict(step="fused_act_order", n=n, k=k, m=m, us=us, bytes=nbytes, route=gptq.last_route(), copies=c))
            del ao
        del layers, dense
        qbytes = n * k // 256 * 144
        qc = _copies(qbytes, 1)
        packed = rng.integers(0, 256, (n, k // 256, 144), dtype=np.uint8)
        packed[:, :, 1] &= 0x3B  # keep the two f16 block scales finite
        packed[:, :, 3] &= 0x3B
        ws = [QTensor.from_numpy(GgmlDType.Q4K, (n, k), packed.reshape(n, -1), dev) for _ in range(qc)]
        for m in (1, 8):
            x = (torch.rand(m, k, generator=g) * 4 - 2).to(dev)
            us = _time(lambda i: fast_mmvq.plain(ws[i], x), iters, qc)
            out.append(dict(step="q4k", n=n, k=k, m=m, us=us, bytes=qbytes, route=0, copies=qc))
        del ws
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gptq.md"))
    a = ap.parse_args()
    if a.run:
        return run(a.iters)
    r = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--run", "--iters", str(a.iters)], capture_output=True, text=True)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        sys.exit(f"the measuring process failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
    rows = json.loads(line[7:])
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = os.environ.get("MRS_COMMIT", "unknown (no git metadata next to the run)")
    label = {"fused": "mrs_gptq_matmul", "fused_act_order": "mrs_gptq_matmul, act-order g_idx", "recon": "mrs_gptq_reconstruct + torch f16 matmul",
             "q4k": "Q4_K MMVQ pair (quantize + launch_mmvq_gguf_q4_k_f32_plain)"}
    md = ["# GPTQ kernels on one MI355X", "",
          f"Written by `python scripts/bench_gptq.py --iters {a.iters}` (one process; HIP events, {a.iters} launches per round after an equal warm-up, a tenth of that "
          "for M > 8 and for the reconstruct lines; median of 5 rounds; weights rotated through > 256 MiB for M <= 8).",
          f"Parent commit of the measured tree: `{commit}`.  4-bit, group 128.  bytes = packed weights + zeros + scales + g_idx read once (Q4_K: its 144-byte "
          "blocks); the fraction is of 8 TB/s and is given for the fused and Q4_K lines at M <= 8 only.", "",
          "| what | N | K | M | route | us | packed bytes / us | of 8 TB/s |", "|---|---|---|---|---|---|---|---|"]
    for r_ in rows:
        rate = r_["bytes"] / r_["us"]
        frac = f"{rate / HBM_BYTES_PER_US:.1%}" if r_["m"] <= 8 and r_["step"] != "recon" else ""
        md.append(f"| {label[r_['step']]} | {r_['n']} | {r_['k']} | {r_['m']} | {r_['route'] or ''} | {r_['us']:.1f} | {rate:,.0f} | {frac} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))
    print(json.dumps(dict(rows=rows, commit=commit)))


if __name__ == "__main__":
    main()
