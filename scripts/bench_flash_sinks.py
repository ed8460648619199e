"""Time prompt attention with sinks on one GPU at GPT-OSS shapes and write profiles/flash_attn_sinks.md.

    python scripts/bench_flash_sinks.py [--out profiles/flash_attn_sinks.md] [--iters 100]

H 64, Hkv 8, D 64, bf16, batch 1, q_len = kv_len = S in 512 / 2048 / 8192, window 0 and 128.  Per shape, in ONE process and alternating round by round
on the same data:
  kernel   paged_attn.flash_attn_sinks with sinks
  library  torch.nn.functional.scaled_dot_product_attention with an explicit boolean mask and no sink (K / V expanded to 64 heads outside the timed window)
Timing: HIP events around `iters * 2048 / S` launches after an equal warm-up, 5 rounds per side, the sides interleaved; the median is reported and
the spread is (max - min) / median over a side's rounds.  FLOPs = 4 * D * H * (visible (row, key) pairs): the two products over the unmasked part only, so a
side that computes masked tiles gets no credit for them.  The fraction is of the 2.5 PFLOP/s bf16 MFMA peak.  `diff` is max |kernel - library| with the sinks
off, at the timed size.  The measuring process runs under a time limit; if it fails nothing more is started on the GPU.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, HKV, D = 64, 8, 64
SEQS, WINDOWS = (512, 2048, 8192), (0, 128)
PEAK_FLOPS_PER_US = 2.5e9  # 2.5 PFLOP/s


def _round(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _time_sides(sides, iters):
    for fn in sides.values():
        _round(fn, iters)
    rounds = {name: [] for name in sides}
    for _ in range(5):
        for name, fn in sides.items():
            rounds[name].append(_round(fn, iters))
    return {name: (sorted(r)[2], (max(r) - min(r)) / sorted(r)[2]) for name, r in rounds.items()}


def visible_pairs(s, w):
    return sum(min(r + 1, w) if w > 0 else r + 1 for r in range(s))


def run(iters):
    import torch
    import mistralrs_amd  # noqa: F401
    from mistralrs_amd import paged_attn
    dev, out = "cuda:0", []
    g = torch.Generator(device="cpu").manual_seed(0)
    sinks = torch.randn(H, generator=g).to(dev)
    scale = D ** -0.5
    for s in SEQS:
        q = torch.randn(1, H, s, D, generator=g).to(torch.bfloat16).to(dev)
        k = torch.randn(1, HKV, s, D, generator=g).to(torch.bfloat16).to(dev)
        v = torch.randn(1, HKV, s, D, generator=g).to(torch.bfloat16).to(dev)
        ke, ve = k.repeat_interleave(H // HKV, dim=1), v.repeat_interleave(H // HKV, dim=1)
        pos = torch.arange(s, device=dev)
        for w in WINDOWS:
            mask = pos[None, :] <= pos[:, None]
            if w > 0:
                mask &= pos[None, :] > pos[:, None] - w
            sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(q, ke, ve, attn_mask=mask, scale=scale)
            diff = (paged_attn.flash_attn_sinks(q, k, v, None, scale, w).float() - sdpa().float()).abs().max().item()
            res = _time_sides({"kernel": lambda: paged_attn.flash_attn_sinks(q, k, v, sinks, scale, w), "library": sdpa},
                              max(3, iters * 2048 // s))
            for side, (us, spread) in res.items():
                out.append(dict(side=side, s=s, w=w, us=us, spread=spread, flops=4 * D * H * visible_pairs(s, w), diff=diff))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flash_attn_sinks.md"))
    a = ap.parse_args()
    if a.run:
        return run(a.iters)
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--run", "--iters", str(a.iters)], capture_output=True, text=True)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        sys.exit(f"the measuring process failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
    rows = json.loads(line[7:])
    label = {"kernel": "flash_attn_sinks (with sinks)", "library": "scaled_dot_product_attention, explicit mask, no sink"}
    md = ["# Prompt attention with sinks on one MI355X", "",
          f"Written by `python scripts/bench_flash_sinks.py --iters {a.iters}` (one process; HIP events, {a.iters} * 2048 / S launches per round after an equal "
          "warm-up; 5 rounds per side with the sides alternating, median).",
          "GPT-OSS attention shape: H 64, Hkv 8, D 64, bf16, batch 1, q_len = kv_len = S.  spread = (max - min) / median over a line's 5 rounds.  FLOPs count the "
          "unmasked (row, key) pairs only; the fraction is of the 2.5 PFLOP/s bf16 MFMA peak.  diff = max |kernel - library| with the sinks off.", "",
          "| what | S | W | us | spread | TFLOP/s | of bf16 peak | diff |", "|---|---|---|---|---|---|---|---|"]
    for r_ in rows:
        rate = r_["flops"] / r_["us"]
        md.append(f"| {label[r_['side']]} | {r_['s']} | {r_['w']} | {r_['us']:.1f} | {r_['spread']:.1%} | {rate / 1e6:.1f} | {rate / PEAK_FLOPS_PER_US:.1%} | {r_['diff']:.2e} |")
    md.append("")
    for s in SEQS:
        for w in WINDOWS:
            t = {r_["side"]: r_["us"] for r_ in rows if r_["s"] == s and r_["w"] == w}
            verdict = "the kernel is faster" if t["kernel"] < t["library"] else "the kernel LOSES to the library route"
            md.append(f"- S {s}, W {w}: {verdict} ({t['library'] / t['kernel']:.2f}x).")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
