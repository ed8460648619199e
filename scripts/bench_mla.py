"""Time MLA paged decode on one GPU at DeepSeek shapes and write profiles/mla.md.

    python scripts/bench_mla.py [--out profiles/mla.md] [--ms 20]

heads 128 and 16 (one rank of TP = 8), batch 1 / 8 / 64, every request `ctx` keys long with ctx in 1024 / 8192 / 32768, bf16, page size 32, shuffled pages.
Per shape, in ONE process and alternating round by round on the same data:
  one      paged_attn.flashinfer_mla_decode(..., num_splits=1)
  auto     paged_attn.flashinfer_mla_decode(...) with the automatic split count (max_kv_len = ctx)
  torch    index_select of the request's pages from both caches, the score as two bf16 matmuls (latent + rotary), an f32 softmax, one bf16 matmul for the output
Timing: HIP events around `iters` calls (iters sized so that a round lasts about --ms milliseconds) after an equal warm-up, 5 rounds per side, the sides
interleaved; the median is reported and the spread is (max - min) / median over a side's rounds.  bytes = every request's ctx * 576 * 2 once, plus Q and O;
FLOPs = 2 * heads * ctx * (576 + 512) per request.  The share of peak is the larger of bytes / 8 TB/s and FLOPs / 2.5 PFLOP/s (bf16 MFMA) over the time;
the column `bound` says which.  `diff` is max |one - torch| and max |auto - one| at the timed size.  The kernels' registers, LDS and scratch come from
scripts/kernel_resources.py.  The measuring process runs under a time limit; if it fails nothing more is started on the GPU.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADS, BATCHES, CTXS, PAGE = (128, 16), (1, 8, 64), (1024, 8192, 32768), 32
HBM_BYTES_PER_US, PEAK_FLOPS_PER_US = 8e6, 2.5e9  # 8 TB/s, 2.5 PFLOP/s
SCALE = 192 ** -0.5


def _round(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _time_sides(sides, ms):
    iters = {name: max(2, min(200, int(ms * 1e3 / max(_round(fn, 2), 1.0)))) for name, fn in sides.items()}  # the sizing pass is the first warm-up
    for name, fn in sides.items():
        _round(fn, iters[name])
    rounds = {name: [] for name in sides}
    for _ in range(5):
        for name, fn in sides.items():
            rounds[name].append(_round(fn, iters[name]))
    return {name: (sorted(r)[2], (max(r) - min(r)) / sorted(r)[2]) for name, r in rounds.items()}


def run(ms):
    import torch
    import mistralrs_amd  # noqa: F401
    from mistralrs_amd import paged_attn
    dev, out = "cuda:0", []
    g = torch.Generator(device=dev).manual_seed(0)
    for ctx in CTXS:
        for batch in BATCHES:
            npg = ctx // PAGE
            ckv = torch.randn(batch * npg, PAGE, 512, generator=g, device=dev, dtype=torch.bfloat16)
            kpe = torch.randn(batch * npg, PAGE, 64, generator=g, device=dev, dtype=torch.bfloat16)
            indices = torch.randperm(batch * npg, generator=g, device=dev).to(torch.int32)
            indptr = (torch.arange(batch + 1, device=dev) * npg).to(torch.int32)
            last = torch.full((batch,), PAGE, dtype=torch.int32, device=dev)
            idx64 = indices.long()
            for heads in HEADS:
                qn = torch.randn(batch, heads, 512, generator=g, device=dev, dtype=torch.bfloat16)
                qp = torch.randn(batch, heads, 64, generator=g, device=dev, dtype=torch.bfloat16)

                def baseline():
                    c = ckv.index_select(0, idx64).view(batch, ctx, 512)
                    r = kpe.index_select(0, idx64).view(batch, ctx, 64)
                    p = torch.softmax((qn @ c.mT + qp @ r.mT).float() * SCALE, dim=-1)
                    return p.to(torch.bfloat16) @ c

                one = lambda: paged_attn.flashinfer_mla_decode(qn, qp, ckv, kpe, indptr, indices, last, SCALE, num_splits=1)
                auto = lambda: paged_attn.flashinfer_mla_decode(qn, qp, ckv, kpe, indptr, indices, last, SCALE, max_kv_len=ctx)
                d_ref = (one().float() - baseline().float()).abs().max().item()
                d_split = (auto().float() - one().float()).abs().max().item()
                res = _time_sides({"one": one, "auto": auto, "torch": baseline}, ms)
                for side, (us, spread) in res.items():
                    out.append(dict(side=side, heads=heads, batch=batch, ctx=ctx, us=us, spread=spread, d_ref=d_ref, d_split=d_split,
                                    splits=paged_attn.mla_decode_splits(batch, heads, ctx) if side == "auto" else 1,
                                    bytes=batch * ctx * 576 * 2 + batch * heads * (576 + 512) * 2, flops=2 * batch * heads * ctx * (576 + 512)))
            del ckv, kpe
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--ms", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mla.md"))
    a = ap.parse_args()
    if a.run:
        return run(a.ms)
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--run", "--ms", str(a.ms)], capture_output=True, text=True)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        sys.exit(f"the measuring process failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
    rows = json.loads(line[7:])
    label = {"one": "kernel, 1 split", "auto": "kernel, automatic split", "torch": "torch: index_select, bf16 matmuls, f32 softmax"}
    md = ["# MLA paged decode on one MI355X", "",
          f"Written by `python scripts/bench_mla.py --ms {a.ms:g}` (one process; HIP events around rounds of about {a.ms:g} ms after an equal warm-up; 5 rounds per "
          "side with the sides alternating, median).",
          "bf16, page size 32, shuffled pages, every request `ctx` keys.  spread = (max - min) / median over a line's 5 rounds.  bytes = ctx * 576 * 2 per request "
          "once, plus Q and O.  The share is of the hardware's least time: the larger of bytes / 8 TB/s (`hbm`) and FLOPs / 2.5 PFLOP/s (`mfma`).  diff = "
          "max |1 split - torch| on the kernel rows' first line, max |automatic - 1 split| on the second.", "",
          "| what | heads | batch | ctx | splits | us | spread | TB/s | share of peak | bound | diff |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r_ in rows:
        t_b, t_f = r_["bytes"] / HBM_BYTES_PER_US, r_["flops"] / PEAK_FLOPS_PER_US
        diff = r_["d_split"] if r_["side"] == "auto" else r_["d_ref"]
        md.append(f"| {label[r_['side']]} | {r_['heads']} | {r_['batch']} | {r_['ctx']} | {r_['splits']} | {r_['us']:.1f} | {r_['spread']:.1%} | "
                  f"{r_['bytes'] / r_['us'] / 1e6:.2f} | {max(t_b, t_f) / r_['us']:.1%} | {'hbm' if t_b >= t_f else 'mfma'} | {diff:.2e} |")
    md.append("")
    for heads in HEADS:
        for batch in BATCHES:
            for ctx in CTXS:
                t = {r_["side"]: r_["us"] for r_ in rows if (r_["heads"], r_["batch"], r_["ctx"]) == (heads, batch, ctx)}
                best = min(t["one"], t["auto"])
                notes = []
                if t["auto"] > t["one"] * 1.02:
                    notes.append(f"the automatic split LOSES to one split ({t['auto'] / t['one']:.2f}x the time)")
                notes.append(f"the kernel is {t['torch'] / best:.2f}x the torch route" if best < t["torch"] else f"the kernel LOSES to the torch route ({best / t['torch']:.2f}x the time)")
                md.append(f"- heads {heads}, batch {batch}, ctx {ctx}: " + "; ".join(notes) + ".")
    md += ["", "## Kernel resources (`scripts/kernel_resources.py`, libmistralrspagedattention.so)", "", "| kernel | VGPRs (incl. AGPRs) | AGPRs | LDS bytes (static) | scratch | spills |",
           "|---|---|---|---|---|---|"]
    from kernel_resources import resources
    for k in sorted(resources(os.path.join(ROOT, "mistral.rs_amd", "lib", "libmistralrspagedattention.so")), key=lambda k: k["demangled"]):
        if "mrs::mla" in k["demangled"]:  # the f16 instantiations (names the demangler leaves alone) equal the bf16 ones
            md.append(f"| `{k['demangled'].split('(')[0]}` | {k.get('vgpr_count', 0)} | {k.get('agpr_count', 0)} | {k.get('group_segment_fixed_size', 0)} | "
                      f"{k.get('private_segment_fixed_size', 0)} | {k.get('vgpr_spill_count', 0)} |")
    md.append("")
    md.append("The decode kernel's LDS is dynamic: 142336 bytes per workgroup for the 64-head block, 109056 for the 32-head block (requested through the function attribute).")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
