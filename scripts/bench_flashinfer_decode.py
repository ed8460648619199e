"""Time the FlashInfer-layout GQA decode on one GPU against paged_attn.paged_attention and write profiles/flashinfer_decode.md.

    python scripts/bench_flashinfer_decode.py [--out profiles/flashinfer_decode.md] [--ms 20]

heads / kv_heads 32 / 8 and 64 / 8, head_size 128, batch 1 / 8 / 64, every request `ctx` keys long with ctx in 1024 / 8192 / 32768, bf16 queries over bf16 and
over E4M3 pages (k_scale 0.5, v_scale 2), page size 32, shuffled pages.  Per shape, in ONE process and alternating round by round on the same keys:
  plan     paged_attn.flashinfer_decode with the plan of flashinfer_decode_split_pages(batch, kv_heads, ctx, page)
  one      paged_attn.flashinfer_decode with one tile per request, partition=False (one launch, no scratch)
  paged    paged_attn.paged_attention (its own v1 / v2 rule) on a vLLM-layout cache (x-packed K, transposed V) holding the same keys and values
Timing: HIP events around `iters` calls (iters sized so that a round lasts about --ms milliseconds) after an equal warm-up, 5 rounds per side, the sides
interleaved; the median is reported and the spread is (max - min) / median over a side's rounds.  bytes = K and V of every request once, plus Q and O; the
share is bytes / 8 TB/s over the time.  `diff` is max |one - paged| and max |plan - one| at the timed size.  The kernels' registers, LDS and scratch come
from scripts/kernel_resources.py.  The measuring process runs under a time limit; if it fails nothing more is started on the GPU.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
HEADS, HKV, D, BATCHES, CTXS, PAGE = (32, 64), 8, 128, (1, 8, 64), (1024, 8192, 32768), 32
HBM_BYTES_PER_US = 8e6  # 8 TB/s
SCALE = D ** -0.5


def run(ms):
    import torch
    import mistralrs_amd  # noqa: F401
    from mistralrs_amd import paged_attn
    from bench_mla import _time_sides
    dev, out, bf16 = "cuda:0", [], torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    for ctx in CTXS:
        for batch in BATCHES:
            npg = ctx // PAGE
            kc, vc = (torch.randn(batch * npg, HKV, PAGE, D, generator=g, device=dev, dtype=bf16) for _ in range(2))
            indices = torch.randperm(batch * npg, generator=g, device=dev).to(torch.int32)
            indptr = (torch.arange(batch + 1, device=dev) * npg).to(torch.int32)
            last = torch.full((batch,), PAGE, dtype=torch.int32, device=dev)
            lens = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
            tables = indices.view(batch, npg).contiguous()
            split = paged_attn.flashinfer_decode_split_pages(batch, HKV, ctx, PAGE)
            plans = {"plan": paged_attn.flashinfer_decode_plan([ctx] * batch, PAGE, split, device=dev),
                     "one": paged_attn.flashinfer_decode_plan([ctx] * batch, PAGE, None, device=dev)}
            for cache in ("bf16", "fp8"):
                ks, vs = (0.5, 2.0) if cache == "fp8" else (1.0, 1.0)
                k, v = (kc, vc) if cache == "bf16" else ((kc.float() / ks).to(torch.float8_e4m3fn), (vc.float() / vs).to(torch.float8_e4m3fn))
                x = 16 // k.element_size()  # the same pages in paged_attention's layout: K [pages, kvh, D / x, page, x], V [pages, kvh, D, page]
                kp = k.view(torch.uint8 if cache == "fp8" else bf16).view(batch * npg, HKV, PAGE, D // x, x).permute(0, 1, 3, 2, 4).contiguous()
                vp = v.view(torch.uint8 if cache == "fp8" else bf16).permute(0, 1, 3, 2).contiguous()
                st = (torch.tensor([ks], device=dev), torch.tensor([vs], device=dev)) if cache == "fp8" else (None, None)
                for heads in HEADS:
                    q = torch.randn(batch, heads, D, generator=g, device=dev, dtype=bf16)
                    fi = lambda side: paged_attn.flashinfer_decode(q, k, v, indptr, indices, last, plans[side], SCALE, k_scale=ks, v_scale=vs,
                                                                   partition=side == "plan")
                    paged = lambda: paged_attn.paged_attention(q, kp, vp, tables, lens, ctx, SCALE, k_scale=st[0], v_scale=st[1])
                    d_ref = (fi("one").float() - paged().float()).abs().max().item()
                    d_split = (fi("plan").float() - fi("one").float()).abs().max().item()
                    res = _time_sides({"plan": lambda: fi("plan"), "one": lambda: fi("one"), "paged": paged}, ms)
                    for side, (us, spread) in res.items():
                        out.append(dict(side=side, cache=cache, heads=heads, batch=batch, ctx=ctx, us=us, spread=spread, d_ref=d_ref, d_split=d_split,
                                        tiles=plans[side].request_indices.numel() // batch if side != "paged" else 0,
                                        bytes=2 * batch * ctx * HKV * D * k.element_size() + 2 * batch * heads * D * 2))
                del k, v, kp, vp
            del kc, vc
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--ms", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flashinfer_decode.md"))
    a = ap.parse_args()
    if a.run:
        return run(a.ms)
    r = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--run", "--ms", str(a.ms)], capture_output=True, text=True)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        sys.exit(f"the measuring process failed (exit {r.returncode}); nothing more is started on the GPU\n{r.stderr[-2000:]}")
    rows = json.loads(line[7:])
    label = {"plan": "flashinfer_decode, planned split", "one": "flashinfer_decode, one tile, no partition", "paged": "paged_attention (v1 / v2)"}
    md = ["# FlashInfer-layout GQA decode on one MI355X", "",
          f"Written by `python scripts/bench_flashinfer_decode.py --ms {a.ms:g}` (one process; HIP events around rounds of about {a.ms:g} ms after an equal "
          "warm-up; 5 rounds per side with the sides alternating, median).",
          f"bf16 queries, head_size {D}, {HKV} KV heads, page size {PAGE}, shuffled pages, every request `ctx` keys; E4M3 pages with k_scale 0.5, v_scale 2.  "
          "spread = (max - min) / median over a line's 5 rounds.  bytes = K and V of every request once, plus Q and O; share = bytes / 8 TB/s over the "
          "time.  tiles = plan tiles per request.  diff = max |one tile - paged_attention| on the first two lines of a shape, max |planned - one tile| "
          "on the planned line.  Losses are listed below the table as measured.", "",
          "| what | pages | heads | batch | ctx | tiles | us | spread | TB/s | share of 8 TB/s | diff |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r_ in rows:
        diff = r_["d_split"] if r_["side"] == "plan" else r_["d_ref"]
        md.append(f"| {label[r_['side']]} | {r_['cache']} | {r_['heads']} | {r_['batch']} | {r_['ctx']} | {r_['tiles'] or ''} | {r_['us']:.1f} | {r_['spread']:.1%} | "
                  f"{r_['bytes'] / r_['us'] / 1e6:.2f} | {r_['bytes'] / HBM_BYTES_PER_US / r_['us']:.1%} | {diff:.2e} |")
    md.append("")
    for cache in ("bf16", "fp8"):
        for heads in HEADS:
            for batch in BATCHES:
                for ctx in CTXS:
                    t = {r_["side"]: r_["us"] for r_ in rows if (r_["cache"], r_["heads"], r_["batch"], r_["ctx"]) == (cache, heads, batch, ctx)}
                    best = min(t["one"], t["plan"])
                    notes = []
                    if t["plan"] > t["one"] * 1.02:
                        notes.append(f"the planned split LOSES to one tile ({t['plan'] / t['one']:.2f}x the time)")
                    notes.append(f"flashinfer_decode is {t['paged'] / best:.2f}x paged_attention" if best < t["paged"]
                                 else f"flashinfer_decode LOSES to paged_attention ({best / t['paged']:.2f}x the time)")
                    md.append(f"- {cache} pages, heads {heads}, batch {batch}, ctx {ctx}: " + "; ".join(notes) + ".")
    md += ["", "## Kernel resources (`scripts/kernel_resources.py`, libmistralrspagedattention.so)", "",
           "| kernel | VGPRs (incl. AGPRs) | AGPRs | LDS bytes (static) | scratch | spills |", "|---|---|---|---|---|---|"]
    from kernel_resources import resources
    for k in sorted(resources(os.path.join(ROOT, "mistral.rs_amd", "lib", "libmistralrspagedattention.so")), key=lambda k: k["demangled"]):
        if "mrs::fid" in k["demangled"]:  # the f16 instantiations (names the demangler leaves alone) equal the bf16 ones
            md.append(f"| `{k['demangled'].split('(')[0]}` | {k.get('vgpr_count', 0)} | {k.get('agpr_count', 0)} | {k.get('group_segment_fixed_size', 0)} | "
                      f"{k.get('private_segment_fixed_size', 0)} | {k.get('vgpr_spill_count', 0)} |")
    md += ["", "The decode kernel's LDS is dynamic: 320 * head_size + 512 bytes per workgroup (20992 / 41472 / 82432 at head_size 64 / 128 / 256)."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
