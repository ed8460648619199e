"""What one FP8 MFMA keeps of a small product next to a large one: the measurement behind the `mfma_cut` term of tests/test_zz_fp8_gpu.py.

    python scripts/probe_fp8_mfma.py [--append profiles/fp8.md]

Through `matmul_q` with unit scales, bf16 out, K = 80, on route 1 (v_mfma_f32_16x16x32_fp8_fp8, 16 rows) and route 2 (v_mfma_f32_32x32x16_fp8_fp8, all rows).  A row
of x holds `big` at k = 0, 2 and 64 and a small value v at k = 1 and 8; three weight rows pick
  same   big * big + v * 1 - big * big, all three products in ONE instruction (k = 0, 1, 2)
  next   big * big + v * 1 in one instruction, - big * big in a later one (k = 64): does the accumulator carry the cut sum on unharmed?
  acc    big * big in one instruction, v * 1 in the next (k = 8), - big * big later: is a product cut against the ACCUMULATOR's exponent?
The f64 result is v in every case.  k = 0..7, 8..15 and 64..71 lie in three different instructions on both routes (csrc/fp8_pertensor.hip)."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--append", default=None, help="a markdown file to append the table to")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mistralrs_amd  # noqa: F401
    from mistralrs_amd import fp8
    from tests.test_blockwise_fp8 import e4m3_encode_f16
    enc = lambda v: e4m3_encode_f16(np.asarray(v, np.float16))
    vals = np.array([s * m * 2.0 ** -j for s in (1, -1) for m in (1.0, 1.75) for j in range(-4, 8)])  # 16 .. 2^-7 and 28 .. 1.75 * 2^-7, both signs; exact in E4M3
    one = torch.ones(1, device="cuda")
    lines = ["| route | big^2 | case | v -> result, where the result is not v (`all kept` otherwise) |", "|---|---|---|---|"]
    for big in (256.0, 16.0, 1.0):
        x, w = np.zeros((len(vals), 80)), np.zeros((16, 80))
        x[:, [0, 2, 64]], x[:, 1], x[:, 8] = big, vals, vals
        w[0, [0, 1, 2]], w[1, [0, 1, 64]], w[2, [0, 8, 64]] = [big, 1, -big], [big, 1, -big], [big, 1, -big]
        xq, wq = enc(x), enc(w)
        mm = lambda rows: fp8.matmul_q(torch.from_numpy(xq[rows]).cuda(), torch.from_numpy(wq).cuda(), one, one, None, torch.bfloat16).float().cpu().numpy()
        for step in (16, len(vals)):  # 16 rows a call: route 1; all rows in one call: route 2
            out = np.concatenate([mm(slice(i, i + step)) for i in range(0, len(vals), step)])
            route = fp8.fp8_pertensor_last_route()
            for c, case in enumerate(("same", "next", "acc")):
                lost = [f"{v:g} -> {r:g}" for v, r in zip(vals, out[:, c]) if v != r]
                lines.append(f"| {route} | 2^{int(np.log2(big * big))} | {case} | {', '.join(lost) or 'all kept'} |")
    print("\n".join(lines))
    if a.append:
        with open(a.append, "a") as f:
            f.write("\n## What one FP8 MFMA keeps (scripts/probe_fp8_mfma.py)\n\n" + __doc__.split("\n\n", 2)[2].strip() + "\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
