#!/usr/bin/env python
"""HQQ forward against its alternatives, one JSON line per case.

decode  (M = 1): fused dequant-GEMV (mrs_hqq_gemv) vs dequantize + dense matmul: us per call and packed-bytes rate.
prompt  (M in 16, 64, 512, 2048; bf16): `forward` (the fused MFMA tile kernel, mrs_hqq_gemm) vs what forward did before that kernel (dequantize() + library
        matmul) vs the library matmul on an already dense weight (the floor).  One process, the three sides alternate inside every round, every shape is warmed,
        HIP events around REPS eager calls, the median of ROUNDS rounds and the spread (max - min) / median of each side.  --no-crossover lifts
        hqq.MFMA_MAX_ROWS so that the kernel itself is timed at every M.
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import mistralrs_amd  # noqa: F401
from mistralrs_amd import hqq
from mistralrs_amd.hqq import HqqConfig, HqqLayer

SHAPES = ((4, 4096, 4096), (4, 14336, 4096), (4, 4096, 14336), (8, 4096, 4096))
ROUNDS, REPS = 7, 20
dev = torch.device("cuda:0")


def timeit_eager(f, reps=REPS):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def timeit(f, reps=REPS):  # one HIP graph of `reps` calls: device time, not the Python launch path (~15 us per eager call)
    f(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            for _ in range(reps):
                f()
    torch.cuda.current_stream().wait_stream(st)
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def decode():
    for bits, n, k in SHAPES:
        for dt in (torch.bfloat16, torch.float32):
            w = (torch.randn(n, k, device=dev) * 0.05).to(dt)
            layer = HqqLayer.quantize(w, HqqConfig(bits=bits, group_size=64))
            x = torch.randn(1, k, device=dev).to(dt)
            fused = timeit(lambda: layer.forward(x))
            unfused = timeit_eager(lambda: x.to(layer.dequantize().dtype) @ layer.dequantize().t())
            nbytes = n * k * bits // 8
            print(json.dumps({"bits": bits, "N": n, "K": k, "dtype": str(dt).split(".")[-1], "fused_us": round(fused, 1), "dequant_matmul_us": round(unfused, 1),
                              "packed_TBps": round(nbytes / fused / 1e6, 3)}), flush=True)


def prompt(rows=(16, 64, 512, 2048)):
    for bits, n, k in SHAPES:
        layer = HqqLayer.quantize(torch.randn(n, k, device=dev) * 0.05, HqqConfig(bits=bits, group_size=64)).to_dtype(torch.bfloat16)
        dense = layer.dequantize()
        for m in rows:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            sides = {"forward": lambda: layer.forward(x), "parent": lambda: x @ layer.dequantize().t(), "floor": lambda: x @ dense.t()}
            err = float((sides["forward"]().float() - sides["parent"]().float()).abs().max())
            route = hqq.last_route() if sides["forward"]() is not None else None
            for f in sides.values():  # every shape warmed
                timeit_eager(f, 3)
            t = {name: [] for name in sides}
            for _ in range(ROUNDS):
                for name, f in sides.items():
                    t[name].append(timeit_eager(f))
            med = {name: statistics.median(v) for name, v in t.items()}
            line = {"bits": bits, "N": n, "K": k, "M": m, "route": route, "max_abs_diff_vs_parent": round(err, 4)}
            for name in sides:
                line[f"{name}_us"] = round(med[name], 1)
                line[f"{name}_spread"] = round((max(t[name]) - min(t[name])) / med[name], 3)
            line["parent_over_forward"] = round(med["parent"] / med["forward"], 2)
            line["forward_over_floor"] = round(med["forward"] / med["floor"], 2)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("decode", "prompt", "all"), default="all")
    ap.add_argument("--no-crossover", action="store_true")
    ap.add_argument("--rows", default="16,64,512,2048", help="row counts of the prompt section")
    a = ap.parse_args()
    if a.no_crossover:
        hqq.MFMA_MAX_ROWS = 1 << 30
    if a.section in ("decode", "all"):
        decode()
    if a.section in ("prompt", "all"):
        prompt(tuple(int(v) for v in a.rows.split(",")))
