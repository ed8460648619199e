"""Time of the batched penalties launch at 128256 logits against the chain of single-row launches it replaces (profiles/penalties_engine.md).

  kernel      device events around back-to-back calls of `mrs_penalties_f32_batched`, parameters already on the device (the method of time_nucleus.py);
  call        host clock around `sampler.Penalties.__call__` (packing, two uploads, one launch) ending in a device synchronise;
  chain       host clock around the reference's way (sampler.rs:1090-1169) for the same rows, ending in a synchronise: per row a dict over the generated part and one
              over the whole context, an upload of ids and counts for each, `apply_sparse_penalties_f32` twice and `apply_sparse_logits_bias_f32` once (each a copy + a
              sparse update launch).  `--chain-lib` names the libmistralrscuda.so the chain is called in (a build of the parent commit, so that the yardstick is not the
              code under test); without it the chain runs in this tree's library and the output says so;
  step        host clock around a nucleus step end to end (draw + copy of the packed rows to the host), with and without `Penalties` in front.
Several windows per figure; microseconds per call (all rows), median and lowest .. highest window."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mistralrs_amd import _lib, sampler  # noqa: E402

VOCAB, WINDOWS = 128256, 5
VP, I, F, LL = C.c_void_p, C.c_int, C.c_float, C.c_int64


def windows(f, calls, warm):
    """host clock: `calls` calls of f then a synchronise, WINDOWS times"""
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    us = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / calls)
    return us


def event_windows(f, calls, warm):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    us = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            f()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1000.0 / calls)
    return us


def show(rows, ctx_len, what, us):
    print(f"rows={rows} context={ctx_len} {what}: median {np.median(us):.2f} us, {min(us):.2f} .. {max(us):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain-lib", default=None, help="libmistralrscuda.so of a build of the parent commit")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.chain_lib:
        lib = C.CDLL(os.path.abspath(a.chain_lib))
        f_pen, f_bias = lib.apply_sparse_penalties_f32, lib.apply_sparse_logits_bias_f32
        f_pen.argtypes, f_pen.restype = [VP, VP, VP, VP, I, I, F, F, F, LL], None
        f_bias.argtypes, f_bias.restype = [VP, VP, VP, VP, I, I, LL], None
        print(f"chain: {a.chain_lib}")
    else:
        f_pen = _lib.sym("core", "apply_sparse_penalties_f32", [VP, VP, VP, VP, I, I, F, F, F, LL])
        f_bias = _lib.sym("core", "apply_sparse_logits_bias_f32", [VP, VP, VP, VP, I, I, LL])
        print("chain: this tree's library (no --chain-lib)")
    f_new = _lib.sym("core", "mrs_penalties_f32_batched", [VP] * 11 + [I, I, I, LL])
    rng = np.random.default_rng(0)
    st = torch.cuda.current_stream().cuda_stream
    fp, pp, rp = 0.5, 0.25, 1.1
    for rows in (1, 8):
        x = torch.from_numpy((rng.standard_normal((rows, VOCAB)) * 3).astype(np.float32)).to(dev)
        t1, t2, dst = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        bias = {int(t): float(v) for t, v in zip(rng.permutation(VOCAB)[:16], rng.standard_normal(16))}
        nuc = sampler.Nucleus(VOCAB, dev, rows)
        for ctx_len in (256, 4096):
            distinct = rng.permutation(VOCAB)[: max(ctx_len // 6, 1)]  # a context repeats itself: about six occurrences per distinct token
            ctxs = [distinct[rng.integers(0, distinct.size, ctx_len)].tolist() for _ in range(rows)]
            plen = ctx_len // 2
            pen = sampler.Penalties(VOCAB, dev, max_rows=rows, max_context=rows * ctx_len)
            call = lambda: pen(x, ctxs, plen, fp, pp, rp, bias)
            want = call().clone()
            # ---- kernel alone: the parameters the wrapper has just uploaded stay where they are
            ip, fl = pen._ints.data_ptr(), pen._floats.data_ptr()
            nb = 16 * rows
            at = lambda base, n: base + 4 * n
            kernel = lambda: f_new(x.data_ptr(), pen.dst.data_ptr(), at(ip, 3 * rows + 2 + nb), ip, at(ip, rows + 1), fl, at(fl, rows), at(fl, 2 * rows), at(ip, 3 * rows + 2),
                                   at(fl, 3 * rows), at(ip, 2 * rows + 1), rows, VOCAB, sampler.CHUNK_SIZE, st)
            show(rows, ctx_len, "kernel mrs_penalties_f32_batched (device events)", event_windows(kernel, 1000, 50))
            assert torch.equal(pen.dst[:rows], want)
            show(rows, ctx_len, "call sampler.Penalties (packing + 2 uploads + 1 launch, host clock)", windows(call, 200, 20))

            # ---- the chain, the reference's way
            def chain():
                for r in range(rows):
                    ctx = ctxs[r]
                    cur = x[r]
                    for tokens, args, out in ((ctx[plen:], (fp, pp, 1.0), t1[r]), (ctx, (0.0, 0.0, rp), t2[r])):
                        counts = {}
                        for t in tokens:
                            counts[t] = counts.get(t, 0) + 1
                        ids = torch.tensor(list(counts.keys()), dtype=torch.int32).to(dev)
                        cnt = torch.tensor(list(counts.values()), dtype=torch.float32).to(dev)
                        f_pen(cur.data_ptr(), out.data_ptr(), ids.data_ptr(), cnt.data_ptr(), VOCAB, len(counts), *args, st)
                        cur = out
                    ids = torch.tensor(list(bias.keys()), dtype=torch.int32).to(dev)
                    val = torch.tensor(list(bias.values()), dtype=torch.float32).to(dev)
                    f_bias(cur.data_ptr(), dst[r].data_ptr(), ids.data_ptr(), val.data_ptr(), VOCAB, len(bias), st)
            us = windows(chain, 100, 10)
            assert torch.equal(dst, want), "the chain and the batched launch differ"
            show(rows, ctx_len, "chain of single-row launches (host dicts + uploads + 6 launches per row, host clock)", us)
            # ---- the chain's launches alone: lists already on the device
            lists = []
            for r in range(rows):
                per = []
                for tokens in (ctxs[r][plen:], ctxs[r]):
                    ids, cnt = np.unique(np.asarray(tokens), return_counts=True)
                    per.append((torch.from_numpy(ids.astype(np.int32)).to(dev), torch.from_numpy(cnt.astype(np.float32)).to(dev)))
                per.append((torch.tensor(list(bias.keys()), dtype=torch.int32).to(dev), torch.tensor(list(bias.values()), dtype=torch.float32).to(dev)))
                lists.append(per)

            def chain_launches():
                for r in range(rows):
                    (gi, gc), (ai, ac), (bi, bv) = lists[r]
                    f_pen(x[r].data_ptr(), t1[r].data_ptr(), gi.data_ptr(), gc.data_ptr(), VOCAB, gi.numel(), fp, pp, 1.0, st)
                    f_pen(t1[r].data_ptr(), t2[r].data_ptr(), ai.data_ptr(), ac.data_ptr(), VOCAB, ai.numel(), 0.0, 0.0, rp, st)
                    f_bias(t2[r].data_ptr(), dst[r].data_ptr(), bi.data_ptr(), bv.data_ptr(), VOCAB, bi.numel(), st)
            show(rows, ctx_len, "chain, launches alone (lists on the device, device events)", event_windows(chain_launches, 300, 20))
            assert torch.equal(dst, want)
            # ---- a nucleus step end to end
            us_u = [0.37] * rows
            plain = lambda: nuc(x, 0.8, us_u, 0.9, 0.0).cpu()
            penalized = lambda: nuc(pen(x, ctxs, plen, fp, pp, rp, bias), 0.8, us_u, 0.9, 0.0).cpu()
            show(rows, ctx_len, "step nucleus top_p=0.9, unpenalized (draw + copy to the host, host clock)", windows(plain, 200, 20))
            show(rows, ctx_len, "step nucleus top_p=0.9, Penalties in front (host clock)", windows(penalized, 200, 20))


if __name__ == "__main__":
    sys.exit(main())
