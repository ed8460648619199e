"""Device time of the sampling launch sets at 128256 logits (the method of profiles/categorical_sampling.md): device events around back-to-back calls of the C entry
points, parameters already on the device, after a warm-up; several windows per figure; microseconds per call.  Prints one line per (rows, entry point)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mistralrs_amd import _lib, sampler  # noqa: E402

VOCAB, CALLS, WARM, WINDOWS = 128256, 1000, 50, 5


def main():
    dev = torch.device("cuda:0")
    vp, i, ll = C.c_void_p, C.c_int, C.c_int64
    rng = np.random.default_rng(0)
    for rows in (1, 8):
        x = torch.from_numpy((rng.standard_normal((rows, VOCAB)) * 3).astype(np.float32)).to(dev)
        nuc, cat, t1, tk = (sampler.Nucleus(VOCAB, dev, rows), sampler.Categorical(VOCAB, dev, rows), sampler.Top1(VOCAB, dev, rows),
                            sampler.TopK(VOCAB, 128, dev, rows))
        par = torch.tensor([[1 / 0.8] * rows, [0.37] * rows, [0.9] * rows, [0.0] * rows, [1.0] * rows, [0.05] * rows], dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        p = [par[j].data_ptr() for j in range(6)]
        nb = nuc.nblocks
        f_nuc = _lib.sym("core", "mrs_nucleus_large_f32_packed_batched", [vp] * 8 + [i] * 4 + [ll])
        calls = {
            "nucleus top_p=0.9": lambda: f_nuc(x.data_ptr(), p[0], p[1], p[2], p[3], nuc.block_values.data_ptr(), nuc.block_sums.data_ptr(), nuc.packed.data_ptr(), rows,
                                               VOCAB, 2048, nb, st),
            "nucleus min_p=0.05 only": lambda: f_nuc(x.data_ptr(), p[0], p[1], p[4], p[5], nuc.block_values.data_ptr(), nuc.block_sums.data_ptr(), nuc.packed.data_ptr(),
                                                     rows, VOCAB, 2048, nb, st),
            "categorical": lambda: cat._many(x.data_ptr(), p[0], p[1], cat.block_values.data_ptr(), cat.block_sums.data_ptr(), cat.packed.data_ptr(), rows, VOCAB, 2048, nb, st),
            "top1": lambda: t1._many(x.data_ptr(), t1.block_values.data_ptr(), t1.block_indices.data_ptr(), t1.packed.data_ptr(), None, rows, VOCAB, 2048, nb, st),
            "topk k=128": lambda: tk._many(x.data_ptr(), p[0], tk.block_values.data_ptr(), tk.block_indices.data_ptr(), tk.block_maxes.data_ptr(), tk.block_sums.data_ptr(),
                                           tk.packed.data_ptr(), rows, VOCAB, 128, 2048, nb, st),
        }
        for name, f in calls.items():
            for _ in range(WARM):
                f()
            torch.cuda.synchronize()
            us = []
            for _ in range(WINDOWS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(CALLS):
                    f()
                b.record()
                torch.cuda.synchronize()
                us.append(a.elapsed_time(b) * 1000.0 / CALLS)
            print(f"rows={rows} {name}: median {np.median(us):.2f} us, {min(us):.2f} .. {max(us):.2f}", flush=True)


if __name__ == "__main__":
    sys.exit(main())
