"""The prompt workspace of the C++ runner (Llama::lay_out_prefill in csrc/host/runtime.cpp): the size mrs_llama_prefill_workspace_bytes asks for and the carve-up
prefill() makes of the caller's buffer are one layout.  Each case hands the runner EXACTLY the bytes it asked for, inside a larger 0xA5-filled allocation: no byte
behind them may change, and logits and every K / V page must equal, bit for bit, those of a second model that prefilled with four times the room.  The cases are the
branches of the layout and of the path selection: the exact path, the fused-dequant path on its f32 route (T <= 16) and on bf16 slabs with split-K partials (T > 16),
each dense and sparse-MoE, and the bf16-shadow path (library GEMMs: not in the host-emulation library)."""
import ctypes as C

import pytest

from tests.test_dec_model import Q4KM, _mk

pytestmark = pytest.mark.gpu

TAIL, FILL = 4096, 0xA5


def _prefill_in(oracle, dev, experts, mode, T, room):
    """A fresh tiny model (2 layers, bf16 pages) prefills T tokens in the first room(need) bytes of a FILL-ed allocation of room(need) + TAIL bytes."""
    import torch
    cfg, _, m, _, _ = _mk(oracle, dev, Q4KM(oracle), "bf16", experts=experts)
    if mode == 0:
        assert m.bf16_shadow or m.build_bf16_shadow(), "mode 0 is meant to run on the bf16 shadow copy"
    m.set_prefill_mode(mode)
    assert m.prefill_is_exact == (mode == 1)
    need = int(m._L.mrs_llama_prefill_workspace_bytes(C.byref(m._c), T))
    big = torch.full((room(need) + TAIL,), FILL, dtype=torch.uint8, device=dev)
    m._prefill_ws = big[:room(need)]  # the wrapper reuses a buffer that is large enough and passes its numel()
    logits = m.prefill([(1000 + 37 * i) % cfg.vocab_size for i in range(T)], 0)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert m._prefill_ws.data_ptr() == big.data_ptr() and m._prefill_ws.numel() == room(need), "the wrapper replaced the workspace under test"
    return m, big, need, logits


@pytest.mark.parametrize("model,mode,T", [("dense", 1, 9), ("dense", 2, 9), ("dense", 2, 40), ("moe4", 1, 40), ("moe4", 2, 9), ("moe4", 2, 40), ("dense", 0, 40)])
def test_prefill_stays_inside_the_workspace_it_asked_for(oracle, dev, request, model, mode, T):
    import torch
    emu = request.config.getoption("--host-emulation")
    if emu and mode == 0:
        pytest.skip("the bf16-shadow path needs hipBLASLt, which the host-emulation library does not have")
    if emu and T == 40:
        T = 17  # fibers: the smallest prompt on the bf16-slab side of prefill_big_min = 16
    experts = 4 if model == "moe4" else 0
    m1, big, need, l1 = _prefill_in(oracle, dev, experts, mode, T, lambda n: n)
    assert bool((big[need:] == FILL).all()), f"prefill wrote behind the {need} bytes it asked for: {int((big[need:] != FILL).sum())} of the next {TAIL} bytes changed"
    m2, _, _, l2 = _prefill_in(oracle, dev, experts, mode, T, lambda n: 4 * n)
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)), "logits depend on the size of the workspace"
    for layer, (k1, k2, v1, v2) in enumerate(zip(m1.key_caches, m2.key_caches, m1.value_caches, m2.value_caches)):
        assert torch.equal(k1.view(torch.int16), k2.view(torch.int16)) and torch.equal(v1.view(torch.int16), v2.view(torch.int16)), f"layer {layer}: K / V pages depend on the size of the workspace"
