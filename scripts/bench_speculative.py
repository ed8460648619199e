#!/usr/bin/env python3
"""Speculative decoding on bench.py's default model (Llama-3-8B shapes, Q4_K_M, synthetic weights, one GPU): what a round costs and when it pays.

    python scripts/bench_speculative.py [--small] [--prompt-len 512] [--new 128] [--steps 32] [--markdown FILE]

Reports, as one JSON line (and as the table of profiles/speculative.md with --markdown):
  * ms per eager batch-1 step (`decode_step`) and per captured-graph replay -- the parent's figures, from the same run;
  * ms per verify step at 2..8 rows (`verify_step`), and per verifier launch group + state advance;
  * tok/s of `generate_speculative` with a replay proposer (it drafts the plain run's own tokens) at planted acceptance: every draft right, an error every
    2 / 4 / 8 drafts, every draft wrong -- for n_draft in 1, 2, 4, 7 -- next to the plain greedy run of the same tokens, and a check that the ids are the plain run's;
  * tok/s with `NGramProposer` on a repetitive prompt;
  * the break-even acceptance: the extra tokens a round of r rows must emit on average to match the batch-1 rate, (t_round(r) / t_step) - 1.
Every timed leg synchronises on both sides.  The speculative loop is host-driven (one read-back per round), so its fair neighbour is the EAGER batch-1 loop; the graph
replay rate is printed next to it because that is what `bench.py` reports."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Replay:
    """drafts the plain run's own tokens; `every` > 0 plants an error into every `every`-th draft it makes (1 = all wrong, 0 = none)"""

    def __init__(self, plain, vocab, every=0):
        self.plain, self.vocab, self.every = plain, vocab, every

    def reset(self):
        self.made = 0

    def propose(self, context, k_max, temperature=0.0, seed=0, n_generated=0):
        out = []
        for t in self.plain[n_generated:n_generated + k_max]:
            self.made += 1
            out.append((t + 1) % self.vocab if self.every and self.made % self.every == 0 else t)
        return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="tiny config (smoke), not the benchmark")
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--new", type=int, default=128, help="tokens generated per end-to-end leg")
    ap.add_argument("--steps", type=int, default=32, help="timed repetitions of a single step")
    ap.add_argument("--markdown", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    import bench
    from mistralrs_amd import speculative
    from mistralrs_amd.llama import LlamaConfig
    dev = torch.device("cuda:0")
    max_ctx = (a.prompt_len + a.new + 16 + 63) // 64 * 64
    if a.small:
        cfg = LlamaConfig(hidden_size=512, intermediate_size=1024, num_layers=2, num_heads=4, num_kv_heads=2, vocab_size=2048, head_dim=128, max_batch=8,
                          max_context_len=max_ctx, max_position_embeddings=max(8192, max_ctx))
        name = "tiny-llama (smoke)"
    else:
        cfg = LlamaConfig.llama3_8b(max_batch=8, max_context_len=max_ctx, max_position_embeddings=max(8192, max_ctx))
        name = "Llama-3-8B Q4_K_M"
    model = bench.build_model(cfg, dev, seed=0, max_new_tokens=a.new + 8)
    if model.decode_path != "engine":
        raise SystemExit("bench_speculative: the model does not run on the decode engine")
    sync = torch.cuda.synchronize
    prompt = [(1000 + i % 2048) % cfg.vocab_size for i in range(a.prompt_len)]

    def timed(fn, reps):
        fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        return (time.perf_counter() - t0) / reps * 1e3

    # ---- the plain greedy run: its tokens (the replay proposer's script) and the eager batch-1 rate
    first = int(model.prefill(prompt, 0).argmax())

    def plain_run():
        model.set_state([prompt[-1]], [len(prompt) - 1])
        model.step_counter.zero_()
        for _ in range(a.new):
            model.decode_step(1)
        sync()
        return model.tokens_out[0, :a.new].cpu().numpy().tolist()

    model.prefill(prompt[:-1], 0)
    plain = plain_run()
    assert plain[0] == first or not model.prefill_is_exact, "prefill and decode disagree on the first token"
    t0 = time.perf_counter()
    plain_run()
    plain_s = time.perf_counter() - t0
    res = {"model": name, "prompt_len": a.prompt_len, "new_tokens": a.new, "eager_batch1_ms": plain_s / a.new * 1e3, "eager_batch1_tok_s": a.new / plain_s}

    # ---- single steps at a fixed position (the state is put back before every step)
    pos = len(prompt) - 1

    def at_anchor(fn):
        def run():
            model.set_state_seq(0, prompt[-1], pos)
            fn()
        return run
    base = timed(at_anchor(lambda: None), a.steps)  # the host cost of putting the state back, subtracted below
    res["set_state_ms"] = base
    res["decode_step_ms"] = timed(at_anchor(lambda: model.decode_step(1)), a.steps) - base
    model.set_state([prompt[-1]], [pos])
    model.step_counter.zero_()
    model.capture_decode_graph(1)
    reps = min(a.steps, cfg.max_context_len - 2 - pos, a.new)
    model.replay()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps - 1):
        model.replay()
    sync()
    res["graph_replay_ms"] = (time.perf_counter() - t0) / max(1, reps - 1) * 1e3
    verify = speculative.SpecVerify(cfg.vocab_size, dev)
    res["verify_step_ms"], res["verifier_ms"], res["break_even_extra_tokens"] = {}, {}, {}
    for rows in range(2, 9):
        drafts = plain[:rows - 1]
        t_step = timed(at_anchor(lambda: model.verify_step(0, rows, drafts)), a.steps) - base
        logits = model.verify_step(0, rows, drafts)

        def judge():
            verify(logits, model.verify_ids_ptr + 4, [0, rows], 0.0)
            model.spec_advance(verify.n_accepted, verify.out_tokens, 0)
            model.step_counter.zero_()
        t_judge = timed(at_anchor(judge), a.steps) - base
        res["verify_step_ms"][rows] = t_step
        res["verifier_ms"][rows] = t_judge
        res["break_even_extra_tokens"][rows] = (t_step + t_judge) / res["decode_step_ms"] - 1.0

    # ---- end to end: generate_speculative against the plain run of the same tokens
    def spec_leg(proposer, n_draft, p=prompt, want=plain):
        speculative.generate_speculative(model, p, min(16, a.new), proposer, n_draft)  # warm-up
        sync()
        start = []

        def prompt_done():  # the prompt is not part of the decode rate (the plain legs do not time it either): the clock starts once it is in the pages
            sync()
            start.append(time.perf_counter())
        toks, st = speculative.generate_speculative(model, p, a.new, proposer, n_draft, after_prompt=prompt_done)
        sync()
        dt = time.perf_counter() - start[0]
        return {"tok_s": len(toks) / dt, "rounds": st["rounds"], "proposed": st["proposed"], "accepted": st["accepted"], "lossless": want is None or toks == want}
    res["replay"] = {}
    for label, every in (("all", 0), ("err/8", 8), ("err/4", 4), ("err/2", 2), ("none", 1)):
        res["replay"][label] = {k: spec_leg(Replay(plain, cfg.vocab_size, every), k) for k in (1, 2, 4, 7)}
    rep_prompt = ([(77 + 13 * i) % cfg.vocab_size for i in range(16)] * (a.prompt_len // 16 + 1))[:a.prompt_len]
    model.prefill(rep_prompt[:-1], 0)
    model.set_state([rep_prompt[-1]], [len(rep_prompt) - 1])
    model.step_counter.zero_()
    t0 = time.perf_counter()
    for _ in range(a.new):
        model.decode_step(1)
    sync()
    rep_plain_s = time.perf_counter() - t0
    rep_plain = model.tokens_out[0, :a.new].cpu().numpy().tolist()
    res["ngram"] = {"plain_tok_s": a.new / rep_plain_s, **{k: spec_leg(speculative.NGramProposer(3, k), k, rep_prompt, rep_plain) for k in (2, 4, 7)}}
    print(json.dumps(res))
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(markdown(res))
    return 0


def markdown(r):
    L = [f"Model: {r['model']}, prompt {r['prompt_len']}, {r['new_tokens']} new tokens per leg.", "",
         "| step | ms |", "|---|---|",
         f"| batch-1 step, eager (`decode_step`; the host loop's `set_state` cost of {r['set_state_ms']:.3f} ms subtracted) | {r['decode_step_ms']:.3f} |",
         f"| batch-1 step, eager loop end to end | {r['eager_batch1_ms']:.3f} ({r['eager_batch1_tok_s']:.1f} tok/s) |",
         f"| batch-1 step, captured graph replay (what `bench.py` times) | {r['graph_replay_ms']:.3f} ({1e3 / r['graph_replay_ms']:.1f} tok/s) |"]
    for rows in sorted(r["verify_step_ms"], key=int):
        L.append(f"| verify step, {rows} rows + verifier and advance | {r['verify_step_ms'][rows]:.3f} + {r['verifier_ms'][rows]:.3f}; break-even "
                 f"{r['break_even_extra_tokens'][rows]:.2f} extra tokens per round |")
    L += ["", "| replay proposer, planted acceptance | n_draft 1 | 2 | 4 | 7 |", "|---|---|---|---|---|"]
    for label, legs in r["replay"].items():
        cell = lambda g: f"{g['tok_s']:.1f} tok/s ({g['accepted']}/{g['proposed']} accepted, {g['rounds']} rounds{'' if g['lossless'] else ', IDS DIFFER'})"
        L.append(f"| {label} | " + " | ".join(cell(legs[k]) for k in sorted(legs, key=int)) + " |")
    ng = r["ngram"]
    L += ["", f"`NGramProposer(3, k)` on a repetitive prompt (plain eager run of the same prompt: {ng['plain_tok_s']:.1f} tok/s): " +
          ", ".join(f"k = {k}: {g['tok_s']:.1f} tok/s ({g['accepted']}/{g['proposed']} accepted{'' if g['lossless'] else ', IDS DIFFER'})" for k, g in ng.items() if k != "plain_tok_s"), ""]
    return "\n".join(L)


if __name__ == "__main__":
    sys.exit(main())
