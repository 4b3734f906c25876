"""Cost of guided decoding: the constrained pre-pass entry (must not move), the guided entry with no, one and every slot guided
(a 200-state guide, about 50 k allowed tokens per state) at T = 4 / 16 / 192 (V = 128256), the in-flight walk at its deepest
rows; build time and bytes of that guide; and the constrained cycle against the guided cycle with 0 / 1 / 4 guided requests
(Llama-3-8B synthetic weights, bs = 4, k = 3).
Medians of 15 rounds of 20 launches, one JSON line.  Usage: python scripts/bench_guided.py [--no-cycle] [--constrained-only]
(--constrained-only: what a build without the guided entry can run, for the before / after comparison)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qspec_amd import ops  # noqa: E402

DEV, V = "cuda:0", 128256


def med_us(fn, rounds=15, inner=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / inner)
    return round(float(np.median(out)), 2)


def big_guide(rs, n_states=200, per_state=50000):
    """n_states states of about per_state allowed tokens with random next states, the final state behind them."""
    from qspec_amd.spec_decode.guides import TokenFSM
    eos = V - 1
    row_ptr, toks, nxt = [0], [], []
    for _ in range(n_states):
        t = np.union1d(rs.choice(V - 1, per_state, replace=False), [eos])
        n = rs.integers(0, n_states, len(t))
        n[-1] = n_states
        toks.append(t); nxt.append(n); row_ptr.append(row_ptr[-1] + len(t))
    toks.append(np.array([eos])); nxt.append(np.array([n_states])); row_ptr.append(row_ptr[-1] + 1)
    return TokenFSM(row_ptr, np.concatenate(toks), np.concatenate(nxt), 0, n_states, V, eos)


def main():
    res = {}
    constrained_only = "--constrained-only" in sys.argv
    g = torch.Generator(device=DEV).manual_seed(1)
    rs = np.random.default_rng(0)
    fsm = None if constrained_only else big_guide(rs)
    for T in (4, 16, 192):
        B = max(1, T // 4)
        lg = (torch.randn(T, V, device=DEV, generator=g) * 3).half()
        out = torch.empty_like(lg)
        table, counted = ops.new_logit_table(B, V, DEV)
        table.random_(0, 3)
        i32 = dict(dtype=torch.int32, device=DEV)
        drafts = torch.zeros(3, B, dtype=torch.int64, device=DEV)
        a = dict(tok_table=table, repetition=torch.full((B,), 1.2, dtype=torch.float16, device=DEV),
                 frequency=torch.full((B,), 0.1, dtype=torch.float16, device=DEV),
                 presence=torch.full((B,), 0.5, dtype=torch.float16, device=DEV), min_tokens=torch.zeros(B, **i32),
                 gen_base=torch.zeros(B, **i32), gen_lens=torch.full((B,), 40, **i32), stop_ids=torch.zeros(B, 16, **i32),
                 num_stop_ids=torch.zeros(B, **i32), draft_ids=drafts)
        gen = torch.randint(0, V, (B, 64), dtype=torch.int64, device=DEV)
        tc = ops.TokenConstraints(B, V, DEV)
        cons = dict(deny=tc.deny, meta=tc.meta, bias_ids=tc.bias_ids, bias_vals=tc.bias_vals, words=tc.words, word_lens=tc.word_lens,
                    tail=tc.tail, gen_tokens=gen)
        res[f"prepass_constrained_none_T{T}_us"] = med_us(lambda: ops.process_logits_constrained(lg, out, rows_per_seq=4, j_base=0,
                                                                                                  **cons, **a))
        if constrained_only:
            continue
        tg = ops.TokenGuides(B, V, DEV, fsm.num_states, fsm.num_transitions)
        if T == 4:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.guide_build(tg, 0, 0, fsm.row_ptr, fsm.tokens, fsm.next_states)
            torch.cuda.synchronize()
            res["guide_build_with_upload_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            up = [torch.from_numpy(x).to(DEV) for x in (fsm.row_ptr, fsm.tokens, fsm.next_states)]
            res["guide_build_kernel_us"] = med_us(lambda: ops._call(
                "qspec_guide_build", tg.allow.data_ptr(), tg.rank.data_ptr(), tg.off.data_ptr(), tg.nxt.data_ptr(), tg.words, tg.words,
                V, tg.max_states, tg.max_transitions, 0, 0, fsm.num_states, fsm.num_transitions, up[0].data_ptr(), up[1].data_ptr(),
                up[2].data_ptr(), ops._stream()), rounds=5, inner=3)
            res["guide_bytes"] = int(fsm.num_states * tg.words * 8 + fsm.num_states * 4 + fsm.num_transitions * 4)
        else:
            ops.guide_build(tg, 0, 0, fsm.row_ptr, fsm.tokens, fsm.next_states)
        # in-flight tokens the guide allows, so the walks run their full length (3 steps for the last row of a sequence)
        s, walk = 0, []
        for _ in range(3):
            t = int(fsm.allowed(s)[7])
            walk.append(t); s = fsm.next(s, t)
        drafts.copy_(torch.tensor(walk, dtype=torch.int64).view(3, 1).expand(3, B))
        for name, slots in (("none", []), ("one", [0]), ("all", list(range(B)))):
            tg.gslot.zero_()
            for b in slots:
                tg.set_slot(b, 0, fsm.miss, guided=True)
            arrays = dict(zip(("guide_allow", "guide_rank", "guide_off", "guide_next", "guide_slots"), tg.arrays()))
            res[f"prepass_guided_{name}_T{T}_us"] = med_us(lambda: ops.process_logits_guided(lg, out, rows_per_seq=4, j_base=0, **cons,
                                                                                              **arrays, **a))
        del tg
    if "--no-cycle" not in sys.argv:
        from qspec_amd.model import CONFIGS, QuarotLlamaForCausalLM
        from qspec_amd.spec_decode import QSpecEngine
        model = QuarotLlamaForCausalLM(CONFIGS["llama-3-8b"], DEV).init_synthetic(seed=0)
        cons = dict(temperature=0.8, repetition_penalty=1.2, min_p=0.05, logit_bias={t: 0.5 for t in range(1000, 1512)},
                    allowed_token_ids=list(range(0, V, 2)))
        variants = [("constrained", [cons] * 4)]
        if not constrained_only:
            variants += [("guided_one", [dict(cons, guide=fsm)] + [cons] * 3), ("guided_all", [dict(cons, guide=fsm)] * 4)]
        for name, kws in variants:
            eng = QSpecEngine(model, 3, 4, max_model_len=1024, block_size=16, max_new_tokens=900, use_graph=True,
                              **({} if constrained_only else dict(guide_states=256, guide_transitions=fsm.num_transitions + 16)))
            for b in range(4):
                eng.set_sampling_params(b, **kws[b])
            eng.add_sequences_to([0, 1, 2, 3], [rs.integers(0, V, 512).tolist() for _ in range(4)])
            eng.step()
            res[f"cycle_{name}_ms"] = round(med_us(eng.step, rounds=15, inner=5) / 1000.0, 4)
            del eng
    print(json.dumps(res))


if __name__ == "__main__":
    main()
