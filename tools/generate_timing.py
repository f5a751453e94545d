"""Rate of TrainEngine.generate and where a generation step's time goes, on ONE engine in ONE process:
bert-base-uncased encoder / decoder (random weights: the rate does not depend on them), bf16, B sentences, Se latent rows,
max_length positions, greedy, no end token.  Three arms, alternated round by round after one warm-up call each (the warm-up of
the first arm includes the capture of the step):

  graph          generate(graph=True): the captured step replayed max_length - 1 times
  eager          generate(graph=False): the same launches issued one by one
  prefix_decode  what the engine offered before generate(): decode() once per position on the growing prefix, the next token
                 taken from recon_ids[:, -1] and appended on the device (no host read either)

Every call is timed twice: by device events recorded around it on the current stream, and by the host clock around the call and
a device synchronise.  Then: about `--replays` back-to-back replays of the captured step alone (whole passes over the positions)
between two events (ms per step), the node census of the captured step, a sampling arm (graph, temperature 1, a new seed per call: the same captured step), and one
eager call under kvq._ffi.family_profile_begin() -- an event pair around every entry point, the empty pair subtracted -- for
the split of a step between the GEMMs, kvq_gen_attn and the rest.
Prints one JSON document; profiles/generate.md records it.

--num-beams W (> 1) measures TrainEngine.beam_search instead: beam_search on B sentences with W beams, graph
and eager, against generate() on B W sentences in the same run -- the same row count through the same GEMMs, so the difference is
what the selection over W V candidates and the reads through the ancestry table cost; tokens/s counts the B (max_length - 1)
tokens of the best hypotheses.  Then the replay of either captured step alone, the census, and the family split of an eager
beam call.  profiles/beam_search.md records it.

--temperature T (> 0), with --top-k K and / or --top-p P, measures the filtered sampling step instead: the
unfiltered generate(temperature=T) -- the launches of the parent commit -- against generate(top_k=K), generate(top_p=P), both, and
want_scores alone, a new seed per call, in alternating rounds; the replay of the unfiltered and of the filtered captured step alone
(ms per step, the filter state rewritten between the variants: one graph); the census; and kvq_gen_select against
kvq_gen_select_filtered alone on one [B, V] buffer of N(0, 1) logits.  profiles/sampling_filters.md records it.

--reconstruct measures TrainEngine.reconstruct instead: encode + generate of B sentences of S = --se tokens,
max_length S + 1 -- the calls an evaluation would make by hand, and all there is to measure on a commit without reconstruct(), where
the mode times that arm alone -- against reconstruct() with and without a census of 9 factors, in alternating rounds; then
kvq_seq_compare and kvq_seq_compare_accumulate alone on the call's own ids.  The shader clock held across the rounds is recorded
(kvq_clock_probe before and behind them).  profiles/free_running_eval.md records it.

    PYTHONPATH=kindergarten-vq-vae_amd python3 tools/generate_timing.py [--out FILE.json] [--rounds 5] [--batch 256] [--se 32] [--max-length 32]
                                                                         [--num-beams W] [--temperature T] [--top-k K] [--top-p P] [--reconstruct]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kindergarten-vq-vae_amd")]


def beam_timing(a, eng, lat, timed):
    """beam_search on B sentences x W beams against generate() on B W sentences: the same rows, in alternating rounds"""
    import torch

    from kvq import _ffi
    B, SE, L, W = a.batch, a.se, a.max_length, a.num_beams
    prompt = torch.full((B, 1), 101, dtype=torch.int64, device="cuda")
    lat_rows = lat.repeat_interleave(W, dim=0).contiguous()
    prompt_rows = torch.full((B * W, 1), 101, dtype=torch.int64, device="cuda")
    arms = {"beam_graph": lambda: eng.beam_search(lat, L, prompt, W),
            "beam_eager": lambda: eng.beam_search(lat, L, prompt, W, graph=False),
            "generate_same_rows": lambda: eng.generate(lat_rows, L, prompt_rows)}
    res = {"model": a.model, "B": B, "num_beams": W, "rows": B * W, "Se": SE, "max_length": L, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        first = {k: fn() for k, fn in arms.items()}                       # warm-up of every arm (captures included)
        res["graph_equals_eager"] = all(bool(torch.equal(first["beam_graph"][k], first["beam_eager"][k])) for k in ("beam_ids", "beam_scores"))
        res["best_hypotheses_differing_from_greedy"] = int((first["beam_graph"]["ids"] != first["generate_same_rows"]["ids"][::W]).any(1).sum())
        times = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                times[k].append(timed(fn)[0])
        for k, v in times.items():
            ev, ho = sorted(t["event_s"] for t in v), sorted(t["host_s"] for t in v)
            res[k] = dict(event_s_median=ev[len(ev) // 2], event_s_min=ev[0], event_s_max=ev[-1], host_s_median=ho[len(ho) // 2],
                          sentence_tokens_per_s_median=B * (L - 1) / ev[len(ev) // 2], row_tokens_per_s_median=B * W * (L - 1) / ev[len(ev) // 2])
        for name, entry in (("beam", next(iter(eng._beam_cache.values()))), ("generate_same_rows", next(iter(eng._gen_cache.values())))):
            def replay_block(entry=entry):                                 # whole passes over the positions, t back to 0 in front of each
                for _ in range(max(a.replays // (L - 1), 1)):
                    entry["state"][0:1].zero_()
                    for _ in range(L - 1):
                        entry["graph"].replay()
            dt, _ = timed(replay_block)
            res[name + "_graph_replay_ms_per_step"] = 1e3 * dt["event_s"] / (max(a.replays // (L - 1), 1) * (L - 1))
        res["census"] = eng.gen_census()
        eng.beam_search(lat, L, prompt, W)                                 # leaves a valid state behind the replays
        _ffi.family_profile_begin()
        eng.beam_search(lat, L, prompt, W, graph=False)
        ms, n, empty = _ffi.family_profile_end()
        res["beam_eager_family_ms_per_call"] = ms
        res["beam_eager_family_launches_per_call"] = n
        res["empty_event_pair_ms"] = empty
    return res


def filter_timing(a, eng, lat, prompt, timed):
    """generate(temperature) unfiltered against top-k, top-p, both and scores alone; then the selection kernels alone"""
    import torch

    from kvq import nnops
    B, SE, L, T = a.batch, a.se, a.max_length, a.temperature
    K, P = a.top_k or 50, a.top_p if a.top_p < 1.0 else 0.9
    seeds = iter(range(1, 1 << 30))
    variants = {"top_k": dict(top_k=K), "top_p": dict(top_p=P), "top_k_and_top_p": dict(top_k=K, top_p=P)}
    arms = {"unfiltered": lambda: eng.generate(lat, L, prompt, temperature=T, seed=next(seeds))["ids"]}
    for name, kw in variants.items():
        arms[name] = lambda kw=kw: eng.generate(lat, L, prompt, temperature=T, seed=next(seeds), **kw)["ids"]
    arms["scores_alone"] = lambda: eng.generate(lat, L, prompt, temperature=T, seed=next(seeds), want_scores=True)["ids"]
    tokens = B * (L - 1)
    res = {"model": a.model, "B": B, "Se": SE, "max_length": L, "temperature": T, "top_k": K, "top_p": P, "tokens_per_call": tokens,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for fn in arms.values():                                           # warm-up of every arm (the two captures included)
            fn()
        times = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                times[k].append(timed(fn)[0])
        for k, v in times.items():
            ev, ho = sorted(t["event_s"] for t in v), sorted(t["host_s"] for t in v)
            res[k] = dict(event_s_median=ev[len(ev) // 2], event_s_min=ev[0], event_s_max=ev[-1], host_s_median=ho[len(ho) // 2],
                          tokens_per_s_median=tokens / ev[len(ev) // 2], ms_per_step_median=1e3 * ev[len(ev) // 2] / (L - 1))
        res["captured_steps_kept"] = len(eng._gen_cache)                   # two: the unfiltered step and the filtered one
        passes = max(a.replays // (L - 1), 1)
        plain = next(g for k, g in eng._gen_cache.items() if "filtered" not in k)
        filt = next(g for k, g in eng._gen_cache.items() if "filtered" in k)

        def replay_of(entry):
            def block():                                                   # whole passes over the positions, t back to 0 in front of each
                for _ in range(passes):
                    entry["state"][0:1].zero_()
                    for _ in range(L - 1):
                        entry["graph"].replay()
            return block
        reps = {}
        for rnd in range(3):                                               # alternated, the median of three
            eng.generate(lat, L, prompt, temperature=T, seed=5)            # a valid sampling state behind every block
            reps.setdefault("unfiltered", []).append(timed(replay_of(plain))[0]["event_s"])
            for name, kw in list(variants.items()) + [("scores_alone", {})]:
                eng.generate(lat, L, prompt, temperature=T, seed=5, want_scores=True, **kw)
                reps.setdefault(name, []).append(timed(replay_of(filt))[0]["event_s"])
        res["graph_replay_ms_per_step"] = {k: 1e3 * sorted(v)[1] / (passes * (L - 1)) for k, v in reps.items()}
        res["graph_replay_ms_per_step_all"] = {k: [1e3 * x / (passes * (L - 1)) for x in v] for k, v in reps.items()}
        res["census"] = eng.gen_census()
        # ---- the selection kernels alone, on one buffer ----
        V, Vp = eng.V, eng.Vp
        logits = torch.randn((B, Vp), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
        ids = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
        fin, lens = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.full((B,), 4, dtype=torch.int32, device="cuda")
        kept, cut = torch.zeros((B, 4), dtype=torch.int32, device="cuda"), torch.zeros((B, 4), dtype=torch.int32, device="cuda")
        lp = torch.zeros((B, 4), dtype=torch.float32, device="cuda")
        st = nnops.new_gen_state("cuda", 1, 1, 4, None, 0, temperature=T, seed=7)
        n = 200
        kern = {}

        def alone(fn):
            fn()
            return 1e3 * sorted(timed(lambda: [fn() for _ in range(n)])[0]["event_s"] for _ in range(3))[1] / n
        kern["kvq_gen_select"] = alone(lambda: nnops.gen_select(st, logits, V, ids, fin, lens))
        for name, (k, p) in {"off": (0, 1.0), "top_k": (K, 1.0), "top_p": (0, P), "top_k_and_top_p": (K, P)}.items():
            f = nnops.new_gen_filter("cuda", k, p)
            kern["kvq_gen_select_filtered_" + name] = alone(lambda f=f: nnops.gen_select_filtered(st, f, logits, V, ids, fin, lens, None, kept, cut, lp))
        res["selection_kernel_alone_ms"] = kern
        res["selection_kernel_alone_shape"] = dict(B=B, V=V, ld=Vp, dtype="bfloat16", launches_per_timing=n)
    return res


def reconstruct_timing(a, eng, timed):
    """encode + generate by hand against reconstruct() (without and with a census), then the two comparison kernels alone"""
    import torch

    from kvq import nnops
    B, S = a.batch, a.se
    L = S + 1
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(S // 2, S + 1, (B,), generator=g)
    keep = torch.arange(S)[None] < lens[:, None]
    ids = (torch.randint(1000, 30000, (B, S), generator=g) * keep).cuda()
    mask = keep.long().cuda()
    prompt = torch.full((B, 1), 101, dtype=torch.int64, device="cuda")

    def by_hand():
        lat = eng.encode(ids, mask)["z"].reshape(B, S, eng.H)
        return eng.generate(lat, L, prompt)["ids"]
    arms = {"encode_generate": by_hand}
    has = hasattr(eng, "reconstruct")
    if has:
        from kvq.census import ReconstructionCensus
        cards = [2, 3, 2, 3, 2, 4, 4, 3, 5]
        census = ReconstructionCensus(cards)
        labels = torch.stack([torch.randint(0, c, (B,), generator=g) for c in cards], dim=1).cuda()
        arms["reconstruct"] = lambda: eng.reconstruct(ids, mask, 101)["dist"]
        arms["reconstruct_census"] = lambda: eng.reconstruct(ids, mask, 101, slots=census.slots_of(labels), census=census)["dist"]
    res = {"model": a.model, "B": B, "S": S, "max_length": L, "rounds": a.rounds, "has_reconstruct": has, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for fn in arms.values():                                           # warm-up of every arm (the capture included)
            fn()
        times = {k: [] for k in arms}
        p0 = nnops.clock_probe()
        for _ in range(a.rounds):                                          # alternating rounds
            for k, fn in arms.items():
                times[k].append(timed(fn)[0])
        p1 = nnops.clock_probe()
        torch.cuda.synchronize()
        res["shader_clock_mhz_over_the_rounds"] = nnops.clock_mhz(p0, p1)[0]
        for k, v in times.items():
            ev, ho = sorted(t["event_s"] for t in v), sorted(t["host_s"] for t in v)
            res[k] = dict(event_ms_median=1e3 * ev[len(ev) // 2], event_ms_min=1e3 * ev[0], event_ms_max=1e3 * ev[-1],
                          host_ms_median=1e3 * ho[len(ho) // 2], host_ms_min=1e3 * ho[0], host_ms_max=1e3 * ho[-1])
        if has:
            gen = eng.reconstruct(ids, mask, 101, want_ids=True)
            hyp, hyp_len = gen["ids"], gen["lengths"].to(torch.int32)
            ref_len = torch.full((B,), S, dtype=torch.int32, device="cuda")
            out, bad = nnops.seq_compare(hyp, hyp_len, ids, ref_len, hyp_skip=1, Lmax=S)
            slots, n = census.slots_of(labels), 200

            def alone(fn):
                fn()
                return 1e3 * sorted(timed(lambda: [fn() for _ in range(n)])[0]["event_s"] for _ in range(3))[1] / n
            res["kernels_alone_us"] = {
                "kvq_seq_compare": 1e3 * alone(lambda: nnops.seq_compare(hyp, hyp_len, ids, ref_len, hyp_skip=1, Lmax=S, out=out, n_bad=bad)),
                "kvq_seq_compare_accumulate": 1e3 * alone(lambda: nnops.seq_compare_accumulate(out, slots, census.table))}
            res["kernels_alone_shape"] = dict(B=B, n=S, m=S, slot_columns=len(cards) + 1, table_rows=census.R, launches_per_timing=n)
            res["mean_edit_distance_of_the_untrained_model"] = float(gen["dist"].float().mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--se", type=int, default=32)
    ap.add_argument("--max-length", type=int, default=32)
    ap.add_argument("--replays", type=int, default=310)
    ap.add_argument("--model", default="bert-base-uncased")
    ap.add_argument("--num-beams", type=int, default=1)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--reconstruct", action="store_true")
    a = ap.parse_args()
    import torch

    from kvq import _ffi
    from kvq.engine import engine_of
    from models.bagon.Bagon import Bagon
    if not torch.cuda.is_available():
        raise SystemExit("generate_timing.py measures on the GPU: there is no CPU path and no number without one")
    B, SE, L = a.batch, a.se, a.max_length
    torch.manual_seed(0)
    model = Bagon(a.model, a.model, True, compute_dtype=torch.bfloat16).cuda().eval()
    eng = engine_of(model)
    lat = torch.randn((B, SE, eng.H), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda().contiguous()
    prompt = torch.full((B, 1), 101, dtype=torch.int64, device="cuda")
    tokens = B * (L - 1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return dict(host_s=time.perf_counter() - t0, event_s=e0.elapsed_time(e1) * 1e-3), out

    if (a.top_k or a.top_p < 1.0) and not a.temperature > 0:
        raise SystemExit("--top-k / --top-p measure the sampling step: give --temperature T > 0")
    if a.num_beams > 1 or a.temperature > 0 or a.reconstruct:
        res = reconstruct_timing(a, eng, timed) if a.reconstruct else \
            beam_timing(a, eng, lat, timed) if a.num_beams > 1 else filter_timing(a, eng, lat, prompt, timed)
        text = json.dumps(res, indent=1)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return

    def prefix_loop():
        ids = prompt
        for _ in range(L - 1):
            nxt = eng.decode(lat, ids, torch.ones_like(ids))["recon_ids"][:, -1:]
            ids = torch.cat([ids, nxt], 1)
        return ids

    seeds = iter(range(1, 1 << 30))
    arms = {"graph": lambda: eng.generate(lat, L, prompt)["ids"],
            "eager": lambda: eng.generate(lat, L, prompt, graph=False)["ids"],
            "prefix_decode": prefix_loop,
            "graph_sampling_new_seed_per_call": lambda: eng.generate(lat, L, prompt, temperature=1.0, seed=next(seeds))["ids"]}
    res = {"model": a.model, "B": B, "Se": SE, "max_length": L, "tokens_per_call": tokens, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        first = {k: fn() for k, fn in arms.items()}                       # warm-up of every arm (capture included)
        res["graph_equals_eager"] = bool(torch.equal(first["graph"], first["eager"]))
        res["prefix_loop_tokens_differing_from_generate"] = int((first["prefix_decode"] != first["graph"]).sum())
        times = {k: [] for k in arms}
        for _ in range(a.rounds):                                          # alternating rounds
            for k, fn in arms.items():
                times[k].append(timed(fn)[0])
        for k, v in times.items():
            ev, ho = sorted(t["event_s"] for t in v), sorted(t["host_s"] for t in v)
            res[k] = dict(event_s_median=ev[len(ev) // 2], event_s_min=ev[0], event_s_max=ev[-1], host_s_median=ho[len(ho) // 2],
                          host_s_min=ho[0], host_s_max=ho[-1], tokens_per_s_median=tokens / ev[len(ev) // 2])
        res["captured_steps_kept"] = len(eng._gen_cache)                   # one: sampling under new seeds reuses the greedy call's graph
        entry = next(iter(eng._gen_cache.values()))
        eng.generate(lat, L, prompt)                                       # leaves a valid state, prompt and latent projection behind

        def replay_block():                                                # whole passes over the positions: t back to 0 (one fill
            for _ in range(max(a.replays // (L - 1), 1)):                  # kernel per pass), then the L - 1 steps -- a step past the
                entry["state"][0:1].zero_()                                # last position would find t outside its buffers and skip
                for _ in range(L - 1):                                     # the attention and selection work
                    entry["graph"].replay()
        dt, _ = timed(replay_block)
        res["graph_replay_ms_per_step"] = 1e3 * dt["event_s"] / (max(a.replays // (L - 1), 1) * (L - 1))
        res["census"] = eng.gen_census()
        _ffi.family_profile_begin()
        eng.generate(lat, L, prompt, graph=False)
        ms, n, empty = _ffi.family_profile_end()
        res["eager_family_ms_per_call"] = ms
        res["eager_family_launches_per_call"] = n
        res["empty_event_pair_ms"] = empty
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
