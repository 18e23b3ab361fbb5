#!/usr/bin/env python3
"""Continuous batching of the full-size TransformerLM (random weights, bf16): TransformerLM.decode_server in both prefill
modes against inference_batch in lockstep groups.

(a) throughput: 32 requests, all there at t = 0, 300 prompt rows each (text + prompt speech tokens), token counts fixed
    (min = max ratio 2 over a text of half that length) from TOKENS below; the server with rows = 8 in the stall mode
    (prefill_rows = 0) and the piggyback mode (--prefill-rows), and inference_batch over the same requests in
    arrival-order groups of 8 (the path as it was before the server).  Wall time from the first submit to the last
    token, tokens/s; --repeats times each.
(b) admission: 7 requests of 400 tokens are decoding, one more 300-row request is submitted after step 50: the largest
    gap between consecutive tokens of the running rows (the host's clock after each step's read) and the newcomer's
    time from submit to first token, in both modes.

usage: python tools/bench_serve.py [--repeats 3] [--prefill-rows 8] [--out profiles/serve_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cosyvoice_lora_finetune_framework_amd.llm_model import build_llm_model  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.modules import Numerics  # noqa: E402

ROWS = 8
N_BODY = 297                  # text + prompt speech tokens; + sos, speaker embedding, task id = 300 prompt rows
RATIO = dict(min_token_text_ratio=2, max_token_text_ratio=2)       # a text of n tokens decodes exactly 2 n speech tokens
# tokens per request, in arrival order (100 .. 400, mean 250)
TOKENS = [310, 120, 400, 180, 260, 100, 350, 220, 140, 390, 280, 200, 330, 160, 240, 370,
          110, 300, 190, 400, 230, 150, 360, 270, 100, 320, 210, 380, 170, 290, 130, 340]


def request(g, dev, lm, ntok):
    """(text, embedding, prompt speech tokens) of a request with 300 prompt rows that decodes ntok tokens."""
    n = ntok // 2
    return (torch.randint(0, lm.text_embedding.num_embeddings, (n,), generator=g).to(dev),
            torch.randn(1, 192, generator=g).to(dev),
            torch.randint(0, lm.speech_token_size, (N_BODY - n,), generator=g).to(dev))


def submit(srv, q, seed):
    return srv.submit(q[0], embedding=q[1], prompt_speech_token=q[2], seed=seed, **RATIO)


def warm(srv, reqs):
    submit(srv, (reqs[0][0][:6], reqs[0][1], reqs[0][2]), 1)
    submit(srv, (reqs[1][0][:3], reqs[1][1], reqs[1][2]), 2)
    srv.run()


def throughput_server(lm, reqs, prefill_rows, repeats):
    srv = lm.decode_server(rows=ROWS, max_cache=N_BODY + 3 + max(TOKENS), prefill_rows=prefill_rows)
    warm(srv, reqs)
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, q in enumerate(reqs):
            submit(srv, q, 100 + i)
        steps = 0
        while srv.pending():
            srv.step()
            steps += 1
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        out = srv.run()
        n = sum(len(v) for v in out.values())
        assert n == sum(TOKENS), (n, sum(TOKENS))
        runs.append(dict(wall_s=round(wall, 4), steps=steps, tokens=n, tokens_per_s=round(n / wall, 1)))
    return runs


def throughput_lockstep(lm, reqs, repeats):
    runs = []
    for rep in range(repeats + 1):                  # (the first pass captures the groups' graphs: not reported)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for g0 in range(0, len(reqs), ROWS):
            idx = range(g0, min(g0 + ROWS, len(reqs)))
            outs = lm.inference_batch([reqs[i][0] for i in idx], embeddings=[reqs[i][1] for i in idx],
                                      prompt_speech_tokens=[reqs[i][2] for i in idx], seeds=[100 + i for i in idx], **RATIO)
            assert [len(o) for o in outs] == [TOKENS[i] for i in idx]
            n += sum(len(o) for o in outs)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if rep:
            runs.append(dict(wall_s=round(wall, 4), tokens=n, tokens_per_s=round(n / wall, 1)))
    return runs


def admission(lm, reqs, long_reqs, prefill_rows):
    srv = lm.decode_server(rows=ROWS, max_cache=N_BODY + 3 + 400, prefill_rows=prefill_rows)
    warm(srv, reqs)
    for i, q in enumerate(long_reqs):
        submit(srv, q, 100 + i)
    running = None
    while running is None or len(running) < 7:      # all seven decoding
        running = {rid for rid, _, _ in srv.step()}
    stamps, new, t_submit, ttft = [], None, None, None
    torch.cuda.synchronize()
    for step in range(200):
        if step == 50:
            t_submit = time.perf_counter()
            new = submit(srv, reqs[5], 107)                   # 300 prompt rows, 100 tokens
        ev = srv.step()
        now = time.perf_counter()
        stamps.append(now)
        if new is not None and ttft is None and any(rid == new for rid, _, _ in ev):
            ttft = now - t_submit
    gaps = [b - a for a, b in zip(stamps, stamps[1:])]
    quiet = gaps[:48]
    res = dict(prefill_rows=prefill_rows, step_gap_ms_median_before=round(statistics.median(quiet) * 1e3, 3),
               step_gap_ms_max_before=round(max(quiet) * 1e3, 3), largest_token_gap_ms=round(max(gaps) * 1e3, 3),
               newcomer_ttft_ms=round(ttft * 1e3, 3))
    for rid in list(srv.req):
        srv.cancel(rid)
    return res


def spread(runs):
    v = [r["tokens_per_s"] for r in runs]
    return dict(best=max(v), worst=min(v), median=statistics.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prefill-rows", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "serve_bench.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    lm = build_llm_model(None, "cuda", numerics=Numerics(dtype=torch.bfloat16)).eval()
    lm.sampling = None
    dev = lm.llm_decoder.weight.device
    g = torch.Generator().manual_seed(5)
    reqs = [request(g, dev, lm, n) for n in TOKENS]
    long_reqs = [request(g, dev, lm, 400) for _ in range(7)]
    res = dict(model="TransformerLM full size, random weights, bf16", rows=ROWS, prompt_rows=N_BODY + 3, requests=len(TOKENS),
               tokens=TOKENS, throughput={}, admission=[])
    with torch.no_grad():
        for name, n in (("stall", 0), ("piggyback", a.prefill_rows)):
            runs = throughput_server(lm, reqs, n, a.repeats)
            res["throughput"][name] = dict(prefill_rows=n, runs=runs, **spread(runs))
            print(json.dumps({name: res["throughput"][name]}), flush=True)
            torch.cuda.empty_cache()
        runs = throughput_lockstep(lm, reqs, a.repeats)
        res["throughput"]["inference_batch_groups_of_8"] = dict(runs=runs, **spread(runs))
        print(json.dumps({"inference_batch": res["throughput"]["inference_batch_groups_of_8"]}), flush=True)
        lm.__dict__.get("_cvft_sessions", {}).clear()
        torch.cuda.empty_cache()
        for n in (0, a.prefill_rows):
            res["admission"].append(admission(lm, reqs, long_reqs, n))
            print(json.dumps(res["admission"][-1]), flush=True)
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
