#!/usr/bin/env python3
"""Latency of streaming synthesis (streaming.StreamingSynthesizer.tts) against the non-streaming path, full-size models.

The CosyVoice-300M LLM and Flow (bf16) and the HiFT vocoder (bf16 weights) with deterministic weights (torch.manual_seed(0)
initialisation; the numbers do not depend on what the weights say).  For each speech-token count (about 150 / 500 / 1000:
the count is fixed by min_len = max_len through the token / text ratios, as bench_decode.py fixes its step count) one
process measures
  * stream=True: the time to the first chunk and the total time, and per chunk its arrival time and its audio length;
  * stream=False: the total time,
each the median of --runs runs after --warmup warm-ups, host clock from the call to a synchronised read (.cpu()) of each
chunk's samples.  From the streamed run's own counters: how many decode steps ran while a chunk was being synthesised (the
two streams overlapping) out of all steps, the host time until token2wav has returned (everything enqueued) and the
time the device still needed after that, per chunk.  One JSON line per token count; --out writes the list.

usage: python tools/bench_stream.py [--tokens 150,500,1000] [--runs 5] [--warmup 2] [--out profiles/r10_stream_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cosyvoice_lora_finetune_framework_amd.flow_model import build_flow_model  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.hift import HiFTGenerator  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.llm_model import build_llm_model  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.modules import Numerics  # noqa: E402
from cosyvoice_lora_finetune_framework_amd.streaming import StreamingSynthesizer  # noqa: E402

N_TEXT = 50


def one_run(syn, text, kw, stream: bool):
    """-> (arrival time of every chunk [s], samples of every chunk, the synthesizer's overlap counters)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    arrivals, samples = [], []
    for item in syn.tts(text, stream=stream, seed=3, hift_seed=5, hift_dtype=torch.bfloat16, llm_kw=kw):
        samples.append(item["tts_speech"].cpu().shape[1])          # the synchronised read
        arrivals.append(time.perf_counter() - t0)
    return arrivals, samples, dict(syn.last_timing) if stream else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="150,500,1000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream.py measures on the GPU; none is visible")
    torch.manual_seed(0)
    dev = torch.device("cuda")
    num = Numerics(dtype=torch.bfloat16)
    llm = build_llm_model(None, "cuda", numerics=num).eval()
    flow = build_flow_model(None, "cuda", numerics=num).eval()
    hift = HiFTGenerator().to(dev).eval()
    syn = StreamingSynthesizer(llm, flow, hift)
    text = torch.randint(0, 1000, (N_TEXT,)).tolist()
    med = statistics.median
    res = []
    for n in [int(v) for v in a.tokens.split(",")]:
        ratio = (n + 0.5) / N_TEXT
        kw = dict(min_token_text_ratio=ratio, max_token_text_ratio=ratio)
        plan = syn.chunk_plan(n)
        runs = {True: [], False: []}
        for stream in (True, False):
            for i in range(a.warmup + a.runs):
                r = one_run(syn, text, kw, stream)
                if i >= a.warmup:
                    runs[stream].append(r)
        s_runs, u_runs = runs[True], runs[False]
        assert all(len(r[0]) == len(plan) for r in s_runs) and all(len(r[0]) == 1 for r in u_runs)
        first = med([r[0][0] for r in s_runs])
        total_s = med([r[0][-1] for r in s_runs])
        total_u = med([r[0][-1] for r in u_runs])
        samples = s_runs[0][1]
        arrive = [med([r[0][k] for r in s_runs]) for k in range(len(plan))]
        gaps = [arrive[0]] + [arrive[k] - arrive[k - 1] for k in range(1, len(plan))]
        rtf = [g / (s / 22050.0) for g, s in zip(gaps, samples)]
        during = med([r[2]["tokens_during_synthesis"] for r in s_runs])
        r = dict(tokens=n, chunks=len(plan), audio_s=round(sum(samples) / 22050.0, 2),
                 first_chunk_ms=round(first * 1e3, 1), stream_total_ms=round(total_s * 1e3, 1),
                 unstreamed_total_ms=round(total_u * 1e3, 1), first_chunk_share_of_unstreamed=round(first / total_u, 3),
                 stream_over_unstreamed=round(total_s / total_u, 3),
                 first_chunk_spread_ms=[round(min(x[0][0] for x in s_runs) * 1e3, 1), round(max(x[0][0] for x in s_runs) * 1e3, 1)],
                 chunk_rtf=[round(v, 4) for v in rtf], chunk_rtf_worst=round(max(rtf), 4),
                 decode_steps_during_synthesis=during, decode_steps_share=round(during / n, 3),
                 llm_host_ms=round(med([x[2]["llm_s"] for x in s_runs]) * 1e3, 1),
                 token2wav_enqueue_ms_per_chunk=round(med([x[2]["enqueue_s"] for x in s_runs]) * 1e3 / len(plan), 1),
                 device_behind_host_ms_per_chunk=round(med([x[2]["drain_s"] for x in s_runs]) * 1e3 / len(plan), 2),
                 runs=a.runs, warmup=a.warmup)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
