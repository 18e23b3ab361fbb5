#!/usr/bin/env python3
"""Golden vectors for autoregressive speech-token generation (TransformerLM.inference / forward_chunk).

Runs the REFERENCE's own ``TransformerLM.inference`` and ``BaseEncoder.forward_chunk`` on the CPU, with the
builders and import shims of ``tools/make_golden.py``.  Deterministic: the sampler is
``partial(ras_sampling, top_k=1, tau_r=1e9)`` (greedy -- nucleus with one candidate, the RAS fallback never fires).
Weights come from ``oracle.detweights`` and are not stored.  A case is only accepted when every step's top-2 margin
of the log-probabilities is >= 1e-3, so that fp32 token equality is a fair assertion on the device.

usage: python tools/make_golden_decode.py [--only tiny|full|joint]
"""
import argparse
import json
import os
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import numpy as np  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tools.make_golden import (FLOW_TARGETS, FULL_LLM, GOLD, LLM_TARGETS, TINY_FLOW, TINY_LLM, build_ref_flow,  # noqa: E402
                               build_ref_llm, npz_save, wrap_and_fill)
from cosyvoice.utils.common import ras_sampling  # noqa: E402

MARGIN = 1e-3
GREEDY = partial(ras_sampling, top_k=1, tau_r=1e9)


def build(c, r, alpha, seed):
    torch.manual_seed(0)
    llm = build_ref_llm(c)
    wrap_and_fill(llm, r=r, alpha=alpha, targets=LLM_TARGETS, seed=seed)
    llm.sampling = GREEDY
    return llm.eval()


def greedy_run(llm, text, ptext, ptok, emb, max_ratio=20.0, min_ratio=2.0):
    """-> (tokens, logp rows [steps, V] (before the step-0 EOS mask), top-2 margins, error message or '')."""
    rows = []
    h = llm.llm_decoder.register_forward_hook(lambda mod, i, o: rows.append(o.detach()[0].log_softmax(-1).clone()))
    toks, err = [], ""
    try:
        for t in llm.inference(text, torch.tensor([text.shape[1]]), ptext, torch.tensor([ptext.shape[1]]), ptok,
                               torch.tensor([ptok.shape[1]]), emb, max_token_text_ratio=max_ratio,
                               min_token_text_ratio=min_ratio):
            toks.append(int(t))
    except RuntimeError as e:
        err = str(e)
    finally:
        h.remove()
    lp = torch.stack(rows).reshape(len(rows), -1)
    eos = llm.speech_token_size
    margins = []
    for i, r in enumerate(lp):
        r = r.clone()
        if i == 0:
            r[eos] = -float('inf')
        v = r.topk(2).values
        margins.append(float(v[0] - v[1]))
    return toks, lp, margins, err


def gen_tiny():
    c = TINY_LLM
    llm = build(c, 4, 8, 5)
    d, V = c['d'], c['speech_vocab'] + 1
    arr, meta = {}, dict(build=c, lora=dict(r=4, alpha=8, targets=LLM_TARGETS), weight_seed=5, margin=MARGIN)

    # forward_chunk: a 23-row prefill then 5 one-row steps, full cache kept
    g = torch.Generator().manual_seed(101)
    xs = [torch.randn(1, 23, d, generator=g)] + [torch.randn(1, 1, d, generator=g) for _ in range(5)]
    cache, cnn = torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0)
    off = 0
    with torch.no_grad():
        for i, x in enumerate(xs):
            T = x.shape[1]
            y, cache, cnn = llm.llm.forward_chunk(x, offset=off, required_cache_size=-1, att_cache=cache, cnn_cache=cnn,
                                                  att_mask=torch.tril(torch.ones(1, T, T)).to(torch.bool))
            off += T
            arr[f"fc_x{i}"], arr[f"fc_y{i}"] = x, y
            if i in (0, len(xs) - 1):
                arr[f"fc_cache{i}"] = cache
    meta['fc_steps'] = len(xs)
    meta['fc_cnn_shape'] = list(cnn.shape)

    # greedy inference cases
    cases = {}
    for seed in range(200, 400):
        g = torch.Generator().manual_seed(seed)
        text = torch.randint(0, c['text_vocab'], (1, 4), generator=g)
        zt, zs = torch.zeros(1, 0, dtype=torch.long), torch.zeros(1, 0, dtype=torch.long)
        toks, lp, mg, err = greedy_run(llm, text, zt, zs, torch.zeros(1, 192))
        if err or min(mg) < MARGIN or len(toks) < 8:
            continue
        cases['i'] = dict(seed=seed, text=text, ptext=zt, ptok=zs, emb=torch.zeros(1, 192), toks=toks, lp=lp, mg=mg)
        break
    for seed in range(400, 600):
        g = torch.Generator().manual_seed(seed)
        text = torch.randint(0, c['text_vocab'], (1, 4), generator=g)
        ptext = torch.randint(0, c['text_vocab'], (1, 3), generator=g)
        ptok = torch.randint(0, c['speech_vocab'], (1, 5), generator=g)
        emb = torch.randn(1, 192, generator=g)
        toks, lp, mg, err = greedy_run(llm, text, ptext, ptok, emb)
        if err or min(mg) < MARGIN or len(toks) < 8:
            continue
        cases['ii'] = dict(seed=seed, text=text, ptext=ptext, ptok=ptok, emb=emb, toks=toks, lp=lp, mg=mg)
        break
    # (iii) EOS made the argmax (decoder bias) -> refused before min_len -> RuntimeError after 100 re-draws
    bump = 40.0
    with torch.no_grad():
        llm.llm_decoder.bias[c['speech_vocab']] += bump
    text = cases['i']['text']
    zt = torch.zeros(1, 0, dtype=torch.long)
    toks, lp, mg, err = greedy_run(llm, text, zt, zt, torch.zeros(1, 192))
    assert err.startswith('sampling reaches max_trials'), err
    with torch.no_grad():
        llm.llm_decoder.bias[c['speech_vocab']] -= bump
    cases['iii'] = dict(seed=cases['i']['seed'], text=text, ptext=zt, ptok=zt, emb=torch.zeros(1, 192), toks=toks, lp=lp,
                        mg=mg)
    meta['eos_bias_bump'] = bump
    meta['error'] = err
    for k, cs in cases.items():
        assert cs['lp'].shape[1] == V
        print(f"tiny case {k}: seed {cs['seed']} tokens {len(cs['toks'])} min margin {min(cs['mg']):.4g}")
        for f in ('text', 'ptext', 'ptok', 'emb', 'lp'):
            arr[f"{k}_{f}"] = cs[f]
        arr[f"{k}_tokens"] = torch.tensor(cs['toks'], dtype=torch.int64)
        meta[f"case_{k}"] = dict(seed=cs['seed'], n_tokens=len(cs['toks']), min_margin=min(cs['mg']))
    npz_save(os.path.join(GOLD, "llm_decode_tiny.npz"), **arr)
    with open(os.path.join(GOLD, "llm_decode_meta.json"), "w") as f:
        json.dump(dict(tiny=meta), f, indent=1)


def gen_full():
    """Full-size (det weights, LoRA folded by the reference's LoRA forward): 32 greedy steps from a 40-token text.  Only
    tokens, logp[token], the top-8 values and the logsumexp of the raw logits per step are kept."""
    c = FULL_LLM
    llm = build(c, 8, 16, 7)
    logits = []
    h = llm.llm_decoder.register_forward_hook(lambda mod, i, o: logits.append(o.detach().reshape(-1).clone()))
    g = torch.Generator().manual_seed(900)
    text = torch.randint(0, c['text_vocab'], (1, 40), generator=g)
    zt = torch.zeros(1, 0, dtype=torch.long)
    toks, lp, mg, err = greedy_run(llm, text, zt, zt, torch.zeros(1, 192), max_ratio=0.8, min_ratio=0.0)
    h.remove()
    assert not err and len(toks) == 32, (err, len(toks))
    assert min(mg) >= MARGIN, min(mg)
    lse = torch.stack([x.logsumexp(-1) for x in logits])[:32]
    lp = lp[:32]
    ids = torch.tensor(toks, dtype=torch.int64)
    npz_save(os.path.join(GOLD, "llm_decode_full.npz"), text=text, tokens=ids, logp_tok=lp.gather(1, ids[:, None])[:, 0],
             top8=lp.topk(8, dim=1).values, lse=lse)
    mpath = os.path.join(GOLD, "llm_decode_meta.json")
    meta = json.load(open(mpath))
    meta['full'] = dict(lora=dict(r=8, alpha=16, targets=LLM_TARGETS), weight_seed=7, steps=32, min_margin=min(mg))
    with open(mpath, "w") as f:
        json.dump(meta, f, indent=1)
    print(f"full: tokens {toks[:8]}... min margin {min(mg):.4g}")


def gen_joint():
    """The no-prompt joint path of inference_joint.py on the tiny models: the greedy LLM tokens of tiny case (i) ->
    the reference's flow.inference (empty prompt, zero embedding, initial noise pinned as gen_inference does) ->
    mel * MEL_STD + MEL_MEAN, and that mel stretched by F.interpolate for speed 0.8."""
    from config import MEL_MEAN, MEL_STD
    tiny = dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz")))
    tokens = torch.from_numpy(tiny["i_tokens"]).reshape(1, -1)
    torch.manual_seed(0)
    flow = build_ref_flow('vendored', **TINY_FLOW)
    wrap_and_fill(flow, r=4, alpha=8, targets=FLOW_TARGETS, seed=3)
    flow.eval()
    n = tokens.shape[1]
    T = int(n / 50 * 22050 / 256)
    z = torch.randn(1, 80, T, generator=torch.Generator().manual_seed(61))
    orig = torch.randn_like
    torch.randn_like = lambda t, *a, **k: z.clone().to(t.dtype)
    try:
        with torch.no_grad():
            mel, _ = flow.inference(tokens, torch.tensor([n]), torch.zeros(1, 0, dtype=torch.long), torch.tensor([0]),
                                    torch.zeros(1, 0, 80), torch.tensor([0]), torch.zeros(1, 192))
    finally:
        torch.randn_like = orig
    mel = mel * MEL_STD + MEL_MEAN
    slow = F.interpolate(mel, size=int(mel.shape[2] / 0.8), mode='linear')
    print(f"joint: {n} tokens -> mel {tuple(mel.shape)}, speed 0.8 -> {tuple(slow.shape)}")
    npz_save(os.path.join(GOLD, "llm_decode_joint.npz"), tokens=tokens, z=z, mel=mel, mel_speed08=slow)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all")
    a = ap.parse_args()
    torch.set_num_threads(8)
    if a.only in ("all", "tiny"):
        gen_tiny()
    if a.only in ("all", "full"):
        gen_full()
    if a.only in ("all", "joint"):
        gen_joint()
