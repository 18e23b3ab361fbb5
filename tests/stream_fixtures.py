"""Shared by tools/make_golden_stream.py, which writes tests/golden/stream_*.npz, and the streaming tests: the cases, how
their inputs and random draws are rebuilt, and a host restatement of the two stitches of the reference's token2wav."""
import math

import numpy as np
import torch

HOP = 30                     # token_min_hop_len = token_max_hop_len of the fixtures
OVERLAP = 20                 # token_overlap_len: the mel overlap stays 34, the length the Flow's cache hard-codes
MEL_OVERLAP, MEL_CACHE, SOURCE_CACHE = 34, 20, 5120
SPEECH_STRIDE = 16           # the vocoder's speech before the stitch is stored every 16th sample

# windows: what CosyVoiceModel.tts cuts out of the token list at hop 30, overlap 20
CASES = {
    "noprompt": dict(n_tokens=130, prompt_frames=0, prompt_tokens=0, seed=611, input_seed=71,
                     windows=[(0, 50, False), (30, 80, False), (60, 110, False), (90, 130, True)]),
    "prompt": dict(n_tokens=100, prompt_frames=40, prompt_tokens=12, seed=612, input_seed=72,
                   windows=[(0, 50, False), (30, 80, False), (60, 100, True)]),
}


def make_inputs(case: dict, vocab: int = 64):
    """(tokens [1, n], prompt tokens [1, p], prompt log-mel [1, frames, 80] (not normalised), embedding [1, 192])"""
    g = torch.Generator().manual_seed(case["input_seed"])
    tokens = torch.randint(0, vocab, (1, case["n_tokens"]), generator=g)
    ptok = torch.randint(0, vocab, (1, case["prompt_tokens"]), generator=g)
    pfeat = torch.randn(1, case["prompt_frames"], 80, generator=g) * 1.5 - 6.0
    emb = torch.randn(1, 192, generator=g)
    return tokens, ptok, pfeat, emb


def redraw(seed: int, plan):
    """The reference's draws of one streamed request seeded with torch.manual_seed(seed), in order.  plan: one
    (kind, shape) per draw, kind 'randn' (torch.randn_like) or 'uniform' (Uniform(-pi, pi).sample)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for kind, shape in plan:
        if kind == "randn":
            out.append(torch.randn(tuple(shape), generator=g))
        else:
            out.append(-math.pi + torch.rand(tuple(shape), generator=g) * (math.pi - -math.pi))
    return out


def chunk_draws(draws, plan_per_chunk):
    """split the flat list of redraw() by chunk: [(flow noise, (phase, source noise)), ...].  Per chunk the reference draws
    the Flow's z, the source's phase, its noise, and one more tensor that it never uses."""
    out, i = [], 0
    for n in plan_per_chunk:
        d = draws[i:i + n]
        out.append((d[0], (d[1], d[2])))
        i += n
    return out


def fade_ref(fade_in: torch.Tensor, fade_out: torch.Tensor, window: np.ndarray) -> torch.Tensor:
    """cosyvoice/utils/common.py fade_in_out: fp32 tensors times an fp64 window, summed in fp64, stored as fp32."""
    n = window.shape[0] // 2
    w = torch.from_numpy(window)
    out = fade_in.clone()
    out[..., :n] = (fade_in[..., :n].double() * w[:n] + fade_out[..., -n:].double() * w[n:]).float()
    return out


def mel_stitch_ref(x, trim, ov, window, prev=None, cache=None, finalize=False, scale_shift=None, cache_len=0):
    """token2wav lines 186-204 and 208 on host tensors: x [80, Tn] -> (vocoder input, new overlap, new cached mel, mask
    of the vocoder-input / overlap columns that went through the fade)."""
    y = x[:, trim:].clone()
    if scale_shift is not None:
        y = y * scale_shift[0] + scale_shift[1]
    faded = torch.zeros(y.shape[1], dtype=torch.bool)
    if prev is not None:
        y = fade_ref(y, prev, window)
        faded[:ov] = True
    mc = 0 if cache is None else cache.shape[1]
    cat = y if cache is None else torch.cat([cache, y], dim=1)
    faded = torch.cat([torch.zeros(mc, dtype=torch.bool), faded])
    if finalize:
        return cat, None, None, faded
    out = cat[:, :cat.shape[1] - ov]
    return out, cat[:, cat.shape[1] - ov:], (out[:, -cache_len:] if cache_len else None), faded


def wav_stitch_ref(speech, sc, window, cache=None, finalize=False):
    """token2wav lines 206-211 / 217-218: speech [N] -> (emitted, new speech cache)."""
    y = fade_ref(speech, cache, window) if cache is not None else speech.clone()
    if finalize:
        return y, None
    return y[:y.shape[0] - sc], y[y.shape[0] - sc:]
