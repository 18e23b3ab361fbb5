"""Streaming synthesis, host side (no GPU): the chunk schedule against the reference's own token windows
(tests/golden/stream_meta.json, tools/make_golden_stream.py), the derived constants, and the refusal of a chunk that is too
short to stitch."""
import json
import os
import types

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def synth(**kw):
    from cosyvoice_lora_finetune_framework_amd.streaming import StreamingSynthesizer
    flow = types.SimpleNamespace(input_frame_rate=50, input_embedding=types.SimpleNamespace(weight=torch.zeros(1)))
    return StreamingSynthesizer(None, flow, None, **kw)


def test_chunk_plan_reproduces_the_fixtures_token_windows():
    from stream_fixtures import CASES, HOP, OVERLAP
    meta = json.load(open(os.path.join(GOLD, "stream_meta.json")))
    assert (meta["hop"], meta["overlap"]) == (HOP, OVERLAP)
    s = synth(token_hop_len=HOP, token_max_hop_len=HOP, token_overlap_len=OVERLAP)
    for name, c in meta["cases"].items():
        want = [tuple(w) for w in c["windows"]]
        assert s.chunk_plan(c["n_tokens"]) == want == [tuple(w) for w in CASES[name]["windows"]], name
    assert [w[:2] for w in s.chunk_plan(130)] == [(0, 50), (30, 80), (60, 110), (90, 130)]


def test_chunk_plan_grows_the_hop_by_the_scale_factor():
    """hop 15 -> 30 -> 50 (60 capped at the ceiling), overlap 20: by hand, 200 tokens.  A window needs hop + 20 tokens to
    be left; after it `hop` tokens are dropped: 0-35 (hop 15), 15-65 (30), 45-115 (50), 95-165 (50), then 145-200 is left
    (55 < 70)."""
    s = synth(token_hop_len=15, token_max_hop_len=50, stream_scale_factor=2)
    assert s.chunk_plan(200) == [(0, 35, False), (15, 65, False), (45, 115, False), (95, 165, False), (145, 200, True)]


def test_chunk_plan_edges():
    s = synth(token_hop_len=30, token_max_hop_len=30)
    assert s.chunk_plan(49) == [(0, 49, True)]                       # below hop + overlap: one final chunk
    assert s.chunk_plan(1) == [(0, 1, True)]
    assert s.chunk_plan(50) == [(0, 50, False), (30, 50, True)]      # exactly hop + overlap: a final chunk of `overlap` tokens
    d = synth()
    assert d.chunk_plan(119) == [(0, 119, True)] and d.chunk_plan(120) == [(0, 120, False), (100, 120, True)]


def test_default_constants_are_the_references():
    from cosyvoice_lora_finetune_framework_amd import config
    s = synth()
    assert (s.token_min_hop_len, s.token_max_hop_len, s.token_overlap_len) == (100, 200, 20)
    assert (s.mel_overlap_len, s.mel_cache_len, s.source_cache_len, s.stream_scale_factor) == (34, 20, 5120, 1)
    assert s.mel_window.dtype == np.float64 and np.array_equal(s.mel_window, np.hamming(68))
    assert np.array_equal(s.speech_window, np.hamming(10240))
    n = np.arange(68)
    assert np.allclose(s.mel_window, 0.54 - 0.46 * np.cos(2 * np.pi * n / 67), rtol=0, atol=1e-15)
    assert s.boundary_trim_ratio == config.INFERENCE_CONFIG['boundary_trim_ratio'] == 0.20
    assert synth(boundary_trim_ratio=0.15).boundary_trim_ratio == 0.15
    with pytest.raises(ValueError):
        synth(stream_scale_factor=0.5)
    with pytest.raises(ValueError, match="token_hop_len 10 is too small"):      # 51 frames - 34 = 17 < the 20 cached
        synth(token_hop_len=10)
    assert synth(token_hop_len=12).token_min_hop_len == 12                      # 55 - 34 = 21


def test_a_chunk_shorter_than_the_overlap_is_refused_on_the_host():
    """19 tokens give 32 mel frames, fewer than the 34 of the overlap: refused before anything touches a device (the
    models here are stand-ins that cannot run).  A lone final chunk of that size is an ordinary short utterance."""
    from cosyvoice_lora_finetune_framework_amd.streaming import StreamState
    from cosyvoice_lora_finetune_framework_amd.hipops import functional as HF
    s = synth()
    empty = torch.zeros(1, 0, 80)
    with pytest.raises(ValueError, match=r"19 tokens give 32 mel frames.*overlap of 34"):
        s.token2wav(StreamState(), torch.zeros(1, 19, dtype=torch.long), torch.zeros(1, 0, dtype=torch.long), empty,
                    torch.zeros(1, 192), finalize=False)
    st = StreamState()
    st.mel_overlap = torch.zeros(80, 34)
    with pytest.raises(ValueError, match=r"32 mel frames"):
        s.token2wav(st, torch.zeros(1, 19, dtype=torch.long), torch.zeros(1, 0, dtype=torch.long), empty, torch.zeros(1, 192),
                    finalize=True)
    # the boundary trim counts: 24 tokens give 41 frames, 33 after a trim of int(40 * 0.2) = 8
    with pytest.raises(ValueError, match=r"41 mel frames, 33 after the boundary trim of 8"):
        s.token2wav(StreamState(), torch.zeros(1, 24, dtype=torch.long), torch.zeros(1, 0, dtype=torch.long),
                    torch.zeros(1, 40, 80), torch.zeros(1, 192), finalize=False)
    assert s.check_chunk(19, 0, True, False) == (32, 0)
    # the wrappers make the same check before they look at the device
    with pytest.raises(ValueError, match=r"40 columns - 8 trimmed = 32, below the overlap of 34"):
        HF.stream_mel_stitch(torch.zeros(80, 40), 8, 34, torch.zeros(68))
    with pytest.raises(ValueError, match=r"5119 samples, below the cache of 5120"):
        HF.stream_wav_stitch(torch.zeros(5119), 5120, torch.zeros(10240))
