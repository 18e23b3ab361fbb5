"""Host logic of autoregressive generation (no GPU): the reference-signature samplers of utils.py on hand-built score
vectors, and how TransformerLM picks the device sampler's parameters from ``self.sampling``."""
import functools
import math

import torch

from cosyvoice_lora_finetune_framework_amd import utils as U
from cosyvoice_lora_finetune_framework_amd.decode import SamplerCfg


def _scores(probs):
    return torch.tensor(probs, dtype=torch.float32).log()


def _support(fn, scores, n=400, **kw):
    torch.manual_seed(0)
    return sorted({int(fn(scores, **kw)) for _ in range(n)})


def test_nucleus_includes_the_token_that_crosses_top_p():
    s = _scores([0.5, 0.25, 0.15, 0.1])
    # cum before each candidate: 0, .5, .75 (< .8 -> the third is taken), .9 (stop)
    assert _support(U.nucleus_sampling, s, top_p=0.8, top_k=25) == [0, 1, 2]
    assert _support(U.nucleus_sampling, s, top_p=0.5, top_k=25) == [0]
    assert _support(U.nucleus_sampling, s, top_p=0.51, top_k=25) == [0, 1]


def test_nucleus_top_k_caps_the_candidates():
    s = _scores([0.1] * 10)
    assert _support(U.nucleus_sampling, s, top_p=0.99, top_k=3) == [0, 1, 2]


def test_nucleus_stable_ties_prefer_lower_ids():
    s = _scores([0.1, 0.3, 0.1, 0.3, 0.1, 0.1])
    # descending, stable: 1, 3, 0, 2, 4, 5 -> top_k=3 keeps 1, 3 and the LOWEST-id of the tied 0.1s
    assert _support(U.nucleus_sampling, s, top_p=0.99, top_k=3) == [0, 1, 3]
    assert _support(U.nucleus_sampling, s, top_p=0.99, top_k=1) == [1]


def test_nucleus_greedy_is_argmax():
    torch.manual_seed(1)
    s = torch.randn(4097).log_softmax(0)
    assert int(U.nucleus_sampling(s, top_p=0.8, top_k=1)) == int(s.argmax())


def test_ras_falls_back_to_the_full_softmax_on_repeats():
    s = _scores([0.7, 0.2, 0.05, 0.05])
    # greedy nucleus (top_k=1) always draws 0; token 0 is in the window -> full-softmax draw, which reaches 2 and 3
    got = _support(U.ras_sampling, s, decoded_tokens=[3, 0, 1], sampling=25, top_k=1, win_size=10, tau_r=0.1)
    assert got == [0, 1, 2, 3]
    # not in the window -> plain nucleus
    assert _support(U.ras_sampling, s, decoded_tokens=[1, 2], sampling=25, top_k=1, win_size=10, tau_r=0.1) == [0]
    # only the last win_size tokens count
    assert _support(U.ras_sampling, s, decoded_tokens=[0, 1, 1], sampling=25, top_k=1, win_size=2, tau_r=0.5) == [0]
    # tau_r huge: never falls back
    assert _support(U.ras_sampling, s, decoded_tokens=[0] * 10, sampling=25, top_k=1, tau_r=1e9) == [0]


def test_random_sampling_covers_the_softmax():
    s = _scores([0.25, 0.25, 0.25, 0.25])
    assert _support(U.random_sampling, s, decoded_tokens=[], sampling=25) == [0, 1, 2, 3]


def test_rep_threshold_matches_the_float_comparison():
    for win, tau in [(10, 0.1), (10, 0.25), (7, 0.3), (10, 1e9), (10, 0.0), (3, 1.0)]:
        cfg = SamplerCfg("ras", win_size=win, tau_r=tau)
        for rep in range(0, win + 1):
            assert (rep >= cfg.rep_thr) == (rep >= win * tau), (win, tau, rep)


def test_sampler_cfg_dispatch():
    from cosyvoice_lora_finetune_framework_amd.llm_model import TransformerLM

    class _LM:
        sampling = None
        sampler_cfg = TransformerLM.sampler_cfg

    m = _LM()
    c = m.sampler_cfg()
    assert (c.mode, c.top_p, c.top_k, c.win) == ("ras", 0.8, 25, 10)
    m.sampling = functools.partial(U.ras_sampling, top_p=0.9, top_k=7, win_size=12, tau_r=0.2)
    c = m.sampler_cfg()
    assert (c.mode, c.top_p, c.top_k, c.win, c.rep_thr) == ("ras", 0.9, 7, 12, math.ceil(12 * 0.2))
    m.sampling = functools.partial(U.nucleus_sampling, top_k=3)
    assert m.sampler_cfg().mode == "nucleus"
    m.sampling = functools.partial(U.random_sampling)
    assert m.sampler_cfg().mode == "random"
    for host in (functools.partial(U.ras_sampling, top_k=100), lambda s, d, n: s.argmax(), U.ras_sampling):
        m.sampling = host
        assert m.sampler_cfg() is None
