"""How the HiFT fixtures' weights and random draws are rebuilt (tests/golden/hift_*.npz): shared by
tools/make_golden_hift.py, which writes the fixtures, and tests/test_hift_gpu.py, which feeds the device the same."""
import math

import torch

from oracle.detweights import det_state_dict

WEIGHT_SEED = 21
POST_SCALE = 0.05           # conv_post g: keeps exp() of its output well below the 1e2 clip


def make_mel(T: int, mel_seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(mel_seed)
    return (torch.randn(1, 80, T, generator=g) * 1.5 - 3.0)


def shaped_weights(spec, classifier=None):
    """the fixtures' state dict: oracle.detweights + the shaping described in the module docstring.  spec: (key, shape)
    pairs; classifier: (weight [1, 512], bias [1]) from hift_weights.npz."""
    sd = det_state_dict(spec, seed=WEIGHT_SEED)
    for k in sd:
        if k.endswith(".alpha"):
            sd[k] = sd[k] + 1.0
    sd["conv_post.parametrizations.weight.original0"] = sd["conv_post.parametrizations.weight.original0"] * POST_SCALE
    if classifier is not None:
        sd["f0_predictor.classifier.weight"] = torch.as_tensor(classifier[0]).float().reshape(1, -1)
        sd["f0_predictor.classifier.bias"] = torch.as_tensor(classifier[1]).float().reshape(1)
    return sd


def redraw(seed: int, B: int, L: int, harmonics: int = 9):
    """the reference's draws for a run seeded with torch.manual_seed(seed): phase [B, 9, 1], SineGen noise [B, 9, L]."""
    g = torch.Generator().manual_seed(seed)
    phase = -math.pi + torch.rand((B, harmonics, 1), generator=g) * (math.pi - -math.pi)
    noise = torch.randn((B, harmonics, L), generator=g)
    return phase, noise
