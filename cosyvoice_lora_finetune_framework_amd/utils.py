"""Length / mask helpers with the reference's names (utils.py:20-109 == cosyvoice/utils/mask.py).

The HIP path never materialises these masks (kernels consume int32 lengths); the functions
exist for API compatibility and run on whatever device `lengths` lives on.  `make_pad_mask`
with max_len=0 needs `lengths.max()`; pass `max_len` to stay sync-free."""
import random

import numpy as np
import torch

IGNORE_ID = -1


def set_all_random_seed(seed: int):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def make_pad_mask(lengths: torch.Tensor, max_len: int = 0) -> torch.Tensor:
    """True at padded positions.  make_pad_mask([5,3,2]) -> [[0,0,0,0,0],[0,0,0,1,1],[0,0,1,1,1]]."""
    n = max_len if max_len > 0 else int(lengths.max().item())
    return torch.arange(n, dtype=torch.int64, device=lengths.device)[None, :] >= lengths[:, None]


def subsequent_chunk_mask(size: int, chunk_size: int, num_left_chunks: int = -1,
                          device: torch.device = torch.device("cpu")) -> torch.Tensor:
    pos = torch.arange(size, device=device)
    limit = (torch.div(pos, chunk_size, rounding_mode='trunc') + 1) * chunk_size
    return pos[None, :] < limit[:, None]


def add_optional_chunk_mask(xs, masks, use_dynamic_chunk, use_dynamic_left_chunk, decoding_chunk_size,
                            static_chunk_size, num_decoding_left_chunks, enable_full_context=True):
    if use_dynamic_chunk:
        raise NotImplementedError("dynamic chunk training is not used by CosyVoice-300M")
    if static_chunk_size > 0:
        cm = masks & subsequent_chunk_mask(xs.size(1), static_chunk_size, num_decoding_left_chunks, xs.device)[None]
    else:
        cm = masks
    assert cm.dtype == torch.bool
    dead = cm.sum(dim=-1) == 0
    if bool(dead.any()):
        cm = cm.clone()
        cm[dead] = True
    return cm


def mask_to_bias(mask: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    assert mask.dtype == torch.bool
    assert dtype in (torch.float32, torch.bfloat16, torch.float16)
    return (1.0 - mask.to(dtype)) * -1.0e+10


def pad_list(xs, pad_value: int):
    n = max(len(x) for x in xs)
    out = xs[0].new_full((len(xs), n) + tuple(xs[0].shape[1:]), pad_value)
    for i, x in enumerate(xs):
        out[i, :len(x)] = x
    return out


# ---------------------------------------------------------------------------------------------- token samplers
# Host forms of the reference samplers (cosyvoice/utils/common.py:111-139), same signatures.  The decode session
# (decode.py) runs a functools.partial of these on the device with the partial's parameters; any other callable is
# called here on the host once per step.
def nucleus_sampling(weighted_scores: torch.Tensor, top_p: float = 0.8, top_k: int = 25) -> torch.Tensor:
    """Draw from the candidates of the stable descending order, taken while their cumulative probability is below
    top_p and fewer than top_k are taken (so the candidate that crosses top_p is included); the draw is proportional to
    the candidates' un-renormalised probabilities."""
    probs, order = weighted_scores.softmax(dim=0).sort(descending=True, stable=True)
    cum = torch.zeros((), dtype=probs.dtype, device=probs.device)
    n = 0
    while n < len(order) and bool(cum < top_p) and n < top_k:
        cum = cum + probs[n]
        n += 1
    pick = probs[:n].multinomial(1, replacement=True)
    return order[:n][pick]


def random_sampling(weighted_scores: torch.Tensor, decoded_tokens, sampling) -> torch.Tensor:
    """One draw from the full softmax."""
    return weighted_scores.softmax(dim=0).multinomial(1, replacement=True)


def ras_sampling(weighted_scores: torch.Tensor, decoded_tokens, sampling, top_p: float = 0.8, top_k: int = 25,
                 win_size: int = 10, tau_r: float = 0.1) -> torch.Tensor:
    """Repetition-aware sampling (VALL-E 2): a nucleus draw, replaced by a draw from the full softmax when the drawn id
    already occurs at least win_size * tau_r times among the last win_size decoded tokens."""
    top_ids = nucleus_sampling(weighted_scores, top_p=top_p, top_k=top_k)
    recent = list(decoded_tokens)[-win_size:] if win_size > 0 else []
    rep = sum(1 for t in recent if int(t) == int(top_ids))
    if rep >= win_size * tau_r:
        top_ids = random_sampling(weighted_scores, decoded_tokens, sampling)
    return top_ids
