"""Text token ids -> speech tokens (the fine-tuned LLM) -> mel (the fine-tuned Flow): the no-prompt path of the
reference's inference_joint.py (empty prompt, zero speaker embedding), without the text front-end and the vocoder.

    python -m cosyvoice_lora_finetune_framework_amd.inference_joint --llm merged/llm.pt --flow merged/flow.pt \\
        --text-tokens 12,873,44,9 --out mel.npy [--speed 0.9] [--seed 0] [--dtype bf16]
        [--top-p 0.8 --top-k 25 --win-size 10 --tau-r 0.1] [--llm-config '{...}' --flow-config '{...}'] [--noise z.npy]

``--llm`` / ``--flow`` are the merged state_dicts ``merge_joint_weights.py`` writes; ``--text-tokens`` is a comma-separated
id list or a ``.npy`` file of ids.  The mel is de-normalised with MEL_MEAN / MEL_STD and written as [80, T] float32.
The LLM samples with ``utils.ras_sampling`` and the given parameters (``--top-k 1 --tau-r 1e9`` is greedy).
``--llm-config`` / ``--flow-config`` are JSON keyword arguments of ``build_llm_model`` / ``build_flow_model`` for models
of other dimensions than CosyVoice-300M; ``--noise`` pins the Flow's initial noise ([1, 80, T] ``.npy``).
"""
from __future__ import annotations

import argparse
import functools
import json
import os
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import utils as U
from .config import MEL_MEAN, MEL_STD


@torch.no_grad()
def synthesize(llm, flow, text_tokens, speed: float = 1.0, seed: Optional[int] = None,
               noise: Optional[torch.Tensor] = None) -> Tuple[List[int], torch.Tensor]:
    """-> (speech tokens, de-normalised mel (1, 80, T) fp32).  `seed` pins the LLM's sampler, `noise` the Flow's
    initial z."""
    dev = llm.llm_decoder.weight.device
    text = torch.as_tensor(text_tokens, dtype=torch.long).reshape(1, -1).to(dev)
    z = torch.zeros(1, 0, dtype=torch.long, device=dev)
    zero = torch.tensor([0])
    emb = torch.zeros(1, 192, device=dev)
    tokens = list(llm.inference(text, torch.tensor([text.shape[1]]), z, zero, z, zero, emb, seed=seed))
    if not tokens:
        raise RuntimeError("the LLM produced no speech tokens")
    tok = torch.tensor([tokens], dtype=torch.long, device=dev)
    mel, _ = flow.inference(tok, torch.tensor([len(tokens)]), z, zero, torch.zeros(1, 0, 80, device=dev), zero,
                            torch.zeros(1, 192, device=dev), noise=noise)
    mel = mel * MEL_STD + MEL_MEAN
    if speed != 1.0:
        mel = F.interpolate(mel, size=int(mel.shape[2] / speed), mode='linear')
    return tokens, mel


def _text_tokens(arg: str) -> List[int]:
    if os.path.exists(arg):
        return [int(v) for v in np.load(arg).reshape(-1)]
    return [int(v) for v in arg.replace(' ', '').split(',') if v]


def main(argv=None):
    from .flow_model import build_flow_model
    from .llm_model import build_llm_model
    from .modules import Numerics
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--llm', required=True, help='merged LLM state_dict (merge_joint_weights.py)')
    ap.add_argument('--flow', required=True, help='merged Flow state_dict (merge_joint_weights.py)')
    ap.add_argument('--text-tokens', required=True, help='comma-separated text token ids, or a .npy file of ids')
    ap.add_argument('--out', default='mel.npy')
    ap.add_argument('--speed', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--dtype', choices=('fp32', 'bf16'), default='fp32')
    ap.add_argument('--top-p', type=float, default=0.8)
    ap.add_argument('--top-k', type=int, default=25)
    ap.add_argument('--win-size', type=int, default=10)
    ap.add_argument('--tau-r', type=float, default=0.1)
    ap.add_argument('--llm-config', default='{}', help='JSON keyword arguments of build_llm_model')
    ap.add_argument('--flow-config', default='{}', help='JSON keyword arguments of build_flow_model')
    ap.add_argument('--noise', default=None, help='.npy of the Flow\'s initial noise [1, 80, T]')
    a = ap.parse_args(argv)
    num = Numerics(dtype=torch.bfloat16 if a.dtype == 'bf16' else torch.float32)
    kw = lambda js: {k: tuple(v) if isinstance(v, list) else v for k, v in json.loads(js).items()}   # noqa: E731
    llm = build_llm_model(None, 'cpu', numerics=num, **kw(a.llm_config))
    llm.load_state_dict(torch.load(a.llm, map_location='cpu', weights_only=True), strict=True)
    flow = build_flow_model(None, 'cpu', numerics=num, **kw(a.flow_config))
    flow.load_state_dict(torch.load(a.flow, map_location='cpu', weights_only=True), strict=True)
    dev = torch.device('cuda')
    llm, flow = llm.to(dev).eval(), flow.to(dev).eval()
    llm.sampling = functools.partial(U.ras_sampling, top_p=a.top_p, top_k=a.top_k, win_size=a.win_size, tau_r=a.tau_r)
    noise = torch.from_numpy(np.load(a.noise)).float().to(dev) if a.noise else None
    tokens, mel = synthesize(llm, flow, _text_tokens(a.text_tokens), a.speed, a.seed, noise=noise)
    np.save(a.out, mel[0].cpu().numpy().astype(np.float32))
    print(f"{len(tokens)} speech tokens -> mel {tuple(mel.shape[1:])} -> {a.out}")


if __name__ == '__main__':
    main()
