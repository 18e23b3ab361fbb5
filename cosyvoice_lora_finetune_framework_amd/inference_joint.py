"""Text token ids -> speech tokens (the fine-tuned LLM) -> mel (the fine-tuned Flow) -> waveform (the HiFT vocoder,
with ``--hift``): the no-prompt path of the reference's inference_joint.py (empty prompt, zero speaker embedding),
without the text front-end.

    python -m cosyvoice_lora_finetune_framework_amd.inference_joint --llm merged/llm.pt --flow merged/flow.pt \\
        --text-tokens 12,873,44,9 --out mel.npy [--speed 0.9] [--seed 0] [--dtype bf16]
        [--top-p 0.8 --top-k 25 --win-size 10 --tau-r 0.1] [--llm-config '{...}' --flow-config '{...}'] [--noise z.npy]
        [--hift hift.pt --wav out.wav [--wav-rate 22050] [--hift-dtype fp32] [--hift-seed 0]]
        [--prompt-wav p.wav --prompt-tokens 5,9,.. --prompt-text-tokens 3,4,.. --embedding e.npy]
        [--speech-tokenizer speech_tokenizer_v1.onnx] [--campplus campplus.onnx]
        [--stream [--token-hop 100]]
        [--lora NAME=PATH ... --voice NAME [--llm-lora-config '{...}' --flow-lora-config '{...}']]

``--llm`` / ``--flow`` are the merged state_dicts ``merge_joint_weights.py`` writes; ``--text-tokens`` is a comma-separated
id list or a ``.npy`` file of ids.  The mel is de-normalised with MEL_MEAN / MEL_STD and written as [80, T] float32.
The LLM samples with ``utils.ras_sampling`` and the given parameters (``--top-k 1 --tau-r 1e9`` is greedy).
``--llm-config`` / ``--flow-config`` are JSON keyword arguments of ``build_llm_model`` / ``build_flow_model`` for models
of other dimensions than CosyVoice-300M; ``--noise`` pins the Flow's initial noise ([1, 80, T] ``.npy``).
``--hift`` is the HiFT generator's state_dict (``hift.pt``); with it the mel also goes through ``hift.HiFTGenerator`` and
``--wav`` is written as 16-bit PCM at 22 050 Hz.  ``--hift-dtype`` is the vocoder's weight dtype (fp32 by default),
``--hift-seed`` pins its source's random phase and noise; ``--wav-rate`` resamples the waveform on the GPU
(``audio.Resampler``) before it is written.  Without ``--hift`` only the mel is written.
``--prompt-wav`` (integer PCM at any rate; resampled to 22 050 Hz on the GPU when it is at another) is turned into the
Flow's prompt mel on the GPU (``audio.MelExtractor``);
``--prompt-tokens`` / ``--prompt-text-tokens`` are the prompt's speech and text token ids (they come from the reference's
tokenizers, which are not rebuilt here) and ``--embedding`` its speaker embedding.  Without them the prompt is empty.
``--speech-tokenizer`` / ``--campplus`` (the reference's two ONNX files, run by ``onnxruntime`` on the CPU) make
``--prompt-wav`` alone enough: the prompt is resampled to 16 kHz on the GPU, its Whisper log-mel and Kaldi fbank are formed
there (``frontend16k.SpeechFrontend``) and the models turn them into the prompt's speech tokens and the speaker embedding.
An explicit ``--prompt-tokens`` or ``--embedding`` still wins.
``--stream`` (needs ``--hift``) synthesises chunk by chunk while the LLM keeps decoding (``streaming.StreamingSynthesizer``,
the reference's ``tts(stream=True)``): each chunk is appended to ``--wav`` as it arrives, the time to the first chunk and
the total time are printed and no mel file is written.  ``--token-hop`` is the number of new speech tokens per chunk
(default 2 x the Flow's token rate).  ``--wav-rate`` must stay 22050 with it: the resampler keeps no state between chunks.
``--lora NAME=PATH`` (repeatable; a name may come twice, one file per branch) serves fine-tuned voices without merging:
``--llm`` / ``--flow`` are then the BASE weights in the original key names, their target layers are LoRA-wrapped as
``--llm-lora-config`` / ``--flow-lora-config`` say (JSON ``{lora_r, lora_alpha, target_modules}``; default config.py's
``llm_lora`` / ``flow_lora``), every PATH (a ``save_lora_weights`` file or a trainer checkpoint) stays resident in an
``adapters.AdapterBank`` and ``--voice NAME`` picks the one to synthesise with (without it: the base models).
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import wave
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import utils as U
from .config import MEL_MEAN, MEL_STD


@torch.no_grad()
def synthesize(llm, flow, text_tokens, speed: float = 1.0, seed: Optional[int] = None,
               noise: Optional[torch.Tensor] = None, *, prompt_wav: Optional[torch.Tensor] = None,
               prompt_speech_token=None, prompt_text=None, embedding: Optional[torch.Tensor] = None,
               prompt_rate: Optional[int] = None, frontend=None, adapter=None) -> Tuple[List[int], torch.Tensor]:
    """-> (speech tokens, de-normalised mel (1, 80, T) fp32).  `seed` pins the LLM's sampler, `noise` the Flow's
    initial z.  Zero-shot prompting: `prompt_wav` (samples at 22 050 Hz, or at `prompt_rate` Hz: then it is resampled to
    22 050 Hz first, audio.Resampler) becomes the Flow's `prompt_feat` -- its log-mel
    (audio.MelExtractor), normalised with MEL_MEAN / MEL_STD as the reference's patched flow inference does for a
    non-empty prompt --, `prompt_speech_token` goes to both models, `prompt_text` to the LLM, `embedding` (1, 192) to
    both.  With none of them the prompt is empty and the embedding zero.  `frontend` (frontend16k.SpeechFrontend) fills
    what `prompt_wav` comes without: `prompt_speech_token` from its speech tokenizer, `embedding` from its speaker
    encoder, both on the prompt resampled to 16 kHz; a value passed explicitly wins.  `adapter`: a voice resident in the
    models' adapters.AdapterBank (or adapters.BASE): `llm` and `flow` then hold the base weights and run with that
    adapter; None runs the models as they are."""
    dev = llm.llm_decoder.weight.device
    if adapter is not None:
        activate_adapter(llm, flow, adapter)
    if frontend is not None and prompt_wav is not None:
        prompt_speech_token, embedding = prompt_from_wav(frontend, prompt_wav, prompt_rate, dev, prompt_speech_token, embedding)
    text = torch.as_tensor(text_tokens, dtype=torch.long).reshape(1, -1).to(dev)
    z = torch.zeros(1, 0, dtype=torch.long, device=dev)
    zero = torch.tensor([0])
    ids = lambda v: z if v is None else torch.as_tensor(v, dtype=torch.long).reshape(1, -1).to(dev)   # noqa: E731
    p_tok, p_text = ids(prompt_speech_token), ids(prompt_text)
    emb = torch.zeros(1, 192, device=dev) if embedding is None else embedding.float().reshape(1, -1).to(dev)
    if prompt_wav is None:
        p_feat = torch.zeros(1, 0, 80, device=dev)
    else:
        from .audio import SAMPLE_RATE, extractor, resample
        p_wav = prompt_wav.float().reshape(1, -1).to(dev)
        if prompt_rate is not None and int(prompt_rate) != SAMPLE_RATE:
            p_wav, _ = resample(p_wav, prompt_rate, SAMPLE_RATE)
        p_feat = (extractor(dev)(p_wav, channel_last=True) - MEL_MEAN) / MEL_STD
    n = lambda t: torch.tensor([t.shape[1]])                                                           # noqa: E731
    tokens = list(llm.inference(text, n(text), p_text, n(p_text), p_tok, n(p_tok), emb, seed=seed, adapter=adapter))
    if not tokens:
        raise RuntimeError("the LLM produced no speech tokens")
    tok = torch.tensor([tokens], dtype=torch.long, device=dev)
    mel, _ = flow.inference(tok, torch.tensor([len(tokens)]), p_tok, n(p_tok), p_feat, n(p_feat), emb, noise=noise)
    mel = mel * MEL_STD + MEL_MEAN
    if speed != 1.0:
        mel = F.interpolate(mel, size=int(mel.shape[2] / speed), mode='linear')
    return tokens, mel


def activate_adapter(llm, flow, adapter) -> None:
    """set the module-run LoRA layers of both models to `adapter` (on the current stream, before either model runs)."""
    from .adapters import bank_of
    banks = [bank_of(llm)] + ([flow.__dict__["_cvft_adapter_bank"]] if "_cvft_adapter_bank" in flow.__dict__ else [])
    for bank in {id(b): b for b in banks}.values():
        bank.activate(adapter)


def load_adapters(llm, flow, specs: List[str], llm_lora: dict, flow_lora: dict, rank: Optional[int] = None):
    """--lora NAME=PATH ...: wrap the base models' target layers (zero adapters), build one AdapterBank over both and
    load every file into its name (one file per branch, or a trainer checkpoint: a name may be given more than once)."""
    from .adapters import RANKS, AdapterBank
    from .lora import apply_lora_to_model
    for model, cfg in ((llm, llm_lora), (flow, flow_lora)):
        apply_lora_to_model(model, r=cfg['lora_r'], lora_alpha=cfg['lora_alpha'], lora_dropout=0.0,
                            target_modules=cfg['target_modules'])
        for n, p in model.named_parameters():
            if 'lora_' in n:
                p.data.zero_()
    pairs = []
    for spec in specs:
        name, sep, path = spec.partition('=')
        if not sep or not name or not path:
            raise SystemExit(f"--lora wants NAME=PATH, got '{spec}'")
        pairs.append((name, path))
    names = list(dict.fromkeys(n for n, _ in pairs))
    if rank is None:
        rank = next(r for r in RANKS if r >= max(llm_lora['lora_r'], 8))
    bank = AdapterBank(llm=llm, flow=flow, capacity=max(len(names), 1), rank=rank)
    for name, path in pairs:
        bank.load(name, path)
    return bank


def prompt_from_wav(frontend, prompt_wav: torch.Tensor, prompt_rate: Optional[int], dev, prompt_speech_token=None,
                    embedding: Optional[torch.Tensor] = None):
    """-> (prompt_speech_token, embedding): whichever is None and has a model in `frontend` is computed from `prompt_wav`
    (at `prompt_rate` Hz, default 22 050) resampled to 16 kHz on `dev`."""
    from .audio import FRONTEND_RATE, SAMPLE_RATE, resample
    want_tok = prompt_speech_token is None and frontend.speech_tokenizer is not None
    want_emb = embedding is None and frontend.speaker_encoder is not None
    if want_tok or want_emb:
        w16, _ = resample(prompt_wav.float().reshape(1, -1).to(dev), SAMPLE_RATE if prompt_rate is None else int(prompt_rate),
                          FRONTEND_RATE)
        if want_tok:
            prompt_speech_token = frontend.tokens(w16)[0]
        if want_emb:
            embedding = frontend.embeddings(w16)
    return prompt_speech_token, embedding


@torch.no_grad()
def vocode(hift, mel: torch.Tensor, seed: Optional[int] = None, draws=None, dtype=None) -> torch.Tensor:
    """de-normalised mel (B, 80, T) -> waveform (B, T*256) fp32 in [-0.99, 0.99] at 22 050 Hz (hift.HiFTGenerator)."""
    wav, _ = hift.inference(mel, draws=draws, seed=seed, dtype=dtype)
    return wav


def pcm16(wav: torch.Tensor) -> np.ndarray:
    return np.clip(np.rint(wav.detach().float().cpu().numpy() * 32767.0), -32768, 32767).astype('<i2')


def write_wav(path: str, wav: torch.Tensor, rate: int = 22050) -> None:
    """mono 16-bit PCM of wav [T] (values in [-1, 1])."""
    with wave.open(path, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm16(wav.reshape(-1)).tobytes())


def _text_tokens(arg: str) -> List[int]:
    if os.path.exists(arg):
        return [int(v) for v in np.load(arg).reshape(-1)]
    return [int(v) for v in arg.replace(' ', '').split(',') if v]


def main(argv=None):
    from .flow_model import build_flow_model
    from .llm_model import build_llm_model
    from .modules import Numerics
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--llm', required=True, help='merged LLM state_dict (merge_joint_weights.py); with --lora: the base LLM')
    ap.add_argument('--flow', required=True, help='merged Flow state_dict (merge_joint_weights.py); with --lora: the base Flow')
    ap.add_argument('--lora', action='append', default=[], metavar='NAME=PATH',
                    help='a voice: LoRA tensors (save_lora_weights file of a branch, or a trainer checkpoint) kept resident '
                         'under NAME over the base models; repeatable, also per name')
    ap.add_argument('--voice', default=None, help='with --lora: the NAME to synthesise with (default: the base models)')
    ap.add_argument('--llm-lora-config', default=None, help='JSON {lora_r, lora_alpha, target_modules} (default: config.py llm_lora)')
    ap.add_argument('--flow-lora-config', default=None, help='JSON {lora_r, lora_alpha, target_modules} (default: config.py flow_lora)')
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
    ap.add_argument('--prompt-wav', default=None, help='zero-shot prompt: integer PCM at any rate (its mel conditions the Flow)')
    ap.add_argument('--prompt-tokens', default=None, help='the prompt\'s speech token ids (comma-separated or .npy)')
    ap.add_argument('--prompt-text-tokens', default=None, help='the prompt\'s text token ids (comma-separated or .npy)')
    ap.add_argument('--embedding', default=None, help='.npy of the speaker embedding (192 floats); default zero')
    ap.add_argument('--speech-tokenizer', default=None, help='the speech tokenizer\'s .onnx: --prompt-wav yields the prompt tokens')
    ap.add_argument('--campplus', default=None, help='the speaker encoder\'s .onnx: --prompt-wav yields the embedding')
    ap.add_argument('--hift', default=None, help='HiFT generator state_dict (hift.pt): also vocode the mel')
    ap.add_argument('--wav', default='out.wav', help='with --hift: the waveform, 16-bit PCM at --wav-rate')
    ap.add_argument('--wav-rate', type=int, default=22050, help='rate of --wav; other than 22050: resampled on the GPU')
    ap.add_argument('--hift-dtype', choices=('fp32', 'bf16'), default='fp32')
    ap.add_argument('--hift-seed', type=int, default=None)
    ap.add_argument('--stream', action='store_true', help='with --hift: synthesise chunk by chunk, appending to --wav')
    ap.add_argument('--token-hop', type=int, default=None, help='with --stream: new speech tokens per chunk')
    a = ap.parse_args(argv)
    if a.stream and not a.hift:
        ap.error('--stream needs --hift: a streamed chunk is a piece of the waveform')
    if a.stream and a.wav_rate != 22050:
        ap.error('--stream writes at 22050 Hz only: the resampler keeps no state from one chunk to the next, '
                 'so --wav-rate %d cannot be combined with it' % a.wav_rate)
    if a.stream and a.noise:
        ap.error('--noise pins one initial noise tensor; with --stream every chunk draws its own (use --seed / torch.manual_seed)')
    if a.token_hop is not None and not a.stream:
        ap.error('--token-hop is an option of --stream')
    if a.voice is not None and not a.lora:
        ap.error('--voice names one of the --lora NAME=PATH adapters')
    num = Numerics(dtype=torch.bfloat16 if a.dtype == 'bf16' else torch.float32)
    kw = lambda js: {k: tuple(v) if isinstance(v, list) else v for k, v in json.loads(js).items()}   # noqa: E731
    llm = build_llm_model(None, 'cpu', numerics=num, **kw(a.llm_config))
    llm.load_state_dict(torch.load(a.llm, map_location='cpu', weights_only=True), strict=True)
    flow = build_flow_model(None, 'cpu', numerics=num, **kw(a.flow_config))
    flow.load_state_dict(torch.load(a.flow, map_location='cpu', weights_only=True), strict=True)
    dev = torch.device('cuda')
    llm, flow = llm.to(dev).eval(), flow.to(dev).eval()
    adapter = None
    if a.lora:
        from .adapters import BASE
        from .config import JOINT_TRAINING_CONFIG
        cfgs = [json.loads(js) if js else JOINT_TRAINING_CONFIG[k]
                for js, k in ((a.llm_lora_config, 'llm_lora'), (a.flow_lora_config, 'flow_lora'))]
        load_adapters(llm, flow, a.lora, *cfgs)
        adapter = a.voice if a.voice is not None else BASE
    llm.sampling = functools.partial(U.ras_sampling, top_p=a.top_p, top_k=a.top_k, win_size=a.win_size, tau_r=a.tau_r)
    noise = torch.from_numpy(np.load(a.noise)).float().to(dev) if a.noise else None
    prompt = {}
    if a.prompt_wav:
        from .audio import load_wav
        prompt['prompt_wav'], prompt['prompt_rate'] = load_wav(a.prompt_wav)
    if a.prompt_tokens:
        prompt['prompt_speech_token'] = _text_tokens(a.prompt_tokens)
    if a.prompt_text_tokens:
        prompt['prompt_text'] = _text_tokens(a.prompt_text_tokens)
    if a.embedding:
        prompt['embedding'] = torch.from_numpy(np.load(a.embedding)).float()
    if (a.speech_tokenizer or a.campplus) and a.prompt_wav:
        from .frontend16k import SpeechFrontend
        fe = SpeechFrontend.from_onnx(a.speech_tokenizer, a.campplus, dev)
        tok, emb = prompt_from_wav(fe, prompt['prompt_wav'], prompt['prompt_rate'], dev, prompt.get('prompt_speech_token'),
                                   prompt.get('embedding'))
        if tok is not None:
            prompt['prompt_speech_token'] = tok
        if emb is not None:
            prompt['embedding'] = emb
    if a.stream:
        return _stream_main(a, llm, flow, dev, prompt, adapter)
    tokens, mel = synthesize(llm, flow, _text_tokens(a.text_tokens), a.speed, a.seed, noise=noise, adapter=adapter, **prompt)
    np.save(a.out, mel[0].cpu().numpy().astype(np.float32))
    print(f"{len(tokens)} speech tokens -> mel {tuple(mel.shape[1:])} -> {a.out}")
    if a.hift:
        from .hift import HiFTGenerator
        voc = HiFTGenerator(dtype=torch.bfloat16 if a.hift_dtype == 'bf16' else torch.float32)
        voc.load_state_dict(torch.load(a.hift, map_location='cpu', weights_only=True), strict=True)
        wav = vocode(voc.to(dev).eval(), mel, seed=a.hift_seed)
        if a.wav_rate != voc.sampling_rate:
            from .audio import resample
            wav, _ = resample(wav, voc.sampling_rate, a.wav_rate)
        write_wav(a.wav, wav[0], a.wav_rate)
        print(f"mel -> {wav.shape[1]} samples at {a.wav_rate} Hz -> {a.wav}")


def _stream_main(a, llm, flow, dev, prompt, adapter=None):
    """--stream: chunks go to --wav as they arrive (16-bit PCM converted on the device by the stitch launch)."""
    import time
    from .hift import HiFTGenerator
    from .streaming import SPEED_MSG, StreamingSynthesizer
    if a.speed != 1.0:
        raise SystemExit(SPEED_MSG)
    voc = HiFTGenerator(dtype=torch.bfloat16 if a.hift_dtype == 'bf16' else torch.float32)
    voc.load_state_dict(torch.load(a.hift, map_location='cpu', weights_only=True), strict=True)
    syn = StreamingSynthesizer(llm, flow, voc.to(dev).eval(), token_hop_len=a.token_hop)
    torch.cuda.synchronize(dev)
    t0, first, n, chunks = time.perf_counter(), None, 0, 0
    with wave.open(a.wav, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(voc.sampling_rate)
        for item in syn.tts(_text_tokens(a.text_tokens), stream=True, seed=a.seed, hift_seed=a.hift_seed,
                            want_pcm=True, adapter=adapter, **prompt):
            pcm = item['pcm'].cpu().numpy().astype('<i2')
            first = time.perf_counter() - t0 if first is None else first
            f.writeframes(pcm.tobytes())
            n, chunks = n + pcm.shape[0], chunks + 1
    total = time.perf_counter() - t0
    print(f"{chunks} chunks -> {n} samples at {voc.sampling_rate} Hz -> {a.wav}")
    print(f"first chunk after {first * 1e3:.1f} ms, total {total * 1e3:.1f} ms")


if __name__ == '__main__':
    main()
