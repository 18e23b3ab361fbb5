"""Streaming synthesis: chunked token -> wav while the LLM keeps decoding (cosyvoice/cli/model.py CosyVoiceModel.tts with
stream=True, token2wav and the per-uuid dictionaries).

As soon as ``token_hop_len + token_overlap_len`` speech tokens exist, ``token2wav`` turns them into audio: the Flow
(``MaskedDiffWithXvec.inference`` with its ``flow_cache``), a Hamming cross-fade of the 34 mel frames that consecutive
chunks share, the HiFT vocoder re-fed 20 cached mel frames and their source, and a cross-fade of the last 5120 samples.
Both fades, with the slicing and concatenation around them, are one launch each (csrc/stream.hip); the state between
chunks (``StreamState``) stays on the device.

One host thread, two streams: the LLM's decode steps (a captured graph) run on a stream of their own, ``token2wav`` on the
caller's.  Tokens cross between them through the host (the one read per decode step), chunks are cut by token COUNT only
(``chunk_plan``), so what is computed never depends on how the two streams interleave.
"""
from __future__ import annotations

import time
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import config as CFG
from .config import MEL_MEAN, MEL_STD
from .hipops import functional as HF

SPEED_MSG = 'speed change only support non-stream inference mode'
MEL_HOP, MEL_RATE = 256, 22050
SERVE_KEYS = {"text_tokens", "prompt_wav", "prompt_rate", "prompt_speech_token", "prompt_text", "embedding", "prompt_feat",
              "seed", "noise", "hift_seed", "hift_draws", "hift_dtype", "want_pcm", "adapter", "llm_kw"}


class StreamState:
    """What one request carries from chunk to chunk (the reference's flow_cache_dict / mel_overlap_dict /
    hift_cache_dict entries), all on the device."""

    def __init__(self):
        self.flow_cache: Optional[torch.Tensor] = None      # [1, 80, prompt + 34, 2]: the sampler's z and mu
        self.mel_overlap: Optional[torch.Tensor] = None     # [80, 34]: the columns cut off the previous chunk
        self.hift_mel: Optional[torch.Tensor] = None        # [80, <= 20]: the end of the previous vocoder input
        self.hift_source: Optional[torch.Tensor] = None     # [1, 1, 5120]: the end of the previous source
        self.hift_speech: Optional[torch.Tensor] = None     # [5120]: the withheld end of the previous speech

    @property
    def cached(self) -> bool:
        return self.hift_mel is not None


class StreamingSynthesizer:
    def __init__(self, llm, flow, hift, *, token_hop_len: Optional[int] = None, token_max_hop_len: Optional[int] = None,
                 token_overlap_len: int = 20, mel_cache_len: int = 20, stream_scale_factor: float = 1,
                 boundary_trim_ratio: Optional[float] = None):
        self.llm, self.flow, self.hift = llm, flow, hift
        rate = flow.input_frame_rate
        self.token_min_hop_len = 2 * rate if token_hop_len is None else int(token_hop_len)
        if token_max_hop_len is None:                  # (a hop above the default ceiling keeps its size)
            token_max_hop_len = max(4 * rate, self.token_min_hop_len)
        self.token_max_hop_len = int(token_max_hop_len)
        self.token_overlap_len = int(token_overlap_len)
        self.mel_overlap_len = int(self.token_overlap_len / rate * MEL_RATE / MEL_HOP)
        self.mel_cache_len = int(mel_cache_len)
        self.source_cache_len = int(self.mel_cache_len * MEL_HOP)
        if stream_scale_factor < 1:
            raise ValueError('stream_scale_factor should be greater than 1, change it according to your actual rtf')
        self.stream_scale_factor = stream_scale_factor
        if self.token_min_hop_len < 1 or self.token_overlap_len < 0:
            raise ValueError(f"token_hop_len {self.token_min_hop_len}, token_overlap_len {self.token_overlap_len}")
        first = int((self.token_min_hop_len + self.token_overlap_len) / rate * MEL_RATE / MEL_HOP) - self.mel_overlap_len
        if first < max(self.mel_cache_len, 1):
            raise ValueError(f"token_hop_len {self.token_min_hop_len} is too small: a chunk of {self.token_min_hop_len} + "
                             f"{self.token_overlap_len} tokens leaves {first} mel frames after the overlap of "
                             f"{self.mel_overlap_len}, fewer than the vocoder's cache of {self.mel_cache_len}")
        if boundary_trim_ratio is None:
            boundary_trim_ratio = getattr(CFG, 'INFERENCE_CONFIG', {}).get('boundary_trim_ratio', 0.15)
        self.boundary_trim_ratio = float(boundary_trim_ratio)
        self.mel_window = np.hamming(2 * self.mel_overlap_len)            # fp64, as the reference holds them
        self.speech_window = np.hamming(2 * self.source_cache_len)
        self._dev_windows: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._llm_stream: Optional[torch.cuda.Stream] = None
        self._servers: Dict[tuple, object] = {}          # serve(): (rows, prefill_rows, adapters, cache) -> DecodeServer
        self.last_timing: Dict[str, float] = {}

    # ------------------------------------------------------------------ host logic
    def chunk_plan(self, n_tokens: int) -> List[Tuple[int, int, bool]]:
        """[(start, stop, finalize), ...]: the token windows the reference's loop (model.py:239-266) cuts out of
        n_tokens speech tokens.  A window of hop + overlap tokens is synthesised whenever that many are left, then hop of
        them are dropped and the hop grows by stream_scale_factor up to token_max_hop_len; what is left at the end is
        the final chunk."""
        plan, start, hop, ov = [], 0, self.token_min_hop_len, self.token_overlap_len
        while n_tokens - start >= hop + ov:
            plan.append((start, start + hop + ov, False))
            start += hop
            hop = min(self.token_max_hop_len, int(hop * self.stream_scale_factor))
        plan.append((start, n_tokens, True))
        return plan

    def chunk_frames(self, n_tokens: int, prompt_mel_len: int) -> Tuple[int, int]:
        """(mel frames the Flow returns for a chunk of n_tokens, the boundary trim applied to them)."""
        mel2 = int(n_tokens / self.flow.input_frame_rate * MEL_RATE / MEL_HOP)
        trim = int(prompt_mel_len * self.boundary_trim_ratio)
        return mel2, trim if trim > 0 and mel2 > trim else 0

    def check_chunk(self, n_tokens: int, prompt_mel_len: int, finalize: bool, has_overlap: bool) -> Tuple[int, int]:
        """On the host, before anything is launched: a chunk that is shorter than the overlap after trimming cannot be
        stitched (the reference fails on a shape mismatch inside fade_in_out)."""
        mel2, trim = self.chunk_frames(n_tokens, prompt_mel_len)
        if mel2 < 1:
            raise ValueError(f"a chunk of {n_tokens} tokens gives no mel frame")
        if mel2 - trim < self.mel_overlap_len and (has_overlap or not finalize):
            raise ValueError(f"chunk too short to stitch: {n_tokens} tokens give {mel2} mel frames, {mel2 - trim} after the "
                             f"boundary trim of {trim}, below the mel overlap of {self.mel_overlap_len}")
        return mel2, trim

    def windows(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mel window [2 * 34], speech window [2 * 5120]) fp32 on `device`, uploaded once."""
        device = torch.device(device)
        if device not in self._dev_windows:
            self._dev_windows[device] = (torch.from_numpy(self.mel_window).float().to(device),
                                         torch.from_numpy(self.speech_window).float().to(device))
        return self._dev_windows[device]

    # ------------------------------------------------------------------ one chunk
    @torch.no_grad()
    def token2wav(self, state: StreamState, token, prompt_token, prompt_feat, embedding, finalize: bool, speed: float = 1.0,
                  noise: Optional[torch.Tensor] = None, hift_draws=None, *, hift_seed: Optional[int] = None,
                  hift_dtype=None, want_pcm: bool = False, taps: Optional[dict] = None) -> torch.Tensor:
        """The reference's token2wav on `state`: token [1, n] -> this chunk's speech [1, samples] (on the device).
        prompt_feat [1, frames, 80] is the prompt's log-mel (not normalised; it is normalised for the Flow here and the
        Flow's output de-normalised before the fade).  The boundary trim is applied to EVERY chunk, as the reference does.
        noise pins the Flow's initial z, hift_draws / hift_seed the vocoder's draws; taps receives the intermediates, at
        no extra launch (flow_raw: the Flow's output as it returns it, normalised; mel: the vocoder's input, overlap,
        cache_mel, source, speech_raw, pcm)."""
        dev = self.flow.input_embedding.weight.device
        token = torch.as_tensor(token, dtype=torch.long).reshape(1, -1)
        mel1 = prompt_feat.shape[1]
        _, trim = self.check_chunk(token.shape[1], mel1, finalize, state.mel_overlap is not None)
        if speed != 1.0 and state.cached:
            raise AssertionError(SPEED_MSG)
        mel_w, speech_w = self.windows(dev)
        n = lambda t: torch.tensor([t.shape[1]])                                                        # noqa: E731
        p_feat = prompt_feat.to(dev).float()
        if mel1 > 0:
            p_feat = (p_feat - MEL_MEAN) / MEL_STD
        mel, state.flow_cache = self.flow.inference(token.to(dev), n(token), prompt_token.to(dev), n(prompt_token), p_feat,
                                                    n(p_feat), embedding.to(dev), flow_cache=state.flow_cache, noise=noise)
        vin, overlap, cache_mel = HF.stream_mel_stitch(mel[0], trim, self.mel_overlap_len, mel_w, prev=state.mel_overlap,
                                                       cache=state.hift_mel, finalize=finalize,
                                                       scale_shift=(MEL_STD, MEL_MEAN),
                                                       cache_len=0 if finalize else self.mel_cache_len)
        if finalize and speed != 1.0:
            vin = F.interpolate(vin.unsqueeze(0), size=int(vin.shape[1] / speed), mode='linear')[0]
        if vin.shape[1] == 0:
            raise ValueError(f"chunk too short to vocode: nothing is left of {mel.shape[2]} mel frames after the trim of "
                             f"{trim} and the overlap of {self.mel_overlap_len}")
        speech, source = self.hift.inference(vin.unsqueeze(0), cache_source=state.hift_source, draws=hift_draws,
                                             seed=hift_seed, dtype=hift_dtype)
        out, cache_speech, pcm = HF.stream_wav_stitch(speech[0], self.source_cache_len, speech_w, cache=state.hift_speech,
                                                      finalize=finalize, want_pcm=want_pcm)
        if taps is not None:
            taps.update(flow_raw=mel, mel=vin, overlap=overlap, cache_mel=cache_mel, source=source, speech_raw=speech,
                        pcm=pcm)
        if not finalize:
            state.mel_overlap, state.hift_mel, state.hift_speech = overlap, cache_mel, cache_speech
            state.hift_source = source[:, :, -self.source_cache_len:]
        return out.unsqueeze(0)

    # ------------------------------------------------------------------ the request
    def _prompt(self, dev, prompt_wav, prompt_rate, prompt_speech_token, prompt_text, embedding):
        z = torch.zeros(1, 0, dtype=torch.long, device=dev)
        ids = lambda v: z if v is None else torch.as_tensor(v, dtype=torch.long).reshape(1, -1).to(dev)   # noqa: E731
        emb = torch.zeros(1, 192, device=dev) if embedding is None else embedding.float().reshape(1, -1).to(dev)
        if prompt_wav is None:
            p_feat = torch.zeros(1, 0, 80, device=dev)
        else:
            from .audio import SAMPLE_RATE, extractor, resample
            p_wav = prompt_wav.float().reshape(1, -1).to(dev)
            if prompt_rate is not None and int(prompt_rate) != SAMPLE_RATE:
                p_wav, _ = resample(p_wav, prompt_rate, SAMPLE_RATE)
            p_feat = extractor(dev)(p_wav, channel_last=True)
        return ids(prompt_speech_token), ids(prompt_text), emb, p_feat

    def llm_stream(self, dev) -> torch.cuda.Stream:
        if self._llm_stream is None:
            self._llm_stream = torch.cuda.Stream(dev)
        return self._llm_stream

    @torch.no_grad()
    def tts(self, text_tokens=None, *, prompt_wav: Optional[torch.Tensor] = None, prompt_rate: Optional[int] = None,
            prompt_speech_token=None, prompt_text=None, embedding: Optional[torch.Tensor] = None,
            prompt_feat: Optional[torch.Tensor] = None, stream: bool = True, speed: float = 1.0, seed: Optional[int] = None,
            source_speech_token: Optional[Sequence[int]] = None, noise=None, hift_seed: Optional[int] = None,
            hift_draws=None, hift_dtype=None, use_graph: bool = True, want_pcm: bool = False,
            llm_kw: Optional[dict] = None, adapter=None) -> Iterator[dict]:
        """Generator of {'tts_speech': [1, n] fp32 on the device, complete when it is yielded} (with want_pcm also
        'pcm': [n] int16).  stream=False yields one item: the whole utterance through one final token2wav, as the reference's
        tts(stream=False) does.  With an empty prompt that is inference_joint.synthesize + vocode bit for bit (at any
        speed); behind a prompt token2wav also applies the boundary trim, which synthesize does not.
        source_speech_token skips the LLM (the reference's vc_job).  seed pins the LLM's sampler; noise (one tensor, or one
        per chunk) the Flow's initial z; hift_seed the vocoder's draws (chunk i draws with hift_seed + i) and hift_draws
        (one pair per chunk) replaces them.  prompt_feat [1, frames, 80] (log-mel, not normalised) may be given in place
        of prompt_wav; llm_kw: further keywords of ``llm.inference`` (the token / text ratios).  adapter: a voice resident in the
        models' adapters.AdapterBank (or adapters.BASE), as ``inference_joint.synthesize(adapter=)``; it is written into the
        modules on the caller's stream before the LLM's stream forks off.  After the generator ends,
        ``last_timing`` holds the host's view of the overlap."""
        dev = self.flow.input_embedding.weight.device
        if adapter is not None:
            from .inference_joint import activate_adapter
            activate_adapter(self.llm, self.flow, adapter)
        p_tok, p_text, emb, p_feat = self._prompt(dev, prompt_wav, prompt_rate, prompt_speech_token, prompt_text, embedding)
        if prompt_feat is not None:
            p_feat = prompt_feat.float().to(dev)
        pick_noise = lambda i: noise[i] if isinstance(noise, (list, tuple)) else noise                    # noqa: E731
        pick_draws = lambda i: hift_draws[i] if isinstance(hift_draws, list) else hift_draws              # noqa: E731
        state = StreamState()

        def chunk(tokens, i, finalize, spd=1.0):
            pcm_taps = {} if want_pcm else None
            wav = self.token2wav(state, torch.tensor([tokens], dtype=torch.long), p_tok, p_feat, emb, finalize, spd,
                                 noise=pick_noise(i), hift_draws=pick_draws(i),
                                 hift_seed=None if hift_seed is None else hift_seed + i, hift_dtype=hift_dtype,
                                 want_pcm=want_pcm, taps=pcm_taps)
            item = {'tts_speech': wav}
            if want_pcm:
                item['pcm'] = pcm_taps['pcm']
            return item

        if source_speech_token is not None:
            tokens_it = iter([int(t) for t in torch.as_tensor(source_speech_token).reshape(-1).tolist()])
            llm_stream = None
        else:
            if text_tokens is None:
                raise ValueError("text_tokens or source_speech_token is needed")
            text = torch.as_tensor(text_tokens, dtype=torch.long).reshape(1, -1).to(dev)
            n = lambda t: torch.tensor([t.shape[1]])                                                    # noqa: E731
            tokens_it = self.llm.inference(text, n(text), p_text, n(p_text), p_tok, n(p_tok), emb, seed=seed,
                                           use_graph=use_graph, **({} if adapter is None else {'adapter': adapter}),
                                           **(llm_kw or {}))
            llm_stream = self.llm_stream(dev) if stream else None

        if not stream:
            tokens = list(tokens_it)
            if not tokens:
                raise RuntimeError("the LLM produced no speech tokens")
            yield chunk(tokens, 0, True, speed)
            return

        caller = torch.cuda.current_stream(dev)      # the request stays on the stream it started on
        if llm_stream is not None:
            # the prompt, the embedding and the decode session's buffers were last touched on the caller's stream
            llm_stream.wait_stream(caller)
            for t in (text, p_tok, p_text, emb):
                t.record_stream(llm_stream)
        tokens: List[int] = []
        llm_done = False
        timing = dict(chunks=0, tokens_during_synthesis=0, llm_s=0.0, enqueue_s=0.0, drain_s=0.0)
        self.last_timing = timing

        def pull() -> bool:
            """one more token from the LLM, decoded on its own stream; False when it has finished."""
            nonlocal llm_done
            t0 = time.perf_counter()
            try:
                if llm_stream is None:
                    tokens.append(next(tokens_it))
                else:
                    with torch.cuda.stream(llm_stream):
                        tokens.append(next(tokens_it))
            except StopIteration:
                llm_done = True
            timing['llm_s'] += time.perf_counter() - t0
            return not llm_done

        def synthesise(window, i, finalize):
            """enqueue one chunk on the caller's stream; -> (item, event recorded behind it)"""
            t0 = time.perf_counter()
            with torch.cuda.stream(caller):
                item = chunk(window, i, finalize)
                ready = torch.cuda.Event()
                ready.record(caller)
            t1 = time.perf_counter()
            timing['enqueue_s'] += t1 - t0                           # host time until token2wav has returned
            return item, (ready, t1)

        def drain(mark):
            ready, t1 = mark
            ready.synchronize()
            timing['drain_s'] += time.perf_counter() - t1            # how long the device still worked after that
            timing['chunks'] += 1

        try:
            base, hop, ov, i = 0, self.token_min_hop_len, self.token_overlap_len, 0
            while True:
                while not llm_done and len(tokens) - base < hop + ov:
                    pull()
                if len(tokens) - base < hop + ov:
                    break
                item, ready = synthesise(tokens[base:base + hop + ov], i, False)
                # keep decoding while the chunk is synthesised; the chunk is yielded once it is complete or the LLM is done
                while not llm_done and not ready[0].query():
                    if pull():
                        timing['tokens_during_synthesis'] += 1
                drain(ready)
                yield item
                base += hop
                hop = min(self.token_max_hop_len, int(hop * self.stream_scale_factor))
                i += 1
            if not tokens:
                raise RuntimeError("the LLM produced no speech tokens")
            item, ready = synthesise(tokens[base:], i, True)
            drain(ready)
            yield item
        finally:
            if hasattr(tokens_it, 'close'):
                tokens_it.close()                      # an abandoned request: the LLM's generator ends here, not at collection
            if llm_stream is not None:
                # whatever the LLM stream still runs (an abandoned request too) is ordered before the caller's next work:
                # the decode session's buffers and the module caches are shared with non-streaming calls on that stream
                caller.wait_stream(llm_stream)

    # ------------------------------------------------------------------ many requests
    @torch.no_grad()
    def serve(self, requests, *, rows: int = 8, prefill_rows: Optional[int] = None, use_graph: bool = True,
              max_cache: int = 2048) -> Iterator[Tuple[object, dict]]:
        """Streamed synthesis of many requests at once: their LLM decodes share one ``DecodeServer`` (continuous batching,
        `rows` requests per decode step, queued ones admitted as rows fall free) on the LLM stream, while each request's
        chunks are cut by tts's own rule and run through token2wav on the caller's stream, one chunk at a time (the Flow and
        the vocoder are not batched across requests).  Yields (key, item): tts's items plus 'final': bool, each request's
        chunks in order and equal to ``tts(stream=True)`` of that request alone under the same seed / noise / hift pins.
        A request whose LLM fails yields {'error': exception, 'final': True} and the others go on.

        requests: an iterable of dicts with tts's keywords (text_tokens, prompt_wav, prompt_rate, prompt_speech_token,
        prompt_text, embedding, prompt_feat, seed, noise, hift_seed, hift_draws, hift_dtype, want_pcm, adapter, llm_kw) and
        an optional 'key' (default: its index).  It may be a generator: it is polled between decode steps, so requests
        can arrive while others run; yielding None means "nothing now".  With an AdapterBank over the models every request
        names its `adapter` (adapters.BASE for none).  max_cache: prompt rows + max_len a request's LLM decode may need."""
        dev = self.flow.input_embedding.weight.device
        caller = torch.cuda.current_stream(dev)
        llm_stream = self.llm_stream(dev)
        banked = "_cvft_adapter_bank" in self.llm.__dict__
        skey = (rows, prefill_rows, banked, max_cache)
        srv = self._servers.get(skey)
        if srv is None:
            self._servers.clear()                  # one server's caches at a time
            srv = self._servers[skey] = self.llm.decode_server(rows=rows, max_cache=max_cache, prefill_rows=prefill_rows,
                                                               adapters=banked)
        it = iter(requests)
        exhausted = False
        live: Dict[int, dict] = {}                 # rid -> request state, in arrival order
        index = 0
        flight = None                              # the chunk on the caller's stream: (request, item, event)

        def take(q: dict) -> None:
            nonlocal index
            q = dict(q)
            key = q.pop("key", index)
            index += 1
            unknown = set(q) - SERVE_KEYS
            if unknown:
                raise ValueError(f"serve: unknown request fields {sorted(unknown)} (a request is streamed at speed 1 from text)")
            adapter = q.get("adapter")
            if q.get("text_tokens") is None:
                raise ValueError("serve: every request needs text_tokens")
            p_tok, p_text, emb, p_feat = self._prompt(dev, q.get("prompt_wav"), q.get("prompt_rate"),
                                                      q.get("prompt_speech_token"), q.get("prompt_text"), q.get("embedding"))
            if q.get("prompt_feat") is not None:
                p_feat = q["prompt_feat"].float().to(dev)
            # the request's lm_input rows are built on the caller's stream, in order with the chunks: both go through
            # the modules an adapter is written into
            rid = srv.submit(torch.as_tensor(q["text_tokens"], dtype=torch.long).reshape(-1).to(dev), embedding=emb,
                             prompt_text=p_text, prompt_speech_token=p_tok, seed=q.get("seed"),
                             **({} if adapter is None else {"adapter": adapter}), **(q.get("llm_kw") or {}))
            x = srv.req[rid].get("x")
            if x is not None:
                x.record_stream(llm_stream)
            llm_stream.wait_stream(caller)
            live[rid] = dict(key=key, q=q, adapter=adapter, p_tok=p_tok, p_feat=p_feat, emb=emb, tokens=[], done=False,
                             error=None, base=0, hop=self.token_min_hop_len, i=0, state=StreamState())

        def poll() -> None:
            nonlocal exhausted
            while not exhausted and srv.pending() < 2 * rows:
                try:
                    q = next(it)
                except StopIteration:
                    exhausted = True
                    return
                if q is None:
                    return
                take(q)

        def ready(r: dict) -> Optional[bool]:
            """None: nothing to synthesise yet; else whether the next chunk is the final one."""
            if len(r["tokens"]) - r["base"] >= r["hop"] + self.token_overlap_len:
                return False
            return True if r["done"] else None

        def synthesise(r: dict, finalize: bool):
            q, i = r["q"], r["i"]
            noise, draws, hseed = q.get("noise"), q.get("hift_draws"), q.get("hift_seed")
            window = r["tokens"][r["base"]:] if finalize else r["tokens"][r["base"]:r["base"] + r["hop"] + self.token_overlap_len]
            if r["adapter"] is not None:
                from .inference_joint import activate_adapter
                activate_adapter(self.llm, self.flow, r["adapter"])
            taps = {} if q.get("want_pcm") else None
            wav = self.token2wav(r["state"], torch.tensor([window], dtype=torch.long), r["p_tok"], r["p_feat"], r["emb"],
                                 finalize, noise=noise[i] if isinstance(noise, (list, tuple)) else noise,
                                 hift_draws=draws[i] if isinstance(draws, list) else draws,
                                 hift_seed=None if hseed is None else hseed + i, hift_dtype=q.get("hift_dtype"),
                                 want_pcm=bool(q.get("want_pcm")), taps=taps)
            item = {"tts_speech": wav, "final": finalize}
            if taps is not None:
                item["pcm"] = taps["pcm"]
            ev = torch.cuda.Event()
            ev.record(caller)
            r["base"] += r["hop"]
            r["hop"] = min(self.token_max_hop_len, int(r["hop"] * self.stream_scale_factor))
            r["i"] += 1
            return item, ev

        try:
            llm_stream.wait_stream(caller)
            while True:
                poll()
                if srv.pending() or srv.events:
                    with torch.cuda.stream(llm_stream):
                        events = srv.step(use_graph)
                    for rid, tok, fin in events:
                        r = live[rid]
                        if tok is not None:
                            r["tokens"].append(tok)
                        if fin:
                            r["done"] = True
                            try:
                                srv.result(rid)
                            except RuntimeError as e:
                                r["error"] = e
                            if not r["tokens"] and r["error"] is None:
                                r["error"] = RuntimeError("the LLM produced no speech tokens")
                if flight is not None and (flight[2].query() or not srv.pending()):
                    r, item, ev = flight
                    ev.synchronize()
                    flight = None
                    yield r["key"], item
                if flight is None:
                    for rid, r in list(live.items()):
                        if r["error"] is not None:
                            del live[rid]
                            yield r["key"], {"error": r["error"], "final": True}
                            continue
                        fin = ready(r)
                        if fin is None:
                            continue
                        item, ev = synthesise(r, fin)
                        flight = (r, item, ev)
                        if fin:
                            del live[rid]
                        break
                if flight is None and not live and exhausted and not srv.pending():
                    return
        finally:
            for rid, r in live.items():
                if not r["done"]:
                    srv.cancel(rid)
            caller.wait_stream(llm_stream)
