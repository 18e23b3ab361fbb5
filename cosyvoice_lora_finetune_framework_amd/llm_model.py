"""Text-token LLM (text -> speech-token LM) on the HIP path.

``TransformerLM`` keeps the attribute names / state-dict keys of the vendored
cosyvoice/llm/llm.py:32-95 that ``JointLLMFlowModel._forward_llm`` consumes
(llm_flow_model.py:118-179): text_embedding, text_encoder, text_encoder_affine_layer,
llm_embedding, llm, llm_decoder, speech_embedding, spk_embed_affine_layer, sos_eos, task_id,
speech_token_size.  Built: the training forward (no-prompt) and the autoregressive generation of
llm.py:147-228 (``sampling_ids`` / ``inference``, plus the batched ``inference_batch``) on the decode kernels of
decode.py / csrc/decode.hip.  Qwen2LM / bistream inference are out of scope.

MI355X-first: the ragged ``[sos, spk, text, task, speech]`` concat + ``-1`` padding
(llm.py:88-95) is ONE row-gather kernel driven by an index map computed on the host from the
CPU-side length vectors (no device sync); the LM target never leaves int32 index form.
"""
from __future__ import annotations

import collections
import functools
from typing import Any, Dict, Generator, List, Optional, Sequence

import torch
import torch.nn as nn

from . import decode as DEC
from . import utils as U
from .config import LLM_MODEL_CONFIG
from .hipops import functional as HF
from .modules import Numerics, RelPosEncoder, _cached, hip_linear, to_len
from .utils import IGNORE_ID

MAX_TRIALS_MSG = ('sampling reaches max_trials {} and still get eos when ignore_eos is True, check your input!')


class TransformerLM(nn.Module):
    def __init__(self, text_encoder_input_size: int, llm_input_size: int, llm_output_size: int, text_token_size: int,
                 speech_token_size: int, text_encoder: nn.Module, llm: nn.Module, sampling=None,
                 length_normalized_loss: bool = True, lsm_weight: float = 0.0, spk_embed_dim: int = 192):
        super().__init__()
        if not length_normalized_loss:      # (denominator = batch size: the sub-batch / DP recombination is built on token counts)
            raise NotImplementedError("only the length-normalised CE (the CosyVoice-300M setting) is built")
        self.lsm_weight = float(lsm_weight)
        self.llm_input_size = llm_input_size
        self.speech_token_size = speech_token_size
        self.text_embedding = nn.Embedding(text_token_size, text_encoder_input_size)
        self.text_encoder = text_encoder
        self.text_encoder_affine_layer = nn.Linear(self.text_encoder.output_size(), llm_input_size)
        self.sos_eos = 0
        self.task_id = 1
        self.llm_embedding = nn.Embedding(2, llm_input_size)
        self.llm = llm
        self.llm_decoder = nn.Linear(llm_output_size, speech_token_size + 1)
        self.speech_embedding = nn.Embedding(speech_token_size, llm_input_size)
        self.spk_embed_affine_layer = nn.Linear(spk_embed_dim, llm_input_size)
        self.sampling = sampling
        self.numerics = Numerics()

    def _table(self, emb: nn.Embedding, dtype):
        w = emb.weight
        return w.detach() if w.dtype == dtype else _cached(emb, "tab", w, dtype, lambda: w.detach().to(dtype))

    @staticmethod
    def build_index_maps(text_len, speech_len, speech_token, B: int, Lx: int, Lt: int, eos: int, pad_to: int = 1, L_min: int = 0):
        """Host-side (CPU tensors only) ragged layout of llm.py:88-95 + llm_flow_model.py:129-139.
        Source rows: [sos, task | spk(B) | text(B*Lx) | speech(B*Lt)].  Returns (idx [B*L] int32,
        target [B*L] int32, lm_len [B] int32, L).  pad_to > 1 rounds L up (rows past an utterance's length are the
        reference's -1 padding either way: masked keys, ignored targets), so that steps of nearby lengths share one
        captured hipGraph."""
        tl = [int(v) for v in text_len.tolist()]
        sl = [int(v) for v in speech_len.tolist()]
        lens = [3 + a + b for a, b in zip(tl, sl)]
        L = max(-(-max(lens) // pad_to) * pad_to, L_min)              # (L_min: the LM length of the captured step this batch joins)
        idx = torch.full((B, L), -1, dtype=torch.int32)
        tgt = torch.full((B, L), IGNORE_ID, dtype=torch.int32)
        st = speech_token.to(torch.int32)
        for i in range(B):
            a, b = tl[i], sl[i]
            idx[i, 0] = 0
            idx[i, 1] = 2 + i
            idx[i, 2:2 + a] = torch.arange(2 + B + i * Lx, 2 + B + i * Lx + a, dtype=torch.int32)
            idx[i, 2 + a] = 1
            idx[i, 3 + a:3 + a + b] = torch.arange(2 + B + B * Lx + i * Lt, 2 + B + B * Lx + i * Lt + b, dtype=torch.int32)
            # target: IGNORE * (2 + text) , speech tokens, EOS   (position 2+a .. 2+a+b)
            tgt[i, 2 + a:2 + a + b] = st[i, :b]
            tgt[i, 2 + a + b] = eos
        return idx.reshape(-1), tgt.reshape(-1), torch.tensor(lens, dtype=torch.int32), L

    def forward_no_prompt(self, batch: dict, device) -> Dict[str, Any]:
        """llm_flow_model.py:109-179."""
        num = self.numerics
        dt = num.dtype
        text = batch['text_token']
        B, Lx = text.shape
        sp = batch['speech_token']
        Lt = sp.shape[1]
        if '_lm_maps' in batch:                       # prepared once on the host (prepare_batch): no sync, graph-safe
            idx, tgt, lm_len, L = batch['_lm_maps']
        else:
            idx, tgt, lm_len, L = self.build_index_maps(batch['text_token_len'].cpu(), batch['speech_token_len'].cpu(),
                                                        sp.cpu(), B, Lx, Lt, self.speech_token_size)
            idx, tgt, lm_len = idx.to(device), tgt.to(device), lm_len.to(device)
        text_len = to_len(batch['text_token_len'], device)
        with torch.no_grad():
            temb = HF.embed_gather(text.to(device), self._table(self.text_embedding, dt))
            semb = HF.embed_gather(sp.to(device), self._table(self.speech_embedding, dt))
            spk = hip_linear(self.spk_embed_affine_layer, HF.l2norm_rows(batch['embedding'].to(device), dt))
            special = self._table(self.llm_embedding, dt)
        enc = self.text_encoder.forward_cl(temb, B, Lx, text_len, num, causal=True)   # encode(): decoding_chunk_size=1
        enc = hip_linear(self.text_encoder_affine_layer, enc)
        src = torch.cat([special, spk, enc, semb], dim=0)
        lm_in = HF.gather_rows(src, idx, float(IGNORE_ID))
        out = self.llm.forward_cl(lm_in, B, L, lm_len, num, causal=True)
        logits = hip_linear(self.llm_decoder, out)
        loss, acc = HF.cross_entropy(logits, tgt, self.lsm_weight)
        return {'loss': loss, 'acc': acc}

    def forward(self, batch: dict, device) -> Dict[str, Any]:
        return self.forward_no_prompt(batch, device)

    def prepare_batch(self, batch: dict, device, lm_pad: int = 1, lm_min: int = 0) -> dict:
        """Host-side preparation of one batch: index maps + H2D copies, done once per batch outside the
        (graph-capturable) step."""
        B, Lx = batch['text_token'].shape
        Lt = batch['speech_token'].shape[1]
        idx, tgt, lm_len, L = self.build_index_maps(batch['text_token_len'].cpu(), batch['speech_token_len'].cpu(),
                                                    batch['speech_token'].cpu(), B, Lx, Lt, self.speech_token_size, lm_pad, lm_min)
        return {'_lm_maps': (idx.to(device), tgt.to(device), lm_len.to(device), L)}


    # ------------------------------------------------------------------ autoregressive generation (llm.py:147-228)
    def sampling_ids(self, weighted_scores: torch.Tensor, decoded_tokens: List, sampling: int, ignore_eos: bool = True):
        """Host form of llm.py:147-163: re-draw while the draw is EOS and ignore_eos, at most 100 re-draws."""
        fn = self.sampling if self.sampling is not None else U.ras_sampling
        trials = 0
        while True:
            top_ids = fn(weighted_scores, decoded_tokens, sampling)
            if (not ignore_eos) or (self.speech_token_size not in top_ids):
                return top_ids
            trials += 1
            if trials > 100:
                raise RuntimeError(MAX_TRIALS_MSG.format(100))

    def sampler_cfg(self) -> Optional[DEC.SamplerCfg]:
        """The device sampler's parameters for ``self.sampling``, or None when it must be called on the host: None ->
        ras_sampling defaults; a functools.partial of utils.ras_sampling / nucleus_sampling / random_sampling (keyword
        parameters, top_k <= 64, win_size <= 64) -> that sampler on the device; anything else -> the host."""
        s = self.sampling
        if s is None:
            return DEC.SamplerCfg("ras")
        if not isinstance(s, functools.partial) or s.args:
            return None
        kw = dict(s.keywords)
        if s.func is U.ras_sampling and set(kw) <= {"top_p", "top_k", "win_size", "tau_r"}:
            cfg = DEC.SamplerCfg("ras", **kw)
        elif s.func is U.nucleus_sampling and set(kw) <= {"top_p", "top_k"}:
            cfg = DEC.SamplerCfg("nucleus", **kw)
        elif s.func is U.random_sampling and not kw:
            cfg = DEC.SamplerCfg("random")
        else:
            return None
        if cfg.mode != "random" and not (1 <= cfg.top_k <= 64 and cfg.top_p > 0 and 0 <= cfg.win <= DEC.HIST):
            return None
        return cfg

    def lm_input_rows(self, text, text_len, prompt_text, prompt_text_len, prompt_speech_token, prompt_speech_token_len,
                      embedding):
        """llm.py:181-210 for one request -> (lm_input rows [T0, llm_input_size] fp32, text length without the prompt)."""
        dev = self.llm_decoder.weight.device
        num, dt = self.numerics, self.numerics.dtype
        text = torch.cat([prompt_text.reshape(1, -1).to(dev), text.reshape(1, -1).to(dev)], dim=1)
        Lx = text.shape[1]
        n_text = int(text_len) if not torch.is_tensor(text_len) else int(text_len.reshape(-1)[0])
        n_prompt = int(prompt_text_len) if not torch.is_tensor(prompt_text_len) else int(prompt_text_len.reshape(-1)[0])
        with torch.no_grad():
            temb = HF.embed_gather(text, self._table(self.text_embedding, dt))
            enc = self.text_encoder.forward_cl(temb, 1, Lx, to_len(torch.tensor([Lx]), dev), num, causal=True)
            enc = hip_linear(self.text_encoder_affine_layer, enc).float()
            parts = [self.llm_embedding.weight[self.sos_eos].detach().float().reshape(1, -1)]
            if embedding is not None and embedding.shape[0] != 0:
                parts.append(hip_linear(self.spk_embed_affine_layer, HF.l2norm_rows(embedding.to(dev), dt)).float())
            parts += [enc, self.llm_embedding.weight[self.task_id].detach().float().reshape(1, -1)]
            n_ps = int(prompt_speech_token_len) if not torch.is_tensor(prompt_speech_token_len) else \
                int(prompt_speech_token_len.reshape(-1)[0])
            if n_ps != 0:
                parts.append(self.speech_embedding.weight.detach().float()[prompt_speech_token.reshape(-1)[:n_ps].to(dev)])
        return torch.cat(parts, dim=0).contiguous(), n_text

    MAX_SESSIONS = 4

    def decode_session(self, B: int, cap: int, bank=None) -> "DEC.LMDecodeSession":
        """The weights are packed once per weight dtype (rebuilt when a parameter changes) and shared by the sessions;
        sessions (K/V caches, positional tables, captured step) are kept per (batch, capacity bucket, dtype), the
        MAX_SESSIONS most recently used ones.  bank (adapters.AdapterBank): the unfolded pack (W alone, rebuilt only when
        a parameter other than the ``lora_`` ones changes) and sessions that read each row's adapter from the bank's
        stacks -- loading, evicting or activating adapters leaves both, and their captured steps, as they are."""
        cap = DEC.bucket(cap)
        fold = bank is None
        dtype = self.numerics.dtype
        sessions = self.__dict__.setdefault("_cvft_sessions", collections.OrderedDict())
        tag = None if fold else id(bank)
        pk = self._decode_pack(fold)
        ver = pk[0]
        key = (B, cap, dtype) if fold else (B, cap, dtype, tag)
        hit = sessions.get(key)
        if hit is None:
            stacks = None if fold else bank.stacks(pk[1].wdtype)
            hit = sessions[key] = (ver, DEC.LMDecodeSession(pk[1], B, cap, bank=stacks))
            while len(sessions) > self.MAX_SESSIONS:
                sessions.popitem(last=False)
        sessions.move_to_end(key)
        return hit[1]

    def _decode_version(self, fold: bool):
        return tuple(p._version for n, p in self.named_parameters() if fold or 'lora_' not in n)

    def _decode_pack(self, fold: bool):
        """(parameter versions, the PackedLM) of the current weight dtype, shared by every session and server; repacked
        (and the LRU sessions over the old pack dropped) when a parameter it depends on has changed."""
        ver = self._decode_version(fold)
        dtype = self.numerics.dtype
        packs = self.__dict__.setdefault("_cvft_decode_weights", {})
        sessions = self.__dict__.setdefault("_cvft_sessions", collections.OrderedDict())
        pkey = dtype if fold else (dtype, "unfolded")
        pk = packs.get(pkey)
        if pk is None or pk[0] != ver:
            for k in [k for k in sessions if k[2] == dtype and (len(k) == 3) == fold]:
                del sessions[k]
            packs[pkey] = pk = (ver, DEC.PackedLM(self, fold=fold))
        return pk

    def decode_server(self, rows: int = 8, max_cache: int = 1024, prefill_rows: Optional[int] = None,
                      adapters: bool = False) -> "DecodeServer":
        """Continuous batching: a DecodeServer that decodes up to `rows` requests at once and admits queued ones into
        rows as they fall free (see DecodeServer).  max_cache: prompt rows + max_len every request must fit in.
        prefill_rows: None takes DEFAULT_PREFILL_ROWS; 0 prefills an admitted request between two decode steps, n > 0
        carries n of its prompt rows along with each decode step (rows + n <= 16).  adapters=True decodes the base
        weights with each request's adapter of the model's AdapterBank."""
        return DecodeServer(self, rows, max_cache, DEFAULT_PREFILL_ROWS if prefill_rows is None else prefill_rows, adapters)

    def _request_seed(self) -> int:
        # one draw of torch's default generator per request (torch.manual_seed makes a run reproducible)
        return int(torch.randint(0, 2 ** 62, (1,), device=self.llm_decoder.weight.device).item())

    @torch.no_grad()
    def inference(self, text: torch.Tensor, text_len: torch.Tensor, prompt_text: torch.Tensor,
                  prompt_text_len: torch.Tensor, prompt_speech_token: torch.Tensor, prompt_speech_token_len: torch.Tensor,
                  embedding: torch.Tensor, sampling: int = 25, max_token_text_ratio: float = 20,
                  min_token_text_ratio: float = 2, uuid: str = '', use_graph: bool = True, seed: Optional[int] = None,
                  uniforms: Optional[torch.Tensor] = None, adapter=None) -> Generator[int, None, None]:
        """llm.py:165-228: yields speech-token ids until EOS (not yielded) or max_len.  `text_len` counts the text
        WITHOUT the prompt (the reference adds prompt_text_len).  Extra keywords: use_graph=False runs the same
        kernels without capture; seed / uniforms pin the sampler's draws (default: one seed per request drawn from
        torch's generator).  adapter: None decodes the module's own (merged) weights; a name resident in the model's
        adapters.AdapterBank, or adapters.BASE, decodes the base weights with that adapter (the text encoder's LoRA
        parameters are set to it first).  The adapter must stay resident until the generator ends."""
        bank, slots = self._adapter_slots([adapter]) if adapter is not None else (None, None)
        rows, n_text = self.lm_input_rows(text, text_len, prompt_text, prompt_text_len, prompt_speech_token,
                                          prompt_speech_token_len, embedding)
        min_len, max_len = int(n_text * min_token_text_ratio), int(n_text * max_token_text_ratio)
        if max_len <= 0:
            return
        cfg = self.sampler_cfg()
        sess = self.decode_session(1, rows.shape[0] + max_len, bank=bank)
        if cfg is None:
            yield from self._inference_host(sess, rows, min_len, max_len, sampling, use_graph, slots)
            return
        sess.start([rows], [min_len], [max_len], [self._request_seed() if seed is None else seed], cfg,
                   uniforms=uniforms, slots=slots)
        while True:
            tok, done, err = sess.read()
            if err[0]:
                raise RuntimeError(MAX_TRIALS_MSG.format(100))
            if tok[0] == self.speech_token_size:
                return
            yield tok[0]
            if done[0]:
                return
            sess.advance(use_graph)

    def _adapter_slots(self, adapters, activate: bool = True):
        """(the model's AdapterBank, each request's decode slot); with one request its adapter is also activated."""
        from .adapters import bank_of
        bank = bank_of(self)
        slots = [bank.slot(a) for a in adapters]
        if activate and len(adapters) == 1:
            bank.activate(adapters[0])
        return bank, slots

    def _inference_host(self, sess, rows, min_len, max_len, sampling, use_graph, slots=None):
        """an arbitrary ``self.sampling`` callable: device logits / log_softmax, the draw on the host per step."""
        sess.start([rows], [0], [max_len], [0], DEC.SamplerCfg("logp"), slots=slots)
        out: List[int] = []
        for i in range(max_len):
            logp = sess.logp[0].clone()
            if i == 0:
                logp[self.speech_token_size] = -float('inf')
            top = int(self.sampling_ids(logp, out, sampling, ignore_eos=i < min_len))
            if top == self.speech_token_size:
                return
            yield top
            out.append(top)
            if i + 1 == max_len:
                return
            sess.next_in.fill_(top)
            sess.advance(use_graph)
            sess.stack.len.add_(1)

    @torch.no_grad()
    def inference_batch(self, texts: Sequence[torch.Tensor], embeddings: Optional[Sequence[torch.Tensor]] = None,
                        prompt_texts: Optional[Sequence[torch.Tensor]] = None,
                        prompt_speech_tokens: Optional[Sequence[torch.Tensor]] = None,
                        seeds: Optional[Sequence[int]] = None, max_token_text_ratio: float = 20,
                        min_token_text_ratio: float = 2, use_graph: bool = True,
                        adapters: Optional[Sequence] = None) -> List[List[int]]:
        """Up to 16 requests (ragged) decoded in lockstep: each is prefilled into its own cache row, then every step
        streams the weights once for all rows; finished rows are skipped by the kernels.  Returns one token list per
        request, equal to what ``inference`` yields for that request with the same seed.  adapters: one name (or
        adapters.BASE) per request, as ``inference(adapter=)``: the base weights are streamed once and every row adds its
        own adapter; None decodes the module's own (merged) weights."""
        B = len(texts)
        assert 1 <= B <= 16, "inference_batch: 1 .. 16 requests"
        bank, slots = (None, None)
        if adapters is not None:
            assert len(adapters) == B, "inference_batch: one adapter per request"
            bank, slots = self._adapter_slots(list(adapters), activate=False)
        cfg = self.sampler_cfg()
        if cfg is None:
            raise NotImplementedError("inference_batch runs the device sampler only (see sampler_cfg)")
        z = torch.zeros(0, dtype=torch.long)
        rows, mins, maxs = [], [], []
        for b in range(B):
            pt = prompt_texts[b] if prompt_texts is not None else z
            ps = prompt_speech_tokens[b] if prompt_speech_tokens is not None else z
            emb = embeddings[b] if embeddings is not None else torch.zeros(1, 192)
            if bank is not None:
                bank.activate(adapters[b])             # the text encoder runs through its modules: this request's adapter
            r, n = self.lm_input_rows(texts[b].reshape(-1), texts[b].numel(), pt.reshape(-1), pt.numel(),
                                      ps.reshape(-1), ps.numel(), emb.reshape(1, -1) if emb.numel() else emb)
            rows.append(r)
            mins.append(int(n * min_token_text_ratio))
            maxs.append(max(int(n * max_token_text_ratio), 0))
        seeds = [self._request_seed() for _ in range(B)] if seeds is None else list(seeds)
        outs: List[List[int]] = [[] for _ in range(B)]
        if max(maxs) <= 0:
            return outs
        sess = self.decode_session(B, max(r.shape[0] + m for r, m in zip(rows, maxs)), bank=bank)
        sess.start(rows, mins, [max(m, 1) for m in maxs], seeds, cfg, slots=slots)
        active = [m > 0 for m in maxs]
        while any(active):
            tok, done, err = sess.read()
            for b in range(B):
                if not active[b]:
                    continue
                if err[b]:
                    raise RuntimeError(MAX_TRIALS_MSG.format(100))
                if tok[b] != self.speech_token_size:
                    outs[b].append(tok[b])
                active[b] = not done[b]
            if any(active):
                sess.advance(use_graph)
        return outs


DEFAULT_PREFILL_ROWS = 0


class DecodeServer:
    """Continuous batching over one TransformerLM: up to `rows` requests decode in one step (the captured decode step of
    decode.LMDecodeSession), a queued request is admitted into a cache row as soon as one is free, and a finished row is
    retired at once.  Every request's tokens are those of ``TransformerLM.inference`` run alone with its seed.

    The server owns a private session over the model's shared packed weights (not one of ``decode_session``'s, which
    ``inference_batch`` resets).  submit() / step() work on the current stream.  While requests are in flight the
    weights must not change (RuntimeError; an idle server repacks), and an adapter must stay resident while a request
    that uses it is alive."""

    def __init__(self, lm: TransformerLM, rows: int, max_cache: int, prefill_rows: int, adapters: bool):
        DEC.check_serve_rows(rows, prefill_rows)
        self.lm, self.rows, self.prefill_rows, self.adapters = lm, int(rows), int(prefill_rows), bool(adapters)
        self.cap = DEC.bucket(max_cache)
        self.cfg = lm.sampler_cfg()
        if self.cfg is None:
            raise NotImplementedError("decode_server runs the device sampler only (see sampler_cfg)")
        self.sched = DEC.RowScheduler(self.rows, self.prefill_rows)
        self.req: Dict[int, dict] = {}                     # rid -> record; dropped by result() / cancel()
        self.by_row: Dict[int, int] = {}                   # decoding rows -> rid
        self.events: List[tuple] = []                      # finished without a step (max_len <= 0)
        self.next_rid = 0
        self.sess: Optional[DEC.LMDecodeSession] = None
        self._pack()

    # ---- weights
    def _pack(self):
        fold = not self.adapters
        self.bank = None
        stacks = None
        if self.adapters:
            from .adapters import bank_of
            self.bank = bank_of(self.lm)
        ver, pk = self.lm._decode_pack(fold)
        if self.bank is not None:
            stacks = self.bank.stacks(pk.wdtype)
        self._params = [p for n, p in self.lm.named_parameters() if fold or 'lora_' not in n]
        self._ver, self._dtype = ver, self.lm.numerics.dtype
        self.sess = DEC.LMDecodeSession(pk, self.rows, self.cap, bank=stacks, prefill_rows=self.prefill_rows)
        self.sess.idle(self.cfg)

    def _check_weights(self):
        if tuple(p._version for p in self._params) == self._ver and self.lm.numerics.dtype == self._dtype:
            return
        if self.pending():
            raise RuntimeError("decode_server: the model's weights changed while requests are in flight")
        self._pack()

    # ---- requests
    def pending(self) -> int:
        """requests queued, being prefilled or decoding."""
        return sum(1 for r in self.req.values() if r["state"] in ("queued", "running"))

    @torch.no_grad()
    def submit(self, text, *, embedding=None, prompt_text=None, prompt_speech_token=None, seed: Optional[int] = None,
               adapter=None, min_token_text_ratio: float = 2, max_token_text_ratio: float = 20) -> int:
        """Queue one request (``inference``'s operands: text without the prompt; embedding [1, 192] or None).  Its
        lm_input rows are built now, with `adapter` activated for the text encoder.  -> the request id."""
        self._check_weights()
        if (adapter is not None) != self.adapters:
            raise ValueError("decode_server: adapter= goes with decode_server(adapters=True), and every request of such a "
                             "server names one (adapters.BASE for none)")
        z = torch.zeros(0, dtype=torch.long)
        text = torch.as_tensor(text, dtype=torch.long).reshape(-1)
        pt = z if prompt_text is None else torch.as_tensor(prompt_text, dtype=torch.long).reshape(-1)
        ps = z if prompt_speech_token is None else torch.as_tensor(prompt_speech_token, dtype=torch.long).reshape(-1)
        emb = torch.zeros(1, 192) if embedding is None else embedding
        emb = emb.reshape(1, -1) if emb.numel() else emb
        n_text = text.numel()
        min_len, max_len = int(n_text * min_token_text_ratio), int(n_text * max_token_text_ratio)
        T = 2 + (1 if emb.shape[0] != 0 else 0) + pt.numel() + n_text + ps.numel()
        if max_len > 0 and T + max_len > self.cap:           # on the host, before anything is launched
            raise ValueError("decode capacity bucket too small")
        slot = None
        if self.adapters:
            slot = self.bank.slot(adapter)
        rid = self.next_rid
        self.next_rid += 1
        rec = self.req[rid] = dict(state="queued", tokens=[], row=None, first=False, error=False)
        if max_len <= 0:
            rec["state"] = "finished"
            self.events.append((rid, None, True))
            return rid
        if self.adapters:
            self.bank.activate(adapter)                       # the text encoder runs through its modules
        x, _ = self.lm.lm_input_rows(text, n_text, pt, pt.numel(), ps, ps.numel(), emb)
        assert x.shape[0] == T
        rec.update(x=x, min_len=min_len, max_len=max_len, slot=slot,
                   seed=self.lm._request_seed() if seed is None else int(seed))
        self.sched.submit(rid, T)
        return rid

    @torch.no_grad()
    def step(self, use_graph: bool = True) -> List[tuple]:
        """Admit the oldest queued request if a row is free, run one step (the captured decode step, or one that also
        carries prompt rows of the admission in flight), read the device once.  -> [(rid, token | None, finished), ...]
        of this step: one entry per decoding request; EOS is not emitted (token None, finished True).  A request whose
        row raised the sampler's error flag finishes alone with token None; result(rid) then raises."""
        self._check_weights()
        out, self.events = self.events, []
        if not self.sched.busy():
            return out
        sess, eos = self.sess, self.lm.speech_token_size
        p = self.sched.plan()
        if p["admit"] is not None:
            rid, row = p["admit"]
            r = self.req[rid]
            r["row"] = row
            r["state"] = "running"
            sess.admit(row, r.pop("x"), r["min_len"], r["max_len"], r["seed"], slot=r["slot"])
        sess.serve_step(sum(p["chunks"]), use_graph)
        if p["first"]:
            self.by_row[p["row"]] = p["rid"]
        if not self.by_row:
            return out
        tok, done, err = sess.read()
        for row, rid in sorted(self.by_row.items()):
            r = self.req[rid]
            if err[row]:
                r["error"] = True
                out.append((rid, None, True))
            elif tok[row] == eos:
                out.append((rid, None, True))
            else:
                r["tokens"].append(tok[row])
                out.append((rid, tok[row], bool(done[row])))
            if out[-1][2]:
                r["state"] = "finished"
                self._free(rid)
        return out

    def _free(self, rid: int):
        row = self.sched.release(rid)
        if row is not None:
            self.sess.retire(row)
            self.by_row.pop(row, None)

    def cancel(self, rid: int) -> None:
        """drop a request at any stage: a queued one leaves the queue, a running one frees its row for the next."""
        r = self.req.pop(rid)
        if r["state"] in ("queued", "running"):
            self._free(rid)

    def result(self, rid: int) -> List[int]:
        """the tokens of a finished request (its record is dropped); the reference's RuntimeError if its sampler kept
        drawing EOS before min_len."""
        r = self.req[rid]
        if r["state"] != "finished":
            raise RuntimeError(f"decode_server: request {rid} has not finished")
        del self.req[rid]
        if r["error"]:
            raise RuntimeError(MAX_TRIALS_MSG.format(100))
        return r["tokens"]

    def run(self, use_graph: bool = True) -> Dict[int, List[int]]:
        """step until nothing is pending; -> {rid: tokens} of every finished request that has not been collected (a
        failed one is left for result(rid) to raise)."""
        while self.pending():
            self.step(use_graph)
        self.events = []
        out = {}
        for rid in [k for k, r in self.req.items() if r["state"] == "finished" and not r["error"]]:
            out[rid] = self.result(rid)
        return out


def build_llm_model(pretrained_path: Optional[str] = None, device: str = 'cuda', numerics: Optional[Numerics] = None,
                    text_encoder_input_size: int = 512, llm_input_size: int = 1024, llm_output_size: int = 1024,
                    text_token_size: int = 51866, speech_token_size: int = 4096, spk_embed_dim: int = 192,
                    attention_heads: int = 16, linear_units: int = 4096, text_encoder_blocks: int = 6,
                    llm_blocks: int = 14) -> TransformerLM:
    """CosyVoice-300M TransformerLM (public upstream cosyvoice.yaml dims; config.LLM_MODEL_CONFIG)."""
    numerics = numerics or Numerics()
    te = RelPosEncoder(input_size=text_encoder_input_size, output_size=llm_input_size, attention_heads=attention_heads,
                       linear_units=linear_units, num_blocks=text_encoder_blocks, dropout_rate=0.1,
                       positional_dropout_rate=0.1, attention_dropout_rate=0.0, input_layer="linear", kind="conformer",
                       static_chunk_size=1, ln_eps=numerics.enc_ln_eps)
    lm = RelPosEncoder(input_size=llm_input_size, output_size=llm_output_size, attention_heads=attention_heads,
                       linear_units=linear_units, num_blocks=llm_blocks, dropout_rate=0.1, positional_dropout_rate=0.1,
                       attention_dropout_rate=0.0, input_layer="linear_legacy", kind="transformer", static_chunk_size=1,
                       ln_eps=numerics.enc_ln_eps)
    model = TransformerLM(text_encoder_input_size, llm_input_size, llm_output_size, text_token_size, speech_token_size,
                          te, lm, sampling=None, length_normalized_loss=True, lsm_weight=0.0, spk_embed_dim=spk_embed_dim)
    model.numerics = numerics
    if pretrained_path is not None:
        import os
        wf = os.path.join(pretrained_path, 'llm.pt') if os.path.isdir(pretrained_path) else pretrained_path
        if os.path.exists(wf):
            model.load_state_dict(torch.load(wf, map_location='cpu', weights_only=True), strict=True)
        else:
            print(f"Warning: Weight file not found: {wf}\nUsing random initialization")
    return model.to(device)
