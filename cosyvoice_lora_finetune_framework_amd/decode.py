"""Autoregressive speech-token generation on HIP (TransformerLM.inference, llm.py:165-228).

A decode session packs the LM's weights once (LoRA folded: W + s*B@A, the merged weights the reference's inference
consumes; fp32 or bf16 per ``numerics.dtype``), builds each layer's relative-position table ``P[d] = linear_pos(pe_d)``
for the distances d >= 0 once, and owns fp32 K/V caches of a fixed capacity bucket.  Every step runs the csrc/decode.hip
kernels: the M <= 16 weight-streaming linear (LayerNorm prologue, bias / ReLU / residual epilogues), the split-key
rel-pos attention that appends the new rows' K/V in place, and the fused sampler that writes the next token, the
per-row length, step and done flags on the device.  So one decode step reads nothing from the host and is captured
once as a hipGraph per (batch, capacity) on one stream; the host reads tokens + done flags after each replay.

Prefill runs through the same kernels in chunks of <= 16 rows (the causal attention of a chunk against the cache is
exactly the reference's full causal prefill).  The text encoder still runs through the training forward
(``RelPosEncoder.forward_cl``), like ``TransformerLM.encode`` with decoding_chunk_size=1.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from .hipops import functional as HF
from .hipops.binding import BF16, F32, check, lib, ptr, stream
from .modules import _lin_parts

ATT_KEYS = 256        # keys per attention workgroup (csrc/decode.hip)
MAX_ROWS = 16         # rows per decode-linear / attention launch
TRIALS = 101          # sampler draws per step before the EOS error (llm.py:147-163)
HIST = 64             # history ring per row (win_size <= 64)
MODES = {"ras": 0, "nucleus": 1, "random": 2, "logp": 3}


# ---------------------------------------------------------------------------------------------- ops
def decode_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, ln=None, act: int = 0,
                  residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [M <= 16, K] fp32, w [N, K] fp32 | bf16 -> act(LN?(x) w^T + bias) (+ residual); ln = (gamma, beta, eps)."""
    M, K = x.shape
    N = w.shape[0]
    assert x.dtype == torch.float32 and x.stride(1) == 1 and w.is_contiguous() and w.shape[1] == K
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    check(lib().cvft_decode_linear(F32 if w.dtype == torch.float32 else BF16, M, N, K, ptr(x), x.stride(0), ptr(g), ptr(b),
                                   float(eps), ptr(w), ptr(bias), act, ptr(residual),
                                   residual.stride(0) if residual is not None else 0, ptr(out), out.stride(0), stream()),
          "cvft_decode_linear")
    return out


def decode_lora_down(x: torch.Tensor, A: torch.Tensor, slot: torch.Tensor, ln=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [M <= 16, K] fp32, A [S, G, R, K] fp32 | bf16 (the adapters' lora_A, stacked), slot [M] int32 (device)
    -> z [M, G*R] fp32: LN?(x) against each row's own adapter; rows whose slot is outside [0, S) get zeros."""
    M, K = x.shape
    S, G, R = A.shape[:3]
    assert x.dtype == torch.float32 and x.stride(1) == 1 and A.is_contiguous() and A.shape[3] == K
    assert slot.dtype == torch.int32 and slot.is_contiguous() and slot.numel() >= M
    if out is None:
        out = torch.empty((M, G * R), dtype=torch.float32, device=x.device)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    check(lib().cvft_decode_lora_down(F32 if A.dtype == torch.float32 else BF16, M, K, S, G, R, ptr(x), x.stride(0), ptr(g),
                                      ptr(b), float(eps), ptr(A), ptr(slot), ptr(out), out.stride(0), stream()),
          "cvft_decode_lora_down")
    return out


def decode_linear_lora(x: torch.Tensor, w: torch.Tensor, Bst: torch.Tensor, scale: torch.Tensor, slot: torch.Tensor,
                       z: torch.Tensor, G: int = 1, bias: Optional[torch.Tensor] = None, ln=None, act: int = 0,
                       residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """decode_linear plus each row's adapter: act(LN?(x) w^T + bias + scale[s] * Bst[s] z_g) (+ residual), s = slot[m],
    z [M, >= G*R] from decode_lora_down, Bst [S, N, R] in w's dtype, scale [S] fp32.  Rows without adapter: decode_linear."""
    M, K = x.shape
    N = w.shape[0]
    S, _, R = Bst.shape
    assert x.dtype == torch.float32 and x.stride(1) == 1 and w.is_contiguous() and w.shape[1] == K
    assert Bst.is_contiguous() and Bst.shape[1] == N and Bst.dtype == w.dtype and scale.numel() == S
    assert scale.dtype == torch.float32 and slot.dtype == torch.int32 and slot.numel() >= M
    assert z.dtype == torch.float32 and z.stride(1) == 1 and z.shape[0] >= M and z.shape[1] >= G * R
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    check(lib().cvft_decode_linear_lora(F32 if w.dtype == torch.float32 else BF16, M, N, K, ptr(x), x.stride(0), ptr(g),
                                        ptr(b), float(eps), ptr(w), ptr(bias), act, ptr(residual),
                                        residual.stride(0) if residual is not None else 0, ptr(out), out.stride(0), S, G, R,
                                        ptr(Bst), ptr(scale), ptr(slot), ptr(z), z.stride(0), stream()),
          "cvft_decode_linear_lora")
    return out


def decode_attn(qkv, kc, vc, length, P, pos_bias_u, pos_bias_v, B: int, H: int, Lq: int, done=None, part=None,
                out=None) -> torch.Tensor:
    """qkv [B*Lq, >= 3*H*64] (q | k | v of the new rows), kc / vc [B, H, cap, 64] fp32 (appended in place at length[b]),
    length [B] int32 (device), P [>= cap, H*64] -> o [B*Lq, H*64]."""
    cap = kc.shape[2]
    nsplit = -(-cap // ATT_KEYS)
    D = H * 64
    if part is None:
        part = torch.empty(B * H * nsplit * Lq * 66, dtype=torch.float32, device=qkv.device)
    if out is None:
        out = torch.empty((B * Lq, D), dtype=torch.float32, device=qkv.device)
    assert P.shape[0] >= cap and kc.is_contiguous() and vc.is_contiguous() and part.numel() >= B * H * nsplit * Lq * 66
    check(lib().cvft_decode_attn(B, H, Lq, cap, nsplit, ptr(qkv), qkv.stride(0), ptr(kc), ptr(vc), ptr(length), ptr(done),
                                 ptr(P), P.stride(0), ptr(pos_bias_u), ptr(pos_bias_v), 1.0 / math.sqrt(64.0), ptr(part),
                                 ptr(out), out.stride(0), stream()), "cvft_decode_attn")
    return out


def _layernorm(x, g, b, eps, out, mean, rstd, relu=False, post_scale=1.0):
    check(lib().cvft_layernorm_fwd(F32, x.shape[0], x.shape[1], ptr(x), ptr(g), ptr(b), float(eps), int(relu),
                                   float(post_scale), ptr(out), ptr(mean), ptr(rstd), stream()), "cvft_layernorm_fwd")
    return out


# ---------------------------------------------------------------------------------------------- weights
def merged_weight(mod, wdtype):
    """(W [out, in] in wdtype with the LoRA product folded, bias fp32 or None) of an nn.Linear / LoRALinear."""
    _, w, b, A, Bm, scale, _ = _lin_parts(mod)
    W = w.detach().float()
    if A is not None:
        W = W + float(scale) * (Bm.detach().float() @ A.detach().float())
    return W.to(wdtype).contiguous(), (b.detach().float().contiguous() if b is not None else None)


def base_weight(mod, wdtype):
    """(W, bias) like merged_weight but of the frozen layer alone: the unfolded pack an AdapterBank decodes against."""
    _, w, b, _, _, _, _ = _lin_parts(mod)
    return w.detach().to(wdtype).contiguous(), (b.detach().float().contiguous() if b is not None else None)


def lora_wrapped(mod) -> bool:
    return _lin_parts(mod)[3] is not None


def rel_pos_table(d: int, n: int) -> torch.Tensor:
    """pe rows for the relative distances 0 .. n-1 (the positive half of EspnetRelPositionalEncoding's table)."""
    pos = torch.arange(0, n, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(n, d, dtype=torch.float32)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


def bucket(n: int) -> int:
    return max(ATT_KEYS, -(-n // ATT_KEYS) * ATT_KEYS)


class PackedStack:
    """The weights of a RelPosEncoder (input layer + pre-norm layers + after_norm) packed once for the decode kernels:
    merged linears in `wdtype`, LayerNorm / positional-bias parameters fp32.  Shared by every DecodeStack (batch size,
    capacity bucket) built from it.  fold=False packs W alone (the unfolded form: the adapters come per row from an
    AdapterBank's stacks, so the pack depends on no ``lora_`` parameter)."""

    def __init__(self, enc, wdtype: torch.dtype, xscale: bool = True, fold: bool = True):
        self.folded = fold
        if not fold and lora_wrapped(enc.embed.out[0]):
            raise NotImplementedError("unfolded decode: a LoRA-wrapped input layer is not built")
        weight = merged_weight if fold else base_weight
        dev = enc.after_norm.weight.device
        f32 = lambda t: t.detach().float().contiguous()       # noqa: E731
        self.d = d = enc.output_size()
        self.dev = dev
        e0, e1 = enc.embed.out[0], enc.embed.out[1]
        self.W_emb, self.b_emb = weight(e0, wdtype)
        self.ln_emb = (f32(e1.weight), f32(e1.bias), e1.eps)
        self.emb_relu, self.emb_scale = enc.embed.legacy, (math.sqrt(d) if xscale else 1.0)
        self.after = (f32(enc.after_norm.weight), f32(enc.after_norm.bias), enc.after_norm.eps)
        self.layers, self.pos_w = [], []
        for layer in enc.encoders:
            at, ff = layer.self_attn, layer.feed_forward
            if ff.activation != "relu":
                raise NotImplementedError("decode is built for the TransformerEncoder (ReLU feed-forward) stack")
            n1, n2 = (layer.norm_mha, layer.norm_ff) if layer.conformer else (layer.norm1, layer.norm2)
            ws = [weight(m, wdtype) for m in (at.linear_q, at.linear_k, at.linear_v)]
            bq = [b if b is not None else torch.zeros(d, device=dev) for _, b in ws]
            Wo, bo = weight(at.linear_out, wdtype)
            W1, b1 = weight(ff.w_1, wdtype)
            W2, b2 = weight(ff.w_2, wdtype)
            self.layers.append(dict(
                Wqkv=torch.cat([w for w, _ in ws]).contiguous(), bqkv=torch.cat(bq).contiguous(),
                ln1=(f32(n1.weight), f32(n1.bias), n1.eps), ln2=(f32(n2.weight), f32(n2.bias), n2.eps),
                Wo=Wo, bo=bo, W1=W1, b1=b1, W2=W2, b2=b2, u=f32(at.pos_bias_u), v=f32(at.pos_bias_v)))
            self.pos_w.append(f32(at.linear_pos.weight))
        self.H = enc.encoders[0].self_attn.h
        self.F = self.layers[0]["W1"].shape[0]

    def pos_tables(self, cap: int) -> List[torch.Tensor]:
        """per layer P[0 .. cap-1] = linear_pos(pe_d) fp32 (a private pack: the module's own packs may be held by a
        trainer's captured graphs)."""
        pe = rel_pos_table(self.d, cap).to(self.dev)
        with torch.no_grad():
            return [HF.lora_linear(pe, HF.LinearPack(w, None, torch.float32)).detach().contiguous() for w in self.pos_w]


class DecodeStack:
    """A PackedStack on the decode kernels, with B rows of K/V cache of capacity `cap` (and the positional tables and
    work buffers of that size)."""

    def __init__(self, packed: PackedStack, cap: int, B: int):
        self.pk = pk = packed
        dev, d = pk.dev, pk.d
        self.d, self.H, self.F, self.cap, self.B, self.dev = d, pk.H, pk.F, cap, B, dev
        self.W_emb, self.b_emb, self.ln_emb, self.after = pk.W_emb, pk.b_emb, pk.ln_emb, pk.after
        self.emb_relu, self.emb_scale = pk.emb_relu, pk.emb_scale
        self.layers = pk.layers
        self.P = pk.pos_tables(cap)
        nl = len(self.layers)
        self.kc = torch.zeros((nl, B, self.H, cap, 64), dtype=torch.float32, device=dev)
        self.vc = torch.zeros_like(self.kc)
        self.len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)
        R = max(B, MAX_ROWS)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)     # noqa: E731
        self.h, self.qkv, self.o, self.f, self.e = z(R, d), z(R, 3 * d), z(R, d), z(R, self.F), z(R, d)
        self.mean, self.rstd = z(R), z(R)
        self.part = z(R * self.H * (-(-cap // ATT_KEYS)) * 66)
        self.z = None             # [R, 3 * bank rank]: the adapters' down-projections (sessions over an AdapterBank)

    def embed(self, xin: torch.Tensor, M: int) -> torch.Tensor:
        """input layer (Linear -> LayerNorm (-> ReLU) -> x sqrt(d)) of M rows into self.h[:M]."""
        decode_linear(xin, self.W_emb, self.b_emb, out=self.e[:M])
        g, b, eps = self.ln_emb
        return _layernorm(self.e[:M], g, b, eps, self.h[:M], self.mean, self.rstd, self.emb_relu, self.emb_scale)

    def layers_fwd(self, B: int, Lq: int, row: Optional[int] = None, lora=None):
        """the layers over self.h[:B*Lq] (Lq new rows per sequence).  row: a single cache row (prefill of one request).
        lora = (an AdapterBank's per-layer stacks, slot [>= B*Lq] int32): every linear becomes down -> linear_lora with
        each row's own adapter (the pack is then the unfolded one)."""
        M = B * Lq
        h = self.h[:M]
        sl = slice(None) if row is None else slice(row, row + 1)
        length = self.len[sl]
        done = self.done[sl]
        if lora is not None:
            return self._layers_fwd_lora(B, Lq, h, sl, length, done, *lora)
        for i, L in enumerate(self.layers):
            qkv = decode_linear(h, L["Wqkv"], L["bqkv"], ln=L["ln1"], out=self.qkv[:M])
            o = decode_attn(qkv, self.kc[i, sl], self.vc[i, sl], length, self.P[i], L["u"], L["v"], B, self.H, Lq, done=done,
                            part=self.part, out=self.o[:M])
            decode_linear(o, L["Wo"], L["bo"], residual=h, out=h)
            f = decode_linear(h, L["W1"], L["b1"], ln=L["ln2"], act=1, out=self.f[:M])
            decode_linear(f, L["W2"], L["b2"], residual=h, out=h)
        return h

    def _layers_fwd_lora(self, B, Lq, h, sl, length, done, bank, slot):
        M = B * Lq
        z, sc = self.z, bank.scale
        for i, (L, A) in enumerate(zip(self.layers, bank.layers)):
            decode_lora_down(h, A["A_qkv"], slot, ln=L["ln1"], out=z[:M])
            qkv = decode_linear_lora(h, L["Wqkv"], A["B_qkv"], sc, slot, z, 3, L["bqkv"], ln=L["ln1"], out=self.qkv[:M])
            o = decode_attn(qkv, self.kc[i, sl], self.vc[i, sl], length, self.P[i], L["u"], L["v"], B, self.H, Lq, done=done,
                            part=self.part, out=self.o[:M])
            decode_lora_down(o, A["A_o"], slot, out=z[:M])
            decode_linear_lora(o, L["Wo"], A["B_o"], sc, slot, z, 1, L["bo"], residual=h, out=h)
            decode_lora_down(h, A["A_1"], slot, ln=L["ln2"], out=z[:M])
            f = decode_linear_lora(h, L["W1"], A["B_1"], sc, slot, z, 1, L["b1"], ln=L["ln2"], act=1, out=self.f[:M])
            decode_lora_down(f, A["A_2"], slot, out=z[:M])
            decode_linear_lora(f, L["W2"], A["B_2"], sc, slot, z, 1, L["b2"], residual=h, out=h)
        return h

    def prefill(self, x: torch.Tensor, row: int = 0) -> torch.Tensor:
        """x [T, input] fp32 rows appended to cache row `row` (length read from / written to self.len); returns the
        after_norm output [T, d] (a new tensor)."""
        T = x.shape[0]
        out = torch.empty((T, self.d), dtype=torch.float32, device=x.device)
        start = int(self.len[row].item())
        if start + T > self.cap:
            raise ValueError(f"decode cache overflow: {start} + {T} rows > capacity {self.cap}")
        for c0 in range(0, T, MAX_ROWS):
            n = min(MAX_ROWS, T - c0)
            self.embed(x[c0:c0 + n].contiguous(), n)
            h = self.layers_fwd(1, n, row=row)
            g, b, eps = self.after
            _layernorm(h, g, b, eps, out[c0:c0 + n], self.mean, self.rstd)
            self.len[row].fill_(start + c0 + n)
        return out


# ---------------------------------------------------------------------------------------------- reference-API surface
def forward_chunk(enc, xs, offset: int, required_cache_size: int, att_cache=None, cnn_cache=None, att_mask=None):
    """BaseEncoder.forward_chunk (encoder.py:184-273) of a causal TransformerEncoder, batch 1, cache layout
    (elayers, head, t, d_k*2) = K | V.  Only the causal mask the LM passes (tril over the chunk, or an empty mask)
    is built; any other mask raises."""
    assert xs.dim() == 3 and xs.shape[0] == 1, "forward_chunk: batch 1"
    dev = xs.device
    nl = len(enc.encoders)
    t0 = att_cache.shape[2] if att_cache is not None and att_cache.dim() == 4 and att_cache.shape[0] > 0 else 0
    if offset != t0:
        raise NotImplementedError(f"forward_chunk: offset ({offset}) != cached length ({t0}) is not built")
    T = xs.shape[1]
    if att_mask is not None and att_mask.numel() > 0:
        causal = torch.tril(torch.ones(T, T, dtype=torch.bool, device=att_mask.device))
        if att_mask.dim() != 3 or att_mask.shape[0] != 1 or tuple(att_mask.shape[1:]) != (T, T) or \
                not torch.equal(att_mask[0].bool(), causal):
            raise NotImplementedError("forward_chunk: only the causal (1, T, T) tril mask the LM passes is built")
    wdtype = torch.bfloat16 if xs.dtype == torch.bfloat16 else torch.float32
    st = DecodeStack(PackedStack(enc, wdtype), bucket(t0 + T), 1)
    if t0:
        c = att_cache.to(device=dev, dtype=torch.float32)
        st.kc[:, 0, :, :t0] = c[..., :64]
        st.vc[:, 0, :, :t0] = c[..., 64:]
        st.len.fill_(t0)
    with torch.no_grad():
        y = st.prefill(xs[0].float().contiguous())
    n = t0 + T
    new = torch.cat([st.kc[:, 0, :, :n], st.vc[:, 0, :, :n]], dim=-1)
    if required_cache_size >= 0:
        start = n if required_cache_size == 0 else max(n - required_cache_size, 0)
        new = new[:, :, start:]
    return y.unsqueeze(0).to(xs.dtype), new.to(xs.dtype), torch.zeros((nl, 0, 0, 0), dtype=xs.dtype, device=dev)


class SamplerCfg:
    def __init__(self, mode: str, top_p: float = 0.8, top_k: int = 25, win_size: int = 10, tau_r: float = 0.1):
        self.mode, self.top_p, self.top_k, self.win = mode, float(top_p), int(top_k), int(win_size)
        thr = win_size * tau_r                    # rep_num >= win_size * tau_r  <=>  rep_num >= ceil(...)
        self.rep_thr = int(min(max(math.ceil(thr), 0), self.win + 1)) if math.isfinite(thr) else self.win + 1


class PackedLM:
    """The weights of a TransformerLM's decode path, packed once per weight dtype (PackedStack + decoder + table).
    fold=False: W only, for sessions that take their adapters per row from an AdapterBank."""

    def __init__(self, lm, fold: bool = True):
        self.wdtype = torch.bfloat16 if lm.numerics.dtype == torch.bfloat16 else torch.float32
        self.folded = fold
        if not fold and lora_wrapped(lm.llm_decoder):
            raise NotImplementedError("unfolded decode: a LoRA-wrapped llm_decoder is not built")
        self.stack = PackedStack(lm.llm, self.wdtype, xscale=lm.numerics.xscale, fold=fold)
        self.W_dec, self.b_dec = (merged_weight if fold else base_weight)(lm.llm_decoder, self.wdtype)
        self.table = lm.speech_embedding.weight.detach().float().contiguous()
        self.eos = lm.speech_token_size
        self.d_in = lm.llm_input_size


class LMDecodeSession:
    """B rows of lockstep decode of a TransformerLM (see the module docstring) over shared packed weights."""

    def __init__(self, packed: PackedLM, B: int, cap: int, bank=None):
        """bank: an adapters.AdapterBank's stacks for packed.wdtype (the pack is then the unfolded one): every row decodes
        with the adapter whose slot stands in self.slot (-1: none); the captured step holds the stacks' fixed addresses."""
        dev = packed.stack.dev
        self.wdtype = packed.wdtype
        assert (bank is None) == packed.folded, "a folded pack decodes without a bank, an unfolded one with one"
        self.bank = bank
        self.slot = torch.full((max(B, MAX_ROWS),), -1, dtype=torch.int32, device=dev)      # per decode row
        self.pslot = torch.full((MAX_ROWS,), -1, dtype=torch.int32, device=dev)             # the request being prefilled
        self.B, self.cap, self.dev = B, cap, dev
        self.stack = DecodeStack(packed.stack, cap, B)
        if bank is not None:
            self.stack.z = torch.zeros((self.stack.h.shape[0], 3 * bank.rank), dtype=torch.float32, device=dev)
        self.W_dec, self.b_dec, self.table, self.eos = packed.W_dec, packed.b_dec, packed.table, packed.eos
        self.V = self.W_dec.shape[0]
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)   # noqa: E731
        self.tok, self.next_in, self.nhist, self.step, self.err = i32(B), i32(B), i32(B), i32(B), i32(B)
        self.hist = i32(B, HIST)
        self.min_len, self.max_len = i32(B), i32(B)
        self.seeds = torch.zeros(B, dtype=torch.int64, device=dev)
        self.uniforms: Optional[torch.Tensor] = None
        self.logits = torch.zeros((B, self.V), dtype=torch.float32, device=dev)
        self.logp = torch.zeros((B, self.V), dtype=torch.float32, device=dev)
        self.xin = torch.zeros((max(B, MAX_ROWS), packed.d_in), dtype=torch.float32, device=dev)
        self.ubuf = torch.zeros((B, TRIALS, 2), dtype=torch.float32, device=dev)   # pinned draws (the graph holds it)
        self.cfg = SamplerCfg("ras")
        self.graph = None
        self.graph_cfg = None

    # ---- pieces of one step
    def _sample(self, bump_len: bool = True):
        c, st = self.cfg, self.stack
        check(lib().cvft_decode_sample(self.B, self.V, ptr(self.logits), self.V, ptr(self.logp), self.eos, MODES[c.mode],
                                       c.top_k, c.top_p, c.win, c.rep_thr, ptr(self.seeds), ptr(self.uniforms),
                                       ptr(self.tok), ptr(self.next_in), ptr(self.hist), HIST, ptr(self.nhist),
                                       ptr(self.step), ptr(self.min_len), ptr(self.max_len),
                                       ptr(st.len) if bump_len else None, ptr(st.done), ptr(self.err), stream()),
              "cvft_decode_sample")

    def _decoder_logits(self, h, rows: Sequence[int], out_rows: Sequence[int]):
        st = self.stack
        for r, o in zip(rows, out_rows):
            decode_linear(h[r:r + 1], self.W_dec, self.b_dec, ln=st.after, out=self.logits[o:o + 1])

    def _step_kernels(self):
        """one decode step of all B rows: gather the sampled tokens' embeddings -> LM -> decoder -> sampler."""
        st, B = self.stack, self.B
        check(lib().cvft_gather_rows(F32, B, self.table.shape[1], ptr(self.next_in), ptr(self.table), 0.0, ptr(self.xin),
                                     stream()), "cvft_gather_rows")
        st.embed(self.xin[:B], B)
        h = st.layers_fwd(B, 1, lora=None if self.bank is None else (self.bank, self.slot))
        decode_linear(h, self.W_dec, self.b_dec, ln=st.after, out=self.logits)
        self._sample(bump_len=self.cfg.mode != "logp")

    # ---- driving
    def start(self, rows: List[torch.Tensor], min_len: Sequence[int], max_len: Sequence[int], seeds: Sequence[int],
              cfg: SamplerCfg, uniforms: Optional[torch.Tensor] = None, slots: Optional[Sequence[int]] = None):
        """prefill every request's lm_input rows into its cache row and draw its first token.  slots (sessions over an
        AdapterBank): each request's adapter slot, -1 for none."""
        st = self.stack
        assert len(rows) == self.B
        assert (slots is not None) == (self.bank is not None), "slots go with a bank session"
        if slots is not None:
            self.slots = [int(v) for v in slots]
            self.slot[:self.B].copy_(torch.tensor(self.slots, dtype=torch.int32))
        self.cfg = cfg
        if uniforms is not None:              # copied into the session's own buffer: a captured step keeps its address
            self.ubuf.copy_(uniforms.reshape(self.B, TRIALS, 2))
        self.uniforms = self.ubuf if uniforms is not None else None
        for t in (st.len, st.done, self.tok, self.next_in, self.nhist, self.step, self.err, self.hist):
            t.zero_()
        st.kc.zero_()
        st.vc.zero_()
        self.min_len.copy_(torch.tensor(list(min_len), dtype=torch.int32))
        self.max_len.copy_(torch.tensor(list(max_len), dtype=torch.int32))
        self.seeds.copy_(torch.tensor([int(s) & 0x7FFFFFFFFFFFFFFF for s in seeds], dtype=torch.int64))
        for b, x in enumerate(rows):
            if x.shape[0] + int(max_len[b]) > self.cap:
                raise ValueError("decode capacity bucket too small")
            self._prefill_row(x, b)
        self._sample(bump_len=False)

    def _prefill_row(self, x, b):
        st = self.stack
        T = x.shape[0]
        for c0 in range(0, T, MAX_ROWS):
            n = min(MAX_ROWS, T - c0)
            st.embed(x[c0:c0 + n].float().contiguous(), n)
            if self.bank is None:
                h = st.layers_fwd(1, n, row=b)
            else:
                self.pslot.fill_(self.slots[b])
                h = st.layers_fwd(1, n, row=b, lora=(self.bank, self.pslot))
            st.len[b].fill_(c0 + n)
        self._decoder_logits(h, [n - 1], [b])

    def advance(self, use_graph: bool = True):
        if not use_graph:
            self._step_kernels()
            return
        key = (self.cfg.mode, self.cfg.top_k, self.cfg.top_p, self.cfg.win, self.cfg.rep_thr, self.uniforms is None)
        if self.graph is None or self.graph_cfg != key:
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step_kernels()
            self.graph, self.graph_cfg = g, key
        self.graph.replay()

    def read(self):
        """(tokens, done, err) of the last step as host lists (the one device->host read per step)."""
        s = torch.stack([self.tok, self.stack.done, self.err]).cpu()
        return s[0].tolist(), s[1].tolist(), s[2].tolist()
