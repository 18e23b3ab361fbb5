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

Continuous batching: ``LMDecodeSession.admit`` / ``serve_step`` / ``retire`` let a request join a
running batch in a free cache row and leave it when it ends, without touching the captured step (it reads only device state
at fixed addresses).  A newcomer's prompt is prefilled either between two decode steps or a few rows per step alongside the
decode rows: one pass over the linears, and the ragged attention (``decode_attn_ragged``: a segment table instead of a
uniform (B, Lq)).  ``RowScheduler`` is the host-only schedule; ``llm_model.DecodeServer`` is the public front.
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


def decode_attn_ragged(qkv, kc, vc, length, P, pos_bias_u, pos_bias_v, seg, nseg: int, H: int, part=None,
                       out=None) -> torch.Tensor:
    """decode_attn driven by a segment table: seg [>= nseg, 3] int32 (device) = (cache row b, first activation row q0, Lq),
    nseg <= 16 live sequences whose rows are disjoint and sum to <= 16.  qkv [M <= 16, >= 3*H*64], kc / vc
    [rows, H, cap, 64] (all cache rows; only the named ones are read and appended to, at length[b]), length [rows] int32
    -> o [M, H*64] (rows no segment names are left as they are).  Every row equals decode_attn of its sequence alone."""
    M = qkv.shape[0]
    nrows, cap = kc.shape[0], kc.shape[2]
    nsplit = -(-cap // ATT_KEYS)
    D = H * 64
    if part is None:
        part = torch.empty(M * H * nsplit * 66, dtype=torch.float32, device=qkv.device)
    if out is None:
        out = torch.zeros((M, D), dtype=torch.float32, device=qkv.device)
    assert 1 <= nseg <= M <= MAX_ROWS and out.shape[0] >= M and part.numel() >= M * H * nsplit * 66
    assert seg.dtype == torch.int32 and seg.is_contiguous() and seg.numel() >= 3 * nseg
    assert P.shape[0] >= cap and kc.is_contiguous() and vc.is_contiguous() and vc.shape == kc.shape and length.numel() >= nrows
    check(lib().cvft_decode_attn_ragged(nseg, M, nrows, H, cap, nsplit, ptr(seg), ptr(qkv), qkv.stride(0), ptr(kc), ptr(vc),
                                        ptr(length), ptr(P), P.stride(0), ptr(pos_bias_u), ptr(pos_bias_v),
                                        1.0 / math.sqrt(64.0), ptr(part), ptr(out), out.stride(0), stream()),
          "cvft_decode_attn_ragged")
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

    def layers_fwd(self, B: int, Lq: int, row: Optional[int] = None, lora=None, seg=None):
        """the layers over self.h[:B*Lq] (Lq new rows per sequence).  row: a single cache row (prefill of one request).
        lora = (an AdapterBank's per-layer stacks, slot [>= B*Lq] int32): every linear becomes down -> linear_lora with
        each row's own adapter (the pack is then the unfolded one).  seg = (table [>= nseg, 3] int32 on the device, nseg,
        M): the M rows of self.h are the sequences of that segment table (decode_attn_ragged); B, Lq and row are unused."""
        if seg is None:
            M = B * Lq
            sl = slice(None) if row is None else slice(row, row + 1)
            length = self.len[sl]
            done = self.done[sl]

            def attn(i, L, qkv):
                return decode_attn(qkv, self.kc[i, sl], self.vc[i, sl], length, self.P[i], L["u"], L["v"], B, self.H, Lq,
                                   done=done, part=self.part, out=self.o[:M])
        else:
            table, nseg, M = seg

            def attn(i, L, qkv):
                return decode_attn_ragged(qkv, self.kc[i], self.vc[i], self.len, self.P[i], L["u"], L["v"], table, nseg,
                                          self.H, part=self.part, out=self.o[:M])
        h = self.h[:M]
        if lora is not None:
            return self._layers_fwd_lora(M, h, attn, *lora)
        for i, L in enumerate(self.layers):
            qkv = decode_linear(h, L["Wqkv"], L["bqkv"], ln=L["ln1"], out=self.qkv[:M])
            o = attn(i, L, qkv)
            decode_linear(o, L["Wo"], L["bo"], residual=h, out=h)
            f = decode_linear(h, L["W1"], L["b1"], ln=L["ln2"], act=1, out=self.f[:M])
            decode_linear(f, L["W2"], L["b2"], residual=h, out=h)
        return h

    def _layers_fwd_lora(self, M, h, attn, bank, slot):
        z, sc = self.z, bank.scale
        for i, (L, A) in enumerate(zip(self.layers, bank.layers)):
            decode_lora_down(h, A["A_qkv"], slot, ln=L["ln1"], out=z[:M])
            qkv = decode_linear_lora(h, L["Wqkv"], A["B_qkv"], sc, slot, z, 3, L["bqkv"], ln=L["ln1"], out=self.qkv[:M])
            o = attn(i, L, qkv)
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


# ---------------------------------------------------------------------------------------------- serving: the schedule
def check_serve_rows(rows: int, prefill_rows: int) -> None:
    if rows < 1 or prefill_rows < 0 or rows + prefill_rows > MAX_ROWS:
        raise ValueError(f"rows {rows} + prefill_rows {prefill_rows}: at least one row, and at most {MAX_ROWS} activation "
                         f"rows per decode launch")


def prefill_chunks(T: int, prefill_rows: int) -> List[int]:
    """the chunk sizes a prompt of T rows is prefilled in: <= prefill_rows per mixed step, or (prefill_rows = 0, stall)
    the <= 16-row chunks of the prefill path, which all run in one step."""
    n = prefill_rows if prefill_rows > 0 else MAX_ROWS
    return [min(n, T - c0) for c0 in range(0, T, n)]


class RowScheduler:
    """The host-only part of continuous batching: which queued request takes which cache row, and which prompt rows run
    in which step.  Requests are admitted one at a time in FIFO order into the lowest free row; a request's first token
    is due in the step that consumes the last row of its prompt."""

    def __init__(self, rows: int, prefill_rows: int):
        check_serve_rows(rows, prefill_rows)
        self.rows, self.prefill_rows = rows, prefill_rows
        self.free = list(range(rows))
        self.queue: List[tuple] = []                       # (rid, prompt rows), oldest first
        self.row_of: dict = {}                             # rid -> row (admitted, not released)
        self.flight: Optional[list] = None                 # [rid, row, chunk sizes still to run]

    def submit(self, rid, T: int) -> None:
        self.queue.append((rid, int(T)))

    def release(self, rid) -> Optional[int]:
        """the request leaves (finished or cancelled, at any stage); -> the row it held, free again, or None if it was
        still queued."""
        for i, (q, _) in enumerate(self.queue):
            if q == rid:
                del self.queue[i]
                return None
        row = self.row_of.pop(rid)
        if self.flight is not None and self.flight[0] == rid:
            self.flight = None
        self.free.append(row)
        self.free.sort()
        return row

    def busy(self) -> bool:
        return bool(self.queue or self.row_of)

    def plan(self) -> dict:
        """the next step: {'admit': (rid, row) | None -- the request to admit before it, 'rid' / 'row' / 'chunks': the
        prompt chunks this step runs for the admission in flight ([] when there is none), 'first': whether that request's
        first token is due in this step's read}."""
        admit = None
        if self.flight is None and self.queue and self.free:
            rid, T = self.queue.pop(0)
            row = self.free.pop(0)
            self.row_of[rid] = row
            self.flight = [rid, row, prefill_chunks(T, self.prefill_rows)]
            admit = (rid, row)
        if self.flight is None:
            return dict(admit=None, rid=None, row=None, chunks=[], first=False)
        rid, row, left = self.flight
        chunks = left[:] if self.prefill_rows == 0 else left[:1]
        del left[:len(chunks)]
        if not left:
            self.flight = None
        return dict(admit=admit, rid=rid, row=row, chunks=chunks, first=not left)


def serve_schedule(rows: int, prefill_rows: int, requests: Sequence[tuple]) -> List[dict]:
    """The schedule of requests = [(arrival step, prompt rows, tokens it will decode), ...] (in arrival order) on the
    RowScheduler, without a device: per request {'row', 'admit_step', 'chunks': [(step, size), ...], 'first_step': the
    step whose read carries its first token, 'last_step': the step of its last token}."""
    sch = RowScheduler(rows, prefill_rows)
    out = [dict(row=None, admit_step=None, chunks=[], first_step=None, last_step=None) for _ in requests]
    left = {}
    step, nxt = 0, 0
    while nxt < len(requests) or sch.busy():
        while nxt < len(requests) and requests[nxt][0] <= step:
            sch.submit(nxt, requests[nxt][1])
            nxt += 1
        p = sch.plan()
        if p["admit"] is not None:
            rid, row = p["admit"]
            out[rid].update(row=row, admit_step=step)
        for rid in list(left):                               # every decoding row draws one token
            left[rid] -= 1
        if p["rid"] is not None:
            out[p["rid"]]["chunks"] += [(step, n) for n in p["chunks"]]
            if p["first"]:
                out[p["rid"]]["first_step"] = step
                left[p["rid"]] = requests[p["rid"]][2] - 1
        for rid in [r for r, n in left.items() if n <= 0]:
            out[rid]["last_step"] = step
            del left[rid]
            sch.release(rid)
        step += 1
    return out


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

    def __init__(self, packed: PackedLM, B: int, cap: int, bank=None, prefill_rows: int = 0):
        """bank: an adapters.AdapterBank's stacks for packed.wdtype (the pack is then the unfolded one): every row decodes
        with the adapter whose slot stands in self.slot (-1: none); the captured step holds the stacks' fixed addresses.
        prefill_rows (admit / serve_step only): 0 prefills an admitted request between two decode steps; n > 0 carries up
        to n of its prompt rows along with every decode step (B + n <= 16)."""
        check_serve_rows(B, prefill_rows)
        self.prefill_rows = int(prefill_rows)
        self.live: set = set()            # rows that decode (admitted, first token drawn, not retired): host view
        self.adm: Optional[dict] = None   # the admission in flight: row, prompt rows, rows consumed, slot
        self.slots = [-1] * B
        dev = packed.stack.dev
        self.seg = torch.zeros((MAX_ROWS, 3), dtype=torch.int32, device=dev)                # the mixed step's segment table
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

    # ---- continuous batching: rows join and leave a running batch (llm_model.DecodeServer drives these)
    def _sample_row(self, b: int):
        """the sampler for row b alone (B = 1, every per-row pointer at row b); lengths are not bumped."""
        c, st, V = self.cfg, self.stack, self.V
        u = None if self.uniforms is None else self.uniforms[b]
        check(lib().cvft_decode_sample(1, V, ptr(self.logits[b]), V, ptr(self.logp[b]), self.eos, MODES[c.mode], c.top_k,
                                       c.top_p, c.win, c.rep_thr, ptr(self.seeds[b:]), ptr(u), ptr(self.tok[b:]),
                                       ptr(self.next_in[b:]), ptr(self.hist[b]), HIST, ptr(self.nhist[b:]),
                                       ptr(self.step[b:]), ptr(self.min_len[b:]), ptr(self.max_len[b:]), None,
                                       ptr(st.done[b:]), ptr(self.err[b:]), stream()), "cvft_decode_sample")

    def idle(self, cfg: SamplerCfg):
        """every row free (done, so the captured step skips it), nothing in flight; `cfg` is the sampler of all admissions."""
        assert cfg.mode != "logp", "admit / serve_step run the device sampler"
        self.cfg = cfg
        self.uniforms = None
        self.stack.done.fill_(1)
        self.live.clear()
        self.adm = None

    def admit(self, b: int, x: torch.Tensor, min_len: int, max_len: int, seed: int, slot: Optional[int] = None,
              uniforms: Optional[torch.Tensor] = None):
        """Start request x [T, input] (its lm_input rows) in the free cache row b while the other rows keep decoding: row
        b's state alone is reset (its K/V needs no clearing, nothing reads past len[b]) and it stays `done` until its
        prompt is in the cache, so the all-rows sampler and the captured step skip it.  The prompt is consumed by the
        following serve_step calls; the read() after the last of its rows carries the request's first token.  One
        admission at a time.  uniforms [101, 2]: pinned draws for every step of this request (then every live row must
        have pinned draws: the sampler takes all of them or none)."""
        st = self.stack
        T = int(x.shape[0])
        if T + int(max_len) > self.cap:
            raise ValueError("decode capacity bucket too small")
        if not 0 <= b < self.B or b in self.live or T < 1 or int(max_len) < 1:
            raise ValueError(f"admit: row {b} of {self.B} (decoding rows {sorted(self.live)}), {T} prompt rows, max_len {max_len}")
        if self.adm is not None:
            raise RuntimeError("admit: another admission is in flight")
        if (slot is not None) != (self.bank is not None):
            raise ValueError("admit: a slot goes with a bank session")
        if self.live and (uniforms is None) != (self.uniforms is None):
            raise ValueError("admit: pinned uniforms for all live rows or for none")
        if uniforms is not None:
            self.ubuf[b].copy_(uniforms.reshape(TRIALS, 2))
        self.uniforms = self.ubuf if uniforms is not None else None
        st.done[b:b + 1].fill_(1)
        for t in (st.len, self.tok, self.next_in, self.nhist, self.step, self.err):
            t[b:b + 1].zero_()
        self.hist[b].zero_()
        self.min_len[b:b + 1].fill_(int(min_len))
        self.max_len[b:b + 1].fill_(int(max_len))
        self.seeds[b:b + 1].fill_(int(seed) & 0x7FFFFFFFFFFFFFFF)
        self.slots[b] = -1 if slot is None else int(slot)
        self.slot[b:b + 1].fill_(self.slots[b])
        self.adm = dict(row=b, x=x.float().contiguous(), pos=0)

    def retire(self, b: int):
        """free row b (a finished or cancelled request, or the admission in flight): done, so every later step skips it."""
        self.stack.done[b:b + 1].fill_(1)
        self.live.discard(b)
        if self.adm is not None and self.adm["row"] == b:
            self.adm = None

    def serve_step(self, prefill: int = 0, use_graph: bool = True):
        """One step of the running batch: every decoding row draws its next token, and `prefill` more prompt rows of the
        admission in flight enter its cache row (the scheduler's chunk: with prefill_rows = 0 the whole prompt, else at
        most prefill_rows).  Without prefill work this is advance(): the captured step, which reads nothing but device
        state at fixed addresses, so rows that joined or left since its capture change nothing about it."""
        a = self.adm
        if a is None or prefill == 0:
            assert prefill == 0, "serve_step: no admission in flight"
            if self.live:
                self.advance(use_graph)
            return
        b, x, pos = a["row"], a["x"], a["pos"]
        T = x.shape[0]
        last = pos + prefill == T
        if self.prefill_rows == 0:
            # stall: the decode step of the others first (row b is still done), then b's prompt through the prefill path
            assert pos == 0 and last, "serve_step: the stall mode prefills a prompt whole"
            if self.live:
                self.advance(use_graph)
            self.stack.done[b:b + 1].zero_()
            self._prefill_row(x, b)
        else:
            assert 1 <= prefill <= self.prefill_rows and pos + prefill <= T
            self._mixed_step(b, x[pos:pos + prefill], pos, last)
        a["pos"] = pos + prefill
        if last:
            self._sample_row(b)
            self.live.add(b)
            self.adm = None

    def _mixed_step(self, b: int, xc: torch.Tensor, pos: int, last: bool):
        """a decode step of rows 0 .. B-1 that carries the prompt chunk xc of row b as activation rows B .. B+n-1 through
        the same weight stream (run eagerly: the segment table and M change from step to step)."""
        st, B, n = self.stack, self.B, xc.shape[0]
        M = B + n
        check(lib().cvft_gather_rows(F32, B, self.table.shape[1], ptr(self.next_in), ptr(self.table), 0.0, ptr(self.xin),
                                     stream()), "cvft_gather_rows")
        self.xin[B:M].copy_(xc)
        self.slot[B:M].fill_(self.slots[b])
        segs = [(r, r, 1) for r in sorted(self.live)] + [(b, B, n)]
        self.seg[:len(segs)].copy_(torch.tensor(segs, dtype=torch.int32))
        st.embed(self.xin[:M], M)
        h = st.layers_fwd(0, 0, lora=None if self.bank is None else (self.bank, self.slot), seg=(self.seg, len(segs), M))
        if self.live:
            decode_linear(h[:B], self.W_dec, self.b_dec, ln=st.after, out=self.logits)
            self._sample(bump_len=True)
        st.len[b:b + 1].fill_(pos + n)
        if last:
            self._decoder_logits(h, [M - 1], [b])
            st.done[b:b + 1].zero_()
