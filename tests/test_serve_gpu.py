"""Continuous batching on the GPU: the ragged decode attention (cvft_decode_attn_ragged) against cvft_decode_attn of each
sequence alone and an fp64 restatement, TransformerLM.decode_server (requests joining and leaving a running batch)
against TransformerLM.inference of every request alone, and StreamingSynthesizer.serve against tts of every request alone."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from helpers import build_llm_product, rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ the kernel
H, CAP = 16, 1536
LENS = [1, 37, 254, 1500, 700]                       # cache row 4 is named by no segment
SEGS = [(0, 0, 1), (3, 1, 1), (2, 2, 5), (1, 7, 9)]   # (cache row, first activation row, Lq): 16 rows; row 2 straddles key 256


@functools.lru_cache(maxsize=None)
def _operands():
    g = torch.Generator(device="cpu").manual_seed(2024)
    D = H * 64
    kc, vc = torch.randn(len(LENS), H, CAP, 64, generator=g), torch.randn(len(LENS), H, CAP, 64, generator=g)
    for b, L in enumerate(LENS[:4]):                  # (rows 0-3: zeros past len, so an append elsewhere would show)
        kc[b, :, L:] = 0
        vc[b, :, L:] = 0
    qkv = torch.randn(16, 3 * D, generator=g)
    P = torch.randn(CAP, D, generator=g) * 0.5
    u, v = torch.randn(H, 64, generator=g) * 0.1, torch.randn(H, 64, generator=g) * 0.1
    return kc, vc, qkv, P, u, v


def _ragged(segs, M):
    from cosyvoice_lora_finetune_framework_amd.decode import decode_attn_ragged
    kc, vc, qkv, P, u, v = _operands()
    kd, vd = kc.to(DEV), vc.to(DEV)
    o = torch.full((M, H * 64), 7.0, device=DEV)
    seg = torch.tensor(segs, dtype=torch.int32, device=DEV)
    decode_attn_ragged(qkv[:M].to(DEV), kd, vd, torch.tensor(LENS, dtype=torch.int32, device=DEV), P.to(DEV), u.to(DEV),
                       v.to(DEV), seg, len(segs), H, out=o)
    torch.cuda.synchronize()
    return o.cpu(), kd.cpu(), vd.cpu()


def _alone(b, q0, Lq):
    from cosyvoice_lora_finetune_framework_amd.decode import decode_attn
    kc, vc, qkv, P, u, v = _operands()
    kd, vd = kc[b:b + 1].to(DEV), vc[b:b + 1].to(DEV)
    o = decode_attn(qkv[q0:q0 + Lq].to(DEV), kd, vd, torch.tensor(LENS[b:b + 1], dtype=torch.int32, device=DEV), P.to(DEV),
                    u.to(DEV), v.to(DEV), 1, H, Lq)
    torch.cuda.synchronize()
    return o.cpu(), kd.cpu()[0], vd.cpu()[0]


def test_ragged_attention_rows_equal_each_sequence_alone():
    from test_llm_decode_gpu import _attn_ref
    kc, vc, qkv, P, u, v = _operands()
    D = H * 64
    o, kd, vd = _ragged(SEGS, 16)
    assert sum(s[2] for s in SEGS) == 16
    for b, q0, Lq in SEGS:
        L = LENS[b]
        rows = slice(q0, q0 + Lq)
        one, k1, v1 = _alone(b, q0, Lq)
        assert torch.equal(o[rows], one), (b, q0, Lq)                        # bit-equal to cvft_decode_attn of that sequence
        assert torch.equal(kd[b], k1) and torch.equal(vd[b], v1)
        for h in range(H):
            c = slice(h * 64, (h + 1) * 64)
            kn, vn = qkv[rows, D + h * 64:D + (h + 1) * 64], qkv[rows, 2 * D + h * 64:2 * D + (h + 1) * 64]
            ref = _attn_ref(qkv[rows, c], kc[b, h], vc[b, h], kn, vn, P[:, c], u[h], v[h], L, Lq)
            assert rel(o[rows, c], ref) < 1e-5, (b, h, rel(o[rows, c], ref))
            assert torch.equal(kd[b, h, L:L + Lq], kn) and torch.equal(vd[b, h, L:L + Lq], vn)        # appended in place
            assert torch.equal(kd[b, h, :L], kc[b, h, :L]) and not kd[b, h, L + Lq:].any()
            assert torch.equal(vd[b, h, :L], vc[b, h, :L]) and not vd[b, h, L + Lq:].any()
    assert torch.equal(kd[4], kc[4]) and torch.equal(vd[4], vc[4])           # the row no segment names


def test_ragged_attention_single_segment_and_unnamed_rows():
    kc, vc, _, _, _, _ = _operands()
    o, kd, vd = _ragged([(2, 0, 16)], 16)                                    # one segment: cvft_decode_attn's launch
    one, k1, v1 = _alone(2, 0, 16)
    assert torch.equal(o, one) and torch.equal(kd[2], k1) and torch.equal(vd[2], v1)
    for b in (0, 1, 3, 4):
        assert torch.equal(kd[b], kc[b]) and torch.equal(vd[b], vc[b])
    o, kd, vd = _ragged([(3, 4, 2)], 8)                                      # activation rows no segment names keep their o
    one, _, _ = _alone(3, 4, 2)
    assert torch.equal(o[4:6], one)
    assert bool((o[:4] == 7.0).all()) and bool((o[6:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ the server
def _meta():
    return json.load(open(os.path.join(GOLD, "llm_decode_meta.json")))["tiny"]


def _greedy():
    from cosyvoice_lora_finetune_framework_amd import utils as U
    return functools.partial(U.ras_sampling, top_k=1, tau_r=1e9)


@functools.lru_cache(maxsize=None)
def _model(sampled: bool, dtype):
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    m = build_llm_product(_meta(), DEV, Numerics(dtype=dtype))
    m.sampling = None if sampled else _greedy()
    return m


TEXT_LENS = (4, 40, 2, 17, 1)
SEEDS = [101, 202, 303, 404, 505]
# greedy runs may stop at any EOS (a greedy draw cannot be redrawn: before min_len it would be the sampler's error); sampled
# runs redraw EOS before min_len
RATIOS = {False: dict(min_token_text_ratio=0, max_token_text_ratio=3), True: dict(min_token_text_ratio=0.5, max_token_text_ratio=3)}
SUBMIT_AFTER = {3: 3, 4: 10}                         # request -> submitted after this many steps (0-2: before the first)


@functools.lru_cache(maxsize=None)
def _requests():
    g = torch.Generator(device="cpu").manual_seed(77)
    texts = [torch.randint(0, 100, (n,), generator=g) for n in TEXT_LENS]
    embs = [torch.zeros(1, 192), torch.randn(1, 192, generator=g), torch.zeros(0, 192), torch.randn(1, 192, generator=g),
            torch.randn(1, 192, generator=g)]
    return texts, embs


def _single(m, i, ratios, **kw):
    """request i through TransformerLM.inference alone: (tokens, the logits row after its first token)."""
    texts, embs = _requests()
    z = torch.zeros(1, 0, dtype=torch.long, device=DEV)
    toks, first = [], None
    for t in m.inference(texts[i][None].to(DEV), torch.tensor([texts[i].numel()]), z, torch.tensor([0]), z,
                         torch.tensor([0]), embs[i].to(DEV), seed=SEEDS[i], **ratios, **kw):
        if first is None:
            first = list(m._cvft_sessions.values())[-1][1].logits[0].clone()
        toks.append(t)
    return toks, first


@functools.lru_cache(maxsize=None)
def _singles(sampled: bool, dtype):
    m = _model(sampled, dtype)
    return [_single(m, i, RATIOS[sampled]) for i in range(len(TEXT_LENS))]


def _drive(srv, submit, n, after):
    """submit requests 0 .. n-1 (request i after after[i] steps, default before the first) and step to the end:
    (tokens per request from the step events, first-token logits rows, the row each request took, the graph objects seen)."""
    rids, toks, first, rows, graphs = {}, {}, {}, {}, set()
    steps = 0
    while len(rids) < n or srv.pending():
        for i in range(n):
            if i not in rids and after.get(i, 0) <= steps:
                rids[i] = submit(i)
                toks[rids[i]] = []
        for rid, tok, fin in srv.step():
            if rid not in first:
                row = srv.req[rid]["row"]
                rows[rid], first[rid] = row, srv.sess.logits[row].clone()
            if tok is not None:
                toks[rid].append(tok)
        steps += 1
        if srv.sess.graph is not None:
            graphs.add(srv.sess.graph)
        assert steps < 2000
    return rids, toks, first, rows, graphs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("prefill_rows", [0, 6], ids=["stall", "piggyback"])
def test_server_equals_single_runs(prefill_rows, sampled, dtype):
    m = _model(sampled, dtype)
    want = _singles(sampled, dtype)
    texts, embs = _requests()
    srv = m.decode_server(rows=2, max_cache=256, prefill_rows=prefill_rows)
    submit = lambda i: srv.submit(texts[i].to(DEV), embedding=embs[i].to(DEV), seed=SEEDS[i], **RATIOS[sampled])      # noqa: E731
    rids, toks, first, rows, graphs = _drive(srv, submit, 5, SUBMIT_AFTER)
    for i in range(5):
        rid = rids[i]
        assert toks[rid] == want[i][0], i
        assert srv.result(rid) == want[i][0]
        assert torch.equal(first[rid], want[i][1]), i
    print("tokens per request", [len(w[0]) for w in want], "rows", [rows[rids[i]] for i in range(5)])
    assert len(graphs) == 1                                       # one captured step, the same object from first to last
    assert len({tuple(w[0]) for w in want}) > 1
    assert -(-(2 + 1 + TEXT_LENS[1]) // 6) >= 3                   # request 1's prompt spans >= 3 piggyback chunks
    # two rows, five requests: rows were reused, and a short request ran in a row that a longer one had left
    assert set(rows.values()) == {0, 1}
    assert any(rows[rids[j]] == rows[rids[i]] and TEXT_LENS[j] < TEXT_LENS[i] for i in range(5) for j in range(i + 1, 5))


def test_server_with_sixteen_activation_rows_equals_single_runs():
    """rows + prefill_rows = 16: the mixed step at the launch limit, all five requests decoding side by side."""
    m = _model(True, torch.float32)
    want = _singles(True, torch.float32)
    texts, embs = _requests()
    srv = m.decode_server(rows=10, max_cache=256, prefill_rows=6)
    submit = lambda i: srv.submit(texts[i].to(DEV), embedding=embs[i].to(DEV), seed=SEEDS[i], **RATIOS[True])      # noqa: E731
    rids, toks, first, rows, graphs = _drive(srv, submit, 5, {})
    for i in range(5):
        assert toks[rids[i]] == want[i][0], i
        assert torch.equal(first[rids[i]], want[i][1]), i
    # (the 12-token request 0 has ended by the time request 4 is admitted: one admission at a time, 8 + 1 + 4 steps ahead of it)
    assert [rows[rids[i]] for i in range(4)] == [0, 1, 2, 3] and len(graphs) == 1


def test_server_with_adapters_equals_single_runs():
    from test_adapters_gpu import _bank_model
    from cosyvoice_lora_finetune_framework_amd.adapters import BASE
    m, _ = _bank_model(sampling="ras")
    texts, embs = _requests()
    names = ["gold", "b", BASE, "b", "gold"]
    srv = m.decode_server(rows=2, max_cache=256, prefill_rows=6, adapters=True)
    submit = lambda i: srv.submit(texts[i].to(DEV), embedding=embs[i].to(DEV), seed=SEEDS[i], adapter=names[i], **RATIOS[True])      # noqa: E731
    rids, toks, _, _, graphs = _drive(srv, submit, 5, SUBMIT_AFTER)
    singles = [_single(m, i, RATIOS[True], adapter=names[i])[0] for i in range(5)]
    for i in range(5):
        assert toks[rids[i]] == singles[i], (i, names[i])
    assert len(graphs) == 1 and len({tuple(s) for s in singles}) > 1
    with pytest.raises(ValueError):
        srv.submit(texts[0].to(DEV), seed=1)                      # a server over the bank: every request names its adapter


def test_cancel_capacity_and_empty_requests():
    m = _model(True, torch.float32)                               # (sampled: request 1 cannot end before its min_len of 20)
    want = _singles(True, torch.float32)
    texts, embs = _requests()
    srv = m.decode_server(rows=1, max_cache=256, prefill_rows=6)
    sub = lambda i, **kw: srv.submit(texts[i].to(DEV), embedding=embs[i].to(DEV), seed=SEEDS[i], **{**RATIOS[True], **kw})      # noqa: E731
    calls = __import__("cosyvoice_lora_finetune_framework_amd.hipops.binding", fromlist=["CALLS"])
    n0 = calls.CALLS
    with pytest.raises(ValueError, match="decode capacity bucket too small"):
        sub(1, max_token_text_ratio=20)                           # 43 prompt rows + 800 tokens > 256
    assert calls.CALLS == n0 and not srv.pending()                # refused on the host: nothing was launched
    empty = sub(2, max_token_text_ratio=0.25)                     # max_len = int(2 * 0.25) = 0
    assert srv.step() == [(empty, None, True)] and srv.result(empty) == []
    a, b, c = sub(1), sub(0), sub(3)
    for _ in range(12):
        srv.step()
    assert srv.req[a]["row"] == 0 and len(srv.req[a]["tokens"]) > 0 and srv.req[b]["state"] == "queued"
    srv.cancel(a)                                                 # the running request leaves: the oldest queued one takes its row
    srv.cancel(c)                                                 # and a queued one leaves the queue
    assert srv.pending() == 1
    srv.step()
    assert srv.req[b]["row"] == 0
    assert srv.run() == {b: want[0][0]}
    with pytest.raises(KeyError):
        srv.result(a)
    with pytest.raises(ValueError):
        m.decode_server(rows=11, prefill_rows=6)
    keep, m.sampling = m.sampling, (lambda s, d, n: s.argmax().reshape(1))          # a host callable
    try:
        with pytest.raises(NotImplementedError):
            m.decode_server(rows=2)
    finally:
        m.sampling = keep


def test_a_request_in_the_eos_error_fails_alone():
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    arr = dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz")))
    meta = _meta()
    m = build_llm_product(meta, DEV, Numerics())
    m.sampling = _greedy()
    with torch.no_grad():
        m.llm_decoder.bias[m.speech_token_size] += meta["eos_bias_bump"]
    t = lambda k, n: torch.from_numpy(arr[f"{k}_{n}"]).to(DEV)          # noqa: E731
    z = torch.zeros(1, 0, dtype=torch.long, device=DEV)
    one = torch.tensor([4])
    # the neighbour may stop at once (min_len 0), so the bumped EOS ends it after its first token instead of failing it
    alone = list(m.inference(t("i", "text"), one, z, torch.tensor([0]), z, torch.tensor([0]), t("i", "emb"), seed=5,
                             min_token_text_ratio=0))
    srv = m.decode_server(rows=2, max_cache=256, prefill_rows=0)
    bad = srv.submit(t("iii", "text"), embedding=t("iii", "emb"), seed=6)          # min_len 8: EOS is redrawn 100 times
    ok = srv.submit(t("i", "text"), embedding=t("i", "emb"), seed=5, min_token_text_ratio=0)
    events = []
    while srv.pending():
        events += srv.step()
    mine = [e for e in events if e[0] == bad]
    assert mine[-1] == (bad, None, True) and [e[2] for e in mine] == [False] * (len(mine) - 1) + [True]
    assert srv.result(ok) == alone and len(alone) >= 1
    with pytest.raises(RuntimeError) as e:
        srv.result(bad)
    assert str(e.value) == meta["error"]


def test_weights_changing_under_requests_in_flight():
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    m = build_llm_product(_meta(), DEV, Numerics())
    m.sampling = _greedy()
    texts, embs = _requests()
    srv = m.decode_server(rows=2, max_cache=256, prefill_rows=0)
    rid = srv.submit(texts[0].to(DEV), embedding=embs[0].to(DEV), seed=1, **RATIOS[False])
    srv.step()
    with torch.no_grad():
        m.llm_decoder.bias.add_(0.25)
    with pytest.raises(RuntimeError, match="weights changed"):
        srv.step()
    srv.cancel(rid)
    rid = srv.submit(texts[0].to(DEV), embedding=embs[0].to(DEV), seed=SEEDS[0], **RATIOS[False])      # idle: repacked
    z = torch.zeros(1, 0, dtype=torch.long, device=DEV)
    alone = list(m.inference(texts[0][None].to(DEV), torch.tensor([4]), z, torch.tensor([0]), z, torch.tensor([0]),
                             embs[0].to(DEV), seed=SEEDS[0], **RATIOS[False]))
    assert srv.run() == {rid: alone}


# ------------------------------------------------------------------------------------------------ the streaming front
def test_serve_chunks_equal_tts_of_each_request_alone():
    from test_stream_gpu import synthesizer
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    llm = build_llm_product(_meta(), DEV, Numerics())
    llm.sampling = None                                           # ras draws keyed by each request's seed; EOS redrawn before min_len
    syn = synthesizer(llm, hop=20)
    text = [int(t) for t in dict(np.load(os.path.join(GOLD, "llm_decode_tiny.npz")))["i_text"][0]]
    specs = [("a", text, 90), ("b", text[::-1], 70), ("c", text[1:] + text[:1], 50)]
    reqs = []
    for n, (key, tx, ntok) in enumerate(specs):
        ratio = (ntok + 0.5) / len(tx)
        g = torch.Generator().manual_seed(900 + n)
        noise = [torch.randn(1, 80, syn.chunk_frames(hi - lo, 0)[0], generator=g).to(DEV) for lo, hi, _ in syn.chunk_plan(ntok)]
        reqs.append(dict(key=key, text_tokens=tx, seed=7 + n, hift_seed=11 + 5 * n, noise=noise,
                         llm_kw=dict(min_token_text_ratio=ratio, max_token_text_ratio=ratio)))
    want = {}
    for q in reqs:
        kw = {k: v for k, v in q.items() if k not in ("key", "text_tokens")}
        want[q["key"]] = [it["tts_speech"] for it in syn.tts(q["text_tokens"], stream=True, **kw)]
    assert [len(want[k]) for k in "abc"] == [4, 3, 2]
    seen = []

    def arrivals():
        yield reqs[0]
        yield reqs[1]
        while not seen:                                           # the third request arrives once the first item is out
            yield None
        yield reqs[2]

    got = {k: [] for k in "abc"}
    for key, item in syn.serve(arrivals(), rows=2, prefill_rows=6, max_cache=256):
        seen.append(key)
        got[key].append(item)
    for k in "abc":
        assert len(got[k]) == len(want[k]), k
        assert [it["final"] for it in got[k]] == [False] * (len(want[k]) - 1) + [True], k
        for i, (it, w) in enumerate(zip(got[k], want[k])):
            assert torch.equal(it["tts_speech"], w), (k, i)
    assert seen.index("c") > 0
