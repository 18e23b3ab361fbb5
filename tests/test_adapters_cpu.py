"""Host logic of adapters.AdapterBank (no GPU, bank on the CPU): slots and LRU eviction, zero-padding to the bank rank,
per-slot alpha / r, the decode-stack layouts against a numpy restatement, prefix-tolerant loading, the errors, and what
``activate`` writes."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import build_llm_product

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CPU = torch.device("cpu")


def _llm():
    from cosyvoice_lora_finetune_framework_amd.modules import Numerics
    meta = json.load(open(os.path.join(GOLD, "llm_decode_meta.json")))["tiny"]
    return build_llm_product(meta, CPU, Numerics()), meta


def _adapter(llm, r, seed):
    """a seeded random adapter of rank r for every LoRA layer of llm (state-dict names)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n, p in llm.named_parameters():
        if "lora_A" in n:
            sd[n] = torch.randn(r, p.shape[1], generator=g) * 0.1
        elif "lora_B" in n:
            sd[n] = torch.randn(p.shape[0], r, generator=g) * 0.1
    return sd


def _bank(llm, **kw):
    from cosyvoice_lora_finetune_framework_amd.adapters import AdapterBank
    return AdapterBank(llm=llm, device="cpu", **kw)


def test_slots_and_lru_eviction():
    from cosyvoice_lora_finetune_framework_amd.adapters import BASE
    llm, _ = _llm()
    bank = _bank(llm, capacity=2, rank=8)
    assert bank.load("a", _adapter(llm, 4, 1)) == 0
    assert bank.load("b", _adapter(llm, 4, 2)) == 1
    assert bank.names() == ["a", "b"]
    assert bank.slot("a") == 0 and bank.names() == ["b", "a"]          # a use moves a name to the recent end
    assert bank.load("c", _adapter(llm, 4, 3)) == 1                     # b was the least recently used: its slot
    assert bank.names() == ["a", "c"] and bank.slot(BASE) == -1
    with pytest.raises(KeyError):
        bank.slot("b")
    bank.evict("a")
    assert bank.names() == ["c"]
    assert bank.load("d", _adapter(llm, 4, 4)) == 0
    assert bank.load("c", _adapter(llm, 4, 5)) == 1                     # a resident name keeps its slot


def test_padding_scale_and_layouts_against_numpy():
    llm, meta = _llm()
    bank = _bank(llm, capacity=3, rank=8)
    st = bank.stacks(torch.float32)
    addr = [t.data_ptr() for L in st.layers for t in L.values()] + [st.scale.data_ptr()]
    sd4, sd8 = _adapter(llm, 4, 11), _adapter(llm, 8, 12)
    bank.load("r4", sd4)                     # alpha defaults to the modules' (8): scale 8 / 4
    bank.load("r8", sd8, alpha=3.0)          # scale 3 / 8
    assert addr == [t.data_ptr() for L in st.layers for t in L.values()] + [st.scale.data_ptr()]
    np.testing.assert_array_equal(st.scale.numpy(), np.array([meta["lora"]["alpha"] / 4, 3.0 / 8, 0.0], dtype=np.float32))
    d, F, R = meta["build"]["d"], meta["build"]["ff"], 8
    for slot, (sd, r) in enumerate(((sd4, 4), (sd8, 8))):
        for i in range(meta["build"]["llm_blocks"]):
            pre = f"llm.encoders.{i}."
            A = np.zeros((3, R, d), dtype=np.float32)
            B = np.zeros((3 * d, R), dtype=np.float32)
            for g, nm in enumerate(("linear_q", "linear_k", "linear_v")):
                A[g, :r] = sd[pre + f"self_attn.{nm}.lora_A"].numpy()
                B[g * d:(g + 1) * d, :r] = sd[pre + f"self_attn.{nm}.lora_B"].numpy()
            L = st.layers[i]
            assert tuple(L["A_qkv"].shape) == (3, 3, R, d) and tuple(L["B_qkv"].shape) == (3, 3 * d, R)
            np.testing.assert_array_equal(L["A_qkv"][slot].numpy(), A)
            np.testing.assert_array_equal(L["B_qkv"][slot].numpy(), B)
            for role, nm, K, N in (("o", "self_attn.linear_out", d, d), ("1", "feed_forward.w_1", d, F),
                                   ("2", "feed_forward.w_2", F, d)):
                A = np.zeros((1, R, K), dtype=np.float32)
                B = np.zeros((N, R), dtype=np.float32)
                A[0, :r] = sd[pre + nm + ".lora_A"].numpy()
                B[:, :r] = sd[pre + nm + ".lora_B"].numpy()
                assert tuple(L["A_" + role].shape) == (3, 1, R, K) and tuple(L["B_" + role].shape) == (3, N, R)
                np.testing.assert_array_equal(L["A_" + role][slot].numpy(), A)
                np.testing.assert_array_equal(L["B_" + role][slot].numpy(), B)
    # a second dtype gets its own stacks, filled from the resident adapters
    sb = bank.stacks(torch.bfloat16)
    assert sb is not st and sb.layers[0]["A_o"].dtype == torch.bfloat16
    assert torch.equal(sb.layers[0]["A_o"][0, 0, :4], sd4["llm.encoders.0.self_attn.linear_out.lora_A"].to(torch.bfloat16))
    # the unfolded restatement of one linear: W x + scale * B (A x) from the stacks == from the adapter's own tensors
    x = torch.randn(d, generator=torch.Generator().manual_seed(1)).double()
    a, b = sd4["llm.encoders.1.feed_forward.w_1.lora_A"].double(), sd4["llm.encoders.1.feed_forward.w_1.lora_B"].double()
    want = (meta["lora"]["alpha"] / 4) * (b @ (a @ x))
    got = st.scale[0].double() * (st.layers[1]["B_1"][0].double() @ (st.layers[1]["A_1"][0, 0].double() @ x))
    assert torch.allclose(got, want, rtol=1e-12, atol=0)


def test_loading_lora_file_and_trainer_checkpoint(tmp_path):
    from cosyvoice_lora_finetune_framework_amd.lora import save_lora_weights
    llm, _ = _llm()
    save_lora_weights(llm, str(tmp_path / "lora.pt"))
    own = {n: p.detach().clone() for n, p in llm.named_parameters() if "lora_" in n}
    bank = _bank(llm, capacity=2, rank=8)
    bank.load("file", str(tmp_path / "lora.pt"))
    # trainer style: {'state_dict': {'model.llm.<name>': ...}} with the frozen base alongside
    ck = {"state_dict": {"model.llm." + k: v.detach().clone() for k, v in llm.state_dict().items()}, "epoch": 3}
    torch.save(ck, tmp_path / "joint.ckpt")
    bank.load("ckpt", str(tmp_path / "joint.ckpt"))
    st = bank.stacks(torch.float32)
    for L in st.layers:
        for t in L.values():
            assert torch.equal(t[0], t[1]) and t[0].abs().sum() > 0
    k = "llm.encoders.0.feed_forward.w_2.lora_B"
    assert torch.equal(st.layers[0]["B_2"][0][:, :4], own[k]) and not st.layers[0]["B_2"][0][:, 4:].any()
    # 'llm.'-prefixed keys of a bare joint state also resolve (the branch's own names start with 'llm.' too)
    bank.load("ckpt", {"llm." + k: v for k, v in own.items()})
    assert torch.equal(st.layers[0]["B_2"][1][:, :4], own[k])


def test_errors():
    from cosyvoice_lora_finetune_framework_amd.adapters import AdapterBank
    from cosyvoice_lora_finetune_framework_amd.lora import LoRALinear
    llm, _ = _llm()
    bank = _bank(llm, capacity=2, rank=8)
    with pytest.raises(ValueError):
        bank.load("big", _adapter(llm, 16, 1))                        # r > bank rank
    assert bank.names() == []
    sd = _adapter(llm, 4, 2)
    sd["llm.encoders.9.self_attn.linear_q.lora_A"] = torch.zeros(4, 128)
    with pytest.raises(KeyError):
        bank.load("stray", sd)                                        # a key that matches nothing
    assert bank.names() == []
    with pytest.raises(KeyError):
        bank.activate("nobody")
    with pytest.raises(ValueError):
        AdapterBank(llm=llm, rank=12, device="cpu")
    llm.llm_decoder = LoRALinear(llm.llm_decoder, r=4)                # a decode-path linear outside the six
    with pytest.raises(NotImplementedError):
        AdapterBank(llm=llm, rank=8, device="cpu")


def test_activate_writes_exactly_the_adapters_module_tensors():
    from cosyvoice_lora_finetune_framework_amd.adapters import BASE
    llm, _ = _llm()
    bank = _bank(llm, capacity=2, rank=8)
    sd4, sd8 = _adapter(llm, 4, 21), _adapter(llm, 8, 22)
    bank.load("r4", sd4)
    bank.load("r8", sd8, alpha=5.0)
    before = {n: p.detach().clone() for n, p in llm.named_parameters()}
    managed = lambda n: "lora_" in n and n.startswith("text_encoder.")      # noqa: E731
    assert sum(managed(n) for n in before) > 0

    def check(sd):
        for n, p in llm.named_parameters():
            if managed(n):
                assert torch.equal(p, sd[n] if sd is not None else torch.zeros_like(p)), n
            else:
                assert torch.equal(p, before[n]), n                   # base weights and the decode stack's own LoRA tensors

    bank.activate("r4")
    check(sd4)
    q = llm.text_encoder.encoders[0].self_attn.linear_q
    assert q.scaling == 8 / 4 and q.lora_A.shape[0] == 4
    bank.activate("r8")                                               # another rank: parameters of the adapter's shape
    check(sd8)
    assert q.scaling == 5.0 / 8 and q.r == 8 and tuple(q.lora_B.shape) == (128, 8)
    bank.activate(BASE)
    check(None)
    bank.activate("r4")
    check(sd4)
    assert q.scaling == 8 / 4
