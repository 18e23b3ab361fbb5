"""The HiFT vocoder's host side (no GPU): state-dict keys, legacy weight-norm names, the weight-norm fold, unsupported
settings, exported symbols, and that the ops refuse CPU tensors."""
import json
import os

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _hift():
    from cosyvoice_lora_finetune_framework_amd import hift
    return hift


def test_state_dict_keys_are_the_reference_ones():
    meta = json.load(open(os.path.join(GOLD, "hift_meta.json")))
    sd = _hift().HiFTGenerator().state_dict()
    assert len(meta["keys"]) == 227
    assert sorted(sd.keys()) == sorted(meta["keys"])
    assert "conv_pre.parametrizations.weight.original0" in sd
    assert sum(v.numel() for v in sd.values()) == 20_460_591


def test_legacy_weight_norm_names_load():
    h = _hift()
    a, b = h.HiFTGenerator(), h.HiFTGenerator()
    legacy = {}
    for k, v in a.state_dict().items():
        k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        legacy[k] = v + 0.25
    assert any(k.endswith("weight_g") for k in legacy)
    b.load_state_dict(legacy, strict=True)
    for (k, x), y in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(x + 0.25, y), k


@pytest.mark.parametrize("shape", [(512, 80, 7), (256, 256, 11), (512, 256, 16), (256, 128, 16), (18, 128, 7)])
def test_weight_norm_fold_is_torchs(shape):
    """Conv1d [out, in, k] and ConvTranspose1d [in, out, k] shapes: the norm runs over every dim but 0."""
    g = torch.Generator().manual_seed(3)
    v = torch.randn(shape, generator=g)
    gg = torch.randn(shape[0], 1, 1, generator=g)
    want = torch._weight_norm(v, gg, 0)
    got = _hift().fold_weight_norm(gg, v)
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
    # and what the parametrised module itself computes
    m = torch.nn.utils.parametrizations.weight_norm(torch.nn.ConvTranspose1d(8, 6, 16, 8, padding=4))
    p = m.parametrizations.weight
    assert torch.allclose(_hift().fold_weight_norm(p.original0, p.original1), m.weight, atol=1e-7)


@pytest.mark.parametrize("kw, word", [
    (dict(sampling_rate=24000), "sampling_rate"),
    (dict(base_channels=480), "base_channels"),
    (dict(istft_params={"n_fft": 32, "hop_len": 8}), "istft_params"),
    (dict(upsample_rates=[8, 5], upsample_kernel_sizes=[16, 11]), "upsample_rates"),
    (dict(resblock_kernel_sizes=[3, 7, 13]), "kernel_size"),
    (dict(f0_predictor=torch.nn.Linear(2, 2)), "f0_predictor"),
])
def test_unsupported_settings_raise(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _hift().HiFTGenerator(**kw)


def test_hift_symbols_are_exported():
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    if not os.path.exists(cb.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = cb.lib()
    for name in ("cvft_hift_conv", "cvft_hift_conv_small", "cvft_hift_scan", "cvft_hift_source", "cvft_hift_stft",
                 "cvft_hift_istft"):
        assert name in cb.SIGNATURES and hasattr(lib, name), name


def test_ops_raise_on_cpu_tensors():
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    h = _hift()
    with pytest.raises(cb.CvftError):
        h.stft(torch.zeros(1, 64))
    with pytest.raises(cb.CvftError):
        h.scan(torch.zeros(2, 8), 8)
    with pytest.raises(cb.CvftError):
        h.istft(torch.zeros(9, 18), 1)
    pk = h.pack_conv1d(torch.zeros(64, 64, 3), None, 1, torch.float32)
    with pytest.raises(cb.CvftError):
        h.hift_conv(torch.zeros(8, 64), pk, 1, 8)
    with pytest.raises(cb.CvftError):
        h.HiFTGenerator().inference(torch.zeros(1, 80, 4))


def test_flop_count_matches_the_issues_estimate():
    h = _hift()
    per_frame = h.conv_flops(h.HiFTGenerator(), 1000) / 1000
    assert 0.55e9 < per_frame < 0.65e9
