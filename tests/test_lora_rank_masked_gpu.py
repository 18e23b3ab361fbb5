"""Masked form of the LoRA adapter-gradient slab kernels (csrc/lora_grad.hip, cvft_lora_rank_partial_*_masked): the wide operand
drop_site(x) of dA = V^T drop(x) is re-derived from the counter-based mask while the chunk sits in LDS, instead of read from a
copy the forward pass wrote.

Bitwise: a masked launch on x equals the unmasked launch on dropout_raw(x, p, site) bit for bit (same operand values, same
products, same order).  fp64: against Rk^T drop(x) in fp64, drop(x) built from the host replica of the mask (tests/helpers.py)
and rounded to bf16 as the operand is by definition (bf16(x * 1/(1-p))), under the tolerance of
test_ops_gpu.py::test_lora_rank_partial_batch_matches_torch (1e-5).  Module level: LinearFn and the stacked q|k|v Function with
CVFT_RANK_MASK=1 and 0 in fresh child processes: equal gradients, no dropped copy on the new path.

Shapes: M in {33, 100, 300, 515} against rows_per_block 64 (one wave per stripe and slab), 128 (stacked four-wave form: with
M = 33 the second wave has one row and the last two start past M) and 256; C = 72 is no multiple of the 64-column stripe (the
chunk clamp), 64 one stripe, 256 one whole block of stripes; r = 16 and 48; p = 0.05 / 0.15 under two seeds."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import keep_scale_host, rel

pytestmark = pytest.mark.gpu

DEV = "cuda"
MS = (33, 100, 300, 515)
RPBS = (64, 128, 256)
CS = (64, 72, 256)
RS = (16, 48)
DRAWS = ((0.05, 1234567), (0.15, 987654321))          # (p, seed)
NB = 72                                                # width of the unmasked dB-like product that shares the launches


def HFmod():
    from cosyvoice_lora_finetune_framework_amd.hipops import functional as HF
    return HF


def cbmod():
    from cosyvoice_lora_finetune_framework_amd.hipops import binding as cb
    return cb


_OPS = {}


def operands(M, Cn, r):
    """x [M, Cn], V [M, r], dY [M, NB], U [M, r] (bf16, made once per shape and never written)"""
    key = (M, Cn, r)
    if key not in _OPS:
        g = torch.Generator().manual_seed(M * 1000 + Cn + r)
        _OPS[key] = tuple(torch.randn(M, n, generator=g).to(DEV, torch.bfloat16) for n in (Cn, r, NB, r))
    return _OPS[key]


def set_seed(seed):
    HF = HFmod()
    if HF._DROPOUT["seed"] is None:
        HF.dropout_begin_step()
    HF._DROPOUT["seed"].fill_(seed)
    return HF._DROPOUT["seed"]


def slabs(M, rpb, r, Cn):
    return torch.full((-(-M // rpb) * r * Cn,), float("nan"), dtype=torch.float32, device=DEV)


def fp64_ref(x, Rk, seed, site, p):
    """Rk^T bf16(x * keep / (1 - p)) in fp64, the mask from the host replica"""
    M, Cn = x.shape
    keep = (keep_scale_host(seed, site, M * Cn, p).reshape(M, Cn) > 0).to(DEV)
    inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    xd = torch.where(keep, x.float() * inv.to(DEV), torch.zeros((), device=DEV)).to(torch.bfloat16)
    return Rk.double().t() @ xd.double()


@pytest.mark.parametrize("rpb", RPBS)
@pytest.mark.parametrize("M", MS)
def test_pair_masked_equals_unmasked_on_dropped_copy(M, rpb):
    HF, cb = HFmod(), cbmod()
    L = cb.lib()
    for Cn in CS:
        for r in RS:
            x, V, dY, U = operands(M, Cn, r)
            for site, (p, seed) in enumerate(DRAWS, start=3):
                sd = set_seed(seed)
                xd = HF.dropout_raw(x, p, site)
                assert not torch.equal(xd, x)
                gotA, gotB, refA, refB = slabs(M, rpb, r, Cn), slabs(M, rpb, r, NB), slabs(M, rpb, r, Cn), slabs(M, rpb, r, NB)
                cb.check(L.cvft_lora_rank_partial_pair(M, r, Cn, cb.ptr(xd), Cn, cb.ptr(V), r, cb.ptr(refA), rpb,
                                                       NB, cb.ptr(dY), NB, cb.ptr(U), r, cb.ptr(refB), rpb, None), "pair")
                cb.check(L.cvft_lora_rank_partial_pair_masked(M, r, Cn, cb.ptr(x), Cn, cb.ptr(V), r, cb.ptr(gotA), rpb,
                                                              NB, cb.ptr(dY), NB, cb.ptr(U), r, cb.ptr(gotB), rpb,
                                                              cb.ptr(sd), site, p, None), "pair_masked")
                torch.cuda.synchronize()
                assert torch.equal(gotA, refA), (Cn, r, p, "dA slabs differ", float((gotA - refA).abs().max()))
                assert torch.equal(gotB, refB), (Cn, r, p, "dB slabs differ")
                ns = -(-M // rpb)
                e = rel(gotA.view(ns, r, Cn).sum(0), fp64_ref(x, V, seed, site, p))
                assert e < 1e-5, (Cn, r, p, e)


def _multi_args(cb, masked, M, r, rpb, wides, Vs, Cn, dY, U, outs, sites, p, seed_t):
    """three rank-r products on `wides` (sites[i]) and one transposed dB-like product on dY (unmasked) as one multi launch"""
    arr = ((cb.RankProbMasked if masked else cb.RankProb) * 4)()
    for i in range(4):
        q = arr[i].prob if masked else arr[i]
        Wd, Rk, C_, tr = (wides[i], Vs[i], Cn, 0) if i < 3 else (dY, U, NB, 1)
        q.C, q.Wd, q.ldw, q.Rk, q.ldr, q.part = C_, Wd.data_ptr(), Wd.stride(0), Rk.data_ptr(), Rk.stride(0), outs[i].data_ptr()
        q.transpose_out, q.rows_per_block = tr, rpb
        if masked:
            arr[i].seed, arr[i].site, arr[i].p = (seed_t.data_ptr(), sites[i], p) if i < 3 else (None, cb.RANK_UNMASKED, 0.0)
    return arr


@pytest.mark.parametrize("rpb", RPBS)
@pytest.mark.parametrize("M", MS)
def test_multi_masked_three_sites_on_one_x(M, rpb):
    """the stacked q|k|v form: three mask sites on ONE x, plus a problem carrying the unmasked marker, in one launch"""
    HF, cb = HFmod(), cbmod()
    L = cb.lib()
    ns = -(-M // rpb)
    for Cn in CS:
        r = 16
        x, V, dY, U = operands(M, Cn, r)
        V3 = operands(M, Cn, 48)[1]                                 # [M, 48]: adapter i reads columns 16 i .. 16 i + 15
        Vs = [V3[:, 16 * i:16 * (i + 1)] for i in range(3)]
        for p, seed in DRAWS:
            sd = set_seed(seed)
            sites = [7, 8, 9]
            xds = [HF.dropout_raw(x, p, st) for st in sites]
            got = [slabs(M, rpb, r, Cn) for _ in range(3)] + [slabs(M, rpb, r, NB)]
            ref = [slabs(M, rpb, r, Cn) for _ in range(3)] + [slabs(M, rpb, r, NB)]
            a0 = _multi_args(cb, False, M, r, rpb, xds, Vs, Cn, dY, U, ref, sites, p, sd)
            a1 = _multi_args(cb, True, M, r, rpb, [x, x, x], Vs, Cn, dY, U, got, sites, p, sd)
            cb.check(L.cvft_lora_rank_partial_multi(M, r, 4, a0, None), "multi")
            cb.check(L.cvft_lora_rank_partial_multi_masked(M, r, 4, a1, None), "multi_masked")
            torch.cuda.synchronize()
            for i in range(4):
                assert torch.equal(got[i], ref[i]), (Cn, p, i)
            assert not torch.equal(got[0], got[1])                  # (three different masks)
            for i in range(3):
                e = rel(got[i].view(ns, r, Cn).sum(0), fp64_ref(x, Vs[i], seed, sites[i], p))
                assert e < 1e-5, (Cn, p, i, e)
            e = rel(got[3].view(ns, NB, r).sum(0).t(), U.double().t() @ dY.double())
            assert e < 1e-5, ("unmasked", Cn, p, e)


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("rpb", RPBS)
def test_batch_masked_problems_of_different_row_counts(r, rpb):
    """every (M, C) as a masked problem of its own site, unmasked problems in between, 52 problems: two launches (48 + 4)"""
    HF, cb = HFmod(), cbmod()
    L = cb.lib()
    p, seed = DRAWS[r == 48]
    sd = set_seed(seed)
    shapes = [(M, Cn) for M in MS for Cn in CS]
    plan = []                                                        # (wide, Rk, C, transpose_out, site or None)
    for rep in range(4):
        for j, (M, Cn) in enumerate(shapes):
            x, V, dY, U = operands(M, Cn, r)
            plan.append((x, V, Cn, 0, 20 + rep * len(shapes) + j))
        x, V, dY, U = operands(MS[rep], CS[0], r)
        plan.append((dY, U, NB, 1, None))
    assert len(plan) == 52
    copies = {}
    a0, a1 = (cb.RankProbM * len(plan))(), (cb.RankProbMMasked * len(plan))()
    keep = []
    for i, (Wd, Rk, C_, tr, site) in enumerate(plan):
        M = Wd.shape[0]
        src = Wd
        if site is not None:
            src = copies[i] = HF.dropout_raw(Wd, p, site)
        ref, got = slabs(M, rpb, r, C_), slabs(M, rpb, r, C_)
        keep.append((ref, got))
        for q, w, out in ((a0[i], src, ref), (a1[i].prob, Wd, got)):
            q.M, q.C, q.Wd, q.ldw, q.Rk, q.ldr, q.part, q.transpose_out, q.rows_per_block = M, C_, w.data_ptr(), C_, Rk.data_ptr(), r, out.data_ptr(), tr, rpb
        a1[i].seed, a1[i].site, a1[i].p = (sd.data_ptr(), site, p) if site is not None else (None, cb.RANK_UNMASKED, 0.0)
    cb.check(L.cvft_lora_rank_partial_batch(r, len(plan), a0, None), "batch")
    cb.check(L.cvft_lora_rank_partial_batch_masked(r, len(plan), a1, None), "batch_masked")
    torch.cuda.synchronize()
    for i, ((ref, got), (Wd, Rk, C_, tr, site)) in enumerate(zip(keep, plan)):
        assert torch.equal(got, ref), (i, Wd.shape, tr, site)
        if i < 13:                                                   # one of each shape and the first unmasked problem
            ns = -(-Wd.shape[0] // rpb)
            if site is None:
                e = rel(got.view(ns, C_, r).sum(0).t(), Rk.double().t() @ Wd.double())
            else:
                e = rel(got.view(ns, r, C_).sum(0), fp64_ref(Wd, Rk, seed, site, p))
            assert e < 1e-5, (i, Wd.shape, site, e)


def test_masked_entries_reject_bad_dropout_args():
    """p outside [2^-16, 1 - 2^-16], a missing seed, or a masked problem whose rows are not contiguous (ldw != C): an error"""
    HF, cb = HFmod(), cbmod()
    L = cb.lib()
    M, Cn, r, rpb = 100, 64, 16, 64
    x, V, dY, U = operands(M, Cn, r)
    sd = set_seed(5)
    oA, oB = slabs(M, rpb, r, Cn), slabs(M, rpb, r, NB)

    def pair(xx, ldx, seed_ptr, site, p):
        return L.cvft_lora_rank_partial_pair_masked(M, r, Cn, cb.ptr(xx), ldx, cb.ptr(V), r, cb.ptr(oA), rpb, NB, cb.ptr(dY), NB,
                                                    cb.ptr(U), r, cb.ptr(oB), rpb, seed_ptr, site, p, None)
    assert pair(x, Cn, cb.ptr(sd), 3, 0.05) == 0
    assert pair(x, Cn, cb.ptr(sd), 3, 1e-6) != 0
    assert pair(x, Cn, cb.ptr(sd), 3, 1.0) != 0
    assert pair(x, Cn, cb.ptr(sd), 3, 0.0) != 0
    assert pair(x, Cn, None, 3, 0.05) != 0
    wide = torch.zeros(M, Cn + 8, dtype=torch.bfloat16, device=DEV)
    assert pair(wide, Cn + 8, cb.ptr(sd), 3, 0.05) != 0
    assert pair(wide, Cn + 8, None, cb.RANK_UNMASKED, 0.0) == 0      # unmasked marker: a plain product, any row pitch
    torch.cuda.synchronize()


def test_modules_equal_gradients_and_no_dropped_copy(tmp_path):
    """LinearFn and LinearQKVStackedFn (in line and postponed) in train mode, CVFT_RANK_MASK=1 against 0 in fresh processes:
    the same gradients bit for bit; with the mask re-derived in the slab launch nothing is parked in _DROPPED and the step's
    peak allocation is lower by at least the copies ([M][K] bf16: one for the linear, three for q|k|v)."""
    here = os.path.dirname(os.path.abspath(__file__))
    kids = {}
    for v in ("1", "0"):
        env = dict(os.environ, CVFT_RANK_MASK=v)
        kids[v] = subprocess.Popen([sys.executable, os.path.join(here, "rank_mask_worker.py"), str(tmp_path / f"rm{v}.pt")], env=env,
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    for v, k in kids.items():
        out, _ = k.communicate(timeout=240)
        assert k.returncode == 0, out.decode()[-3000:]
    on, off = torch.load(tmp_path / "rm1.pt"), torch.load(tmp_path / "rm0.pt")
    assert on["rank_mask"] is True and off["rank_mask"] is False
    M, K = 1000, 256
    copy = M * K * 2
    for name, ncopies in (("linear", 1), ("qkv_defer0", 3), ("qkv_defer1", 3)):
        a, b = on[name], off[name]
        print(f"[rank mask] {name}: held {a['held']} / {b['held']} copies, peak {a['peak']} / {b['peak']} B (copies {ncopies * copy} B)")
        for ga, gb in zip(a["grads"], b["grads"]):
            assert torch.equal(ga, gb), name
            assert float(ga.abs().sum()) > 0
        assert torch.equal(a["dx"], b["dx"]), name
        assert a["held"] == 0 and b["held"] == ncopies, (name, a["held"], b["held"])
        assert b["peak"] - a["peak"] >= ncopies * copy, (name, a["peak"], b["peak"])
