"""Many fine-tuned voices over one base model: LoRA adapters kept resident and chosen per request at inference.

An ``AdapterBank`` is built over an LLM and / or a Flow whose target layers are LoRA-wrapped (``apply_lora_to_model``) and
whose frozen weights are the base.  It holds up to ``capacity`` named adapters:

  * the LLM decode stack (``llm.llm``: per layer q | k | v, linear_out, w_1, w_2) never goes through modules at inference
    -- csrc/decode.hip streams packed weights --, so those adapters live in fixed-address stacks, one set per weight
    dtype in use, that the decode kernels index per row (``cvft_decode_lora_down`` / ``cvft_decode_linear_lora``):

        A_qkv [S][3][R][d]   B_qkv [S][3d][R]        A_o [S][1][R][d]   B_o [S][d][R]
        A_1   [S][1][R][d]   B_1   [S][F][R]         A_2 [S][1][R][F]   B_2 [S][d][R]        scale [S] = alpha / r

    S = capacity, R = the bank rank; an adapter of rank r <= R is zero-padded (its scale keeps its own r).  A captured
    decode step holds these addresses, so loading, evicting or switching adapters neither repacks the base weights nor
    re-captures a graph.
  * every other LoRA layer (the LLM's text encoder, the whole Flow) runs through its module; the bank keeps the
    adapter's tensors on the device and ``activate(name)`` writes them into those modules' ``lora_A`` / ``lora_B``
    (in place; a module whose rank differs from the adapter's gets parameters of the adapter's shape) and sets the
    modules' ``scaling`` to the adapter's alpha / r.

``BASE`` stands for "no adapter": slot -1 in the decode stack, zeros in the modules.
"""
from __future__ import annotations

import collections
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .lora import LoRAConv1d, LoRALinear

RANKS = (8, 16, 32, 64)                  # bank ranks the decode kernels are built for
ROLES = (("qkv", ("self_attn.linear_q", "self_attn.linear_k", "self_attn.linear_v")), ("o", ("self_attn.linear_out",)),
         ("1", ("feed_forward.w_1",)), ("2", ("feed_forward.w_2",)))


class _Base:
    def __repr__(self):
        return "BASE"


BASE = _Base()


class BankStacks:
    """The decode-stack adapters of every slot in one weight dtype (see the module docstring); addresses never change."""

    def __init__(self, shapes: List[Dict[str, Tuple[int, int]]], capacity: int, rank: int, dtype, device):
        self.rank, self.dtype = rank, dtype
        self.scale = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.layers = []
        for sh in shapes:
            L = {}
            for role, (G, K, N) in sh.items():
                L["A_" + role] = torch.zeros((capacity, G, rank, K), dtype=dtype, device=device)
                L["B_" + role] = torch.zeros((capacity, N, rank), dtype=dtype, device=device)
            self.layers.append(L)

    def write(self, slot: int, scale: float, layers: List[Dict[str, torch.Tensor]]):
        self.scale[slot] = float(scale)
        for dst, src in zip(self.layers, layers):
            for k, t in src.items():
                dst[k][slot].copy_(t)

    def nbytes_per_slot(self) -> int:
        return 4 + sum(t[0].numel() * t.element_size() for L in self.layers for t in L.values())


class _Adapter:
    def __init__(self):
        self.mod: Dict[Tuple[str, str], torch.Tensor] = {}      # (branch, parameter name) -> tensor on the device
        self.mod_alpha: Dict[Tuple[str, str], float] = {}       # (branch, module name) -> alpha
        self.dec: Dict[Tuple[int, str, int], Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = {}   # host fp32
        self.r: Optional[int] = None
        self.alpha: Optional[float] = None


class AdapterBank:
    def __init__(self, llm: Optional[nn.Module] = None, flow: Optional[nn.Module] = None, capacity: int = 8, rank: int = 16,
                 device=None):
        if llm is None and flow is None:
            raise ValueError("AdapterBank needs an llm, a flow, or both")
        if rank not in RANKS:
            raise ValueError(f"bank rank {rank}: one of {RANKS}")
        if capacity < 1:
            raise ValueError("capacity >= 1")
        first = next((llm if llm is not None else flow).parameters())
        self.device = torch.device(device) if device is not None else first.device
        self.capacity, self.rank = int(capacity), int(rank)
        self.branches = {k: m for k, m in (("llm", llm), ("flow", flow)) if m is not None}
        self._shape = {k: {n: tuple(t.shape) for n, t in m.state_dict().items()} for k, m in self.branches.items()}
        self._names = {k: set(v) for k, v in self._shape.items()}
        # LoRA modules that run as modules at inference: (branch, module name) -> module; their alpha as built
        self._mods: Dict[Tuple[str, str], nn.Module] = {}
        self._alpha0: Dict[Tuple[str, str], float] = {}
        # decode-stack linears: parameter-name stem -> (layer, role, group)
        self._dec: Dict[str, Tuple[int, str, int]] = {}
        self._dec_alpha0: Dict[str, float] = {}
        self._shapes: List[Dict[str, Tuple[int, int, int]]] = []
        for br, model in self.branches.items():
            dec_stems = self._decode_stems(model) if br == "llm" else {}
            for name, mod in model.named_modules():
                if not isinstance(mod, (LoRALinear, LoRAConv1d)):
                    continue
                if br == "llm" and name in dec_stems:
                    self._dec[name] = dec_stems[name]
                    self._dec_alpha0[name] = float(mod.lora_alpha)
                elif br == "llm" and (name == "llm_decoder" or name.startswith("llm.")):
                    raise NotImplementedError(f"AdapterBank: the decode-path linear '{name}' is LoRA-wrapped; only the six "
                                              f"per-layer linears (q, k, v, linear_out, w_1, w_2) take adapters at decode")
                else:
                    self._mods[(br, name)] = mod
                    self._alpha0[(br, name)] = float(mod.lora_alpha)
        self._adapters: "collections.OrderedDict[str, _Adapter]" = collections.OrderedDict()    # least recently used first
        self._slot: Dict[str, int] = {}
        self._stacks: Dict[torch.dtype, BankStacks] = {}
        self._gen: Dict[str, int] = {}             # loads per name: what the modules hold is (name, generation)
        self._active = None
        for model in self.branches.values():
            model.__dict__["_cvft_adapter_bank"] = self

    # ---------------------------------------------------------------------------------------- structure
    def _decode_stems(self, llm) -> Dict[str, Tuple[int, str, int]]:
        stems = {}
        for i, layer in enumerate(llm.llm.encoders):
            d = layer.self_attn.linear_q
            d = (d.original_layer if isinstance(d, LoRALinear) else d).in_features
            w1 = layer.feed_forward.w_1
            F = (w1.original_layer if isinstance(w1, LoRALinear) else w1).out_features
            self._shapes.append({"qkv": (3, d, 3 * d), "o": (1, d, d), "1": (1, d, F), "2": (1, F, d)})
            for role, subs in ROLES:
                for g, sub in enumerate(subs):
                    stems[f"llm.encoders.{i}.{sub}"] = (i, role, g)
        return stems

    # ---------------------------------------------------------------------------------------- residency
    def names(self) -> List[str]:
        """resident adapters, least recently used first."""
        return list(self._adapters.keys())

    def slot(self, name) -> int:
        """the decode-stack slot of a resident adapter (-1 for BASE); counts as a use."""
        if name is BASE:
            return -1
        if name not in self._adapters:
            raise KeyError(f"adapter '{name}' is not resident (resident: {self.names()})")
        self._adapters.move_to_end(name)
        return self._slot[name]

    def evict(self, name: str) -> None:
        if name not in self._adapters:
            raise KeyError(f"adapter '{name}' is not resident")
        del self._adapters[name]
        s = self._slot.pop(name)
        for st in self._stacks.values():
            st.scale[s] = 0.0

    def stacks(self, dtype: torch.dtype) -> BankStacks:
        """the decode stacks in `dtype` (built on first use from the resident adapters; fixed addresses afterwards)."""
        if "llm" not in self.branches:
            raise ValueError("this AdapterBank was built without an llm")
        st = self._stacks.get(dtype)
        if st is None:
            st = self._stacks[dtype] = BankStacks(self._shapes, self.capacity, self.rank, dtype, self.device)
            for name, ad in self._adapters.items():
                self._write(st, self._slot[name], ad)
        return st

    def nbytes_per_voice(self, name: str) -> Dict[str, int]:
        """device bytes one resident voice takes: its slot of every decode stack in use + its module tensors."""
        ad = self._adapters[name]
        return {"decode_stacks": sum(st.nbytes_per_slot() for st in self._stacks.values()),
                "module_tensors": sum(t.numel() * t.element_size() for t in ad.mod.values())}

    # ---------------------------------------------------------------------------------------- loading
    def _resolve(self, key: str) -> Optional[Tuple[str, str]]:
        """checkpoint key -> (branch, state-dict name): the prefix handling of merge_joint_weights._fill_branch
        (``model.<branch>.`` / ``<branch>.`` / bare), tried on every branch the bank holds."""
        for br in self.branches:
            for p in (f"model.{br}.", f"{br}."):
                if key.startswith(p) and key[len(p):] in self._names[br]:
                    return br, key[len(p):]
        for br in self.branches:
            if key in self._names[br]:
                return br, key
        return None

    def load(self, name: str, state_or_path, alpha: Optional[float] = None) -> int:
        """Make adapter `name` resident from what ``save_lora_weights`` writes for a branch, or from a trainer
        checkpoint (``{'state_dict': ...}`` or bare, any of the prefixes above).  Loading into a resident name adds to /
        replaces its tensors (one file per branch: two calls).  alpha: the adapter's lora_alpha (default: the alpha the
        wrapped modules were built with).  A full bank evicts the least recently used name.  Keys that name nothing in
        the models raise KeyError; non-LoRA keys that name a base parameter are the base and are not the bank's to
        take.  Returns the slot."""
        if name is BASE or not isinstance(name, str):
            raise ValueError("adapter names are strings (BASE is reserved)")
        state = state_or_path
        if not isinstance(state, dict):
            state = torch.load(state_or_path, map_location="cpu", weights_only=True)
        state = state.get("state_dict", state)
        ad = self._adapters.get(name)
        new = _Adapter() if ad is None else ad
        staged_mod, staged_dec, unmatched = {}, {}, []
        for key, value in state.items():
            hit = self._resolve(key)
            if hit is None:
                unmatched.append(key)
                continue
            if "lora_" not in hit[1]:
                continue
            br, pname = hit
            stem, leaf = pname.split(".lora_", 1)
            which = leaf[0]                                     # 'A' / 'B' (LoRAConv1d: 'A.weight')
            if br == "llm" and stem in self._dec:
                staged_dec.setdefault(stem, {})[which] = value.detach().float().cpu()
            else:
                staged_mod[(br, pname)] = value.detach().float()
        if unmatched:
            raise KeyError(f"adapter '{name}': {len(unmatched)} keys match nothing in the models, e.g. {unmatched[:3]}")
        if not staged_mod and not staged_dec:
            raise KeyError(f"adapter '{name}': no LoRA tensors found")
        # decode stack: shapes, one rank, r <= bank rank
        r = new.r
        for stem, ab in staged_dec.items():
            i, role, g = self._dec[stem]
            G, K, N = self._shapes[i][role]
            A, B = ab.get("A"), ab.get("B")
            if A is None or B is None:
                raise KeyError(f"adapter '{name}': {stem} needs both lora_A and lora_B")
            if A.shape[1] != K or B.shape[0] != N // G or A.shape[0] != B.shape[1]:
                raise ValueError(f"adapter '{name}': {stem} has lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)}, the "
                                 f"layer is {K} -> {N // G}")
            if r is not None and A.shape[0] != r:
                raise ValueError(f"adapter '{name}': ranks {r} and {A.shape[0]} in one decode stack")
            r = A.shape[0]
        if r is not None and r > self.rank:
            raise ValueError(f"adapter '{name}' has rank {r} > bank rank {self.rank}")
        for (br, pname), t in staged_mod.items():
            want = self._shape[br][pname]                            # (as built: only the rank may differ later)
            keep = (lambda sh: tuple(sh[1:])) if ".lora_A" in pname else (lambda sh: tuple(sh[:1] + sh[2:]))   # all but r
            if keep(t.shape) != keep(want):
                raise ValueError(f"adapter '{name}': {pname} has shape {tuple(t.shape)}, the layer's is {tuple(want)}")
        # commit
        for stem, ab in staged_dec.items():
            new.dec[self._dec[stem]] = (ab["A"], ab["B"])
        if staged_dec:
            new.r = r
            new.alpha = float(alpha) if alpha is not None else self._dec_alpha0[next(iter(staged_dec))]
        for (br, pname), t in staged_mod.items():
            new.mod[(br, pname)] = t.to(self.device)
            mname = pname.split(".lora_", 1)[0]
            new.mod_alpha[(br, mname)] = float(alpha) if alpha is not None else self._alpha0[(br, mname)]
        if ad is None:
            if len(self._adapters) >= self.capacity:
                self.evict(next(iter(self._adapters)))
            used = set(self._slot.values())
            self._slot[name] = next(s for s in range(self.capacity) if s not in used)
            self._adapters[name] = new
        self._adapters.move_to_end(name)
        self._gen[name] = self._gen.get(name, 0) + 1
        for st in self._stacks.values():
            self._write(st, self._slot[name], new)
        return self._slot[name]

    def _padded(self, ad: _Adapter) -> List[Dict[str, torch.Tensor]]:
        """the adapter's decode tensors in the stacks' per-slot layout (host fp32, zero-padded to the bank rank)."""
        R, out = self.rank, []
        for i, sh in enumerate(self._shapes):
            L = {}
            for role, (G, K, N) in sh.items():
                A, B = torch.zeros(G, R, K), torch.zeros(N, R)
                for g in range(G):
                    a, b = ad.dec.get((i, role, g), (None, None))
                    if a is not None:
                        A[g, :a.shape[0]] = a
                        B[g * (N // G):(g + 1) * (N // G), :b.shape[1]] = b
                L["A_" + role], L["B_" + role] = A, B
            out.append(L)
        return out

    def _write(self, st: BankStacks, slot: int, ad: _Adapter) -> None:
        st.write(slot, (ad.alpha / ad.r) if ad.r else 0.0, self._padded(ad))

    # ---------------------------------------------------------------------------------------- modules
    @torch.no_grad()
    def activate(self, name, force: bool = False) -> None:
        """write adapter `name` (BASE: zeros) into the LoRA modules that run as modules at inference -- the LLM's text
        encoder, every Flow LoRA layer --; LoRA layers the adapter has no tensors for are zeroed.  Counts as a use.
        Nothing is copied when the bank's last activation already wrote this load of `name` (force=True copies anyway:
        for LoRA parameters changed behind the bank's back)."""
        ad = None
        if name is not BASE:
            if name not in self._adapters:
                raise KeyError(f"adapter '{name}' is not resident (resident: {self.names()})")
            self._adapters.move_to_end(name)
            ad = self._adapters[name]
        key = (name, self._gen.get(name) if name is not BASE else 0)
        if self._active == key and not force:
            return
        self._active = key
        for (br, mname), mod in self._mods.items():
            conv = isinstance(mod, LoRAConv1d)
            r_new = None
            for which in ("A", "B"):
                pname = f"{mname}.lora_{which}" + (".weight" if conv else "")
                holder = getattr(mod, "lora_" + which) if conv else mod
                attr = "weight" if conv else "lora_" + which
                p = getattr(holder, attr)
                t = ad.mod.get((br, pname)) if ad is not None else None
                if t is None:
                    p.zero_()
                elif t.shape == p.shape:
                    p.copy_(t)
                else:
                    setattr(holder, attr, nn.Parameter(t.to(device=p.device, dtype=p.dtype).clone(), requires_grad=p.requires_grad))
                if t is not None and which == "A":
                    r_new = t.shape[0]
            if r_new is not None:
                mod.r, mod.lora_alpha = r_new, ad.mod_alpha[(br, mname)]
                mod.scaling = mod.lora_alpha / r_new


def bank_of(model: nn.Module) -> AdapterBank:
    bank = model.__dict__.get("_cvft_adapter_bank")
    if bank is None:
        raise RuntimeError("adapter= needs an adapters.AdapterBank built over this model")
    return bank
