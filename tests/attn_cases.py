"""Inputs of the attention-oracle tests, shared by the CPU file (the fp32 reference alone must pass
the bound on them) and the GPU file (the HIP kernels must).  Everything is generated on the CPU
from fixed seeds and rounded to bf16 once, so both files see bit-identical inputs.

A case is the PADDED problem the oracle solves -- qkv [B*S, 3*H*64], dctx [B*S, H*64], a [B, S]
0/1 mask -- plus how the kernels are to be driven (layout, lens, q_live, short).  Varlen cases
keep ``lens`` (zeros allowed): the oracle's mask is their prefix mask, with key 0 of an empty
sequence switched on so that no oracle row is empty (nothing of such a sequence is ever compared:
it owns no packed row), and dctx is zero on the padding rows, which the packed layout does not have.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import torch

GROUPS = ("lengths", "masks", "heads", "range", "varlen", "q_live", "dropout")
FILLER = 64  # varlen: zero rows appended after the last sequence


@dataclass
class Case:
    group: str
    name: str
    S: int
    H: int
    mask: torch.Tensor            # [B, S] int64, the oracle's mask
    p: float
    seed: int
    scale: float = 1.0
    lens: Optional[List[int]] = None   # varlen (packed) layout
    q_live: int = 0
    short: bool = False
    plant: Optional[List[int]] = None  # range: the planted key of each batch row
    counter: int = field(init=False)
    site: int = field(init=False)

    def __post_init__(self):
        self.counter, self.site = 3 + self.seed % 11, 16 + 4 * (self.seed % 6)

    @property
    def B(self):
        return self.mask.shape[0]

    @property
    def varlen(self):
        return self.lens is not None

    def inputs(self):
        """(qkv bf16 [B*S, 3D], dctx bf16 [B*S, D]) of the padded problem, on the CPU."""
        B, S, H = self.B, self.S, self.H
        g = torch.Generator().manual_seed(1000 + self.seed)
        qkv = torch.randn(B * S, 3 * H * 64, generator=g) * self.scale
        dctx = torch.randn(B * S, H * 64, generator=g)
        if self.plant is not None:
            # one key per row of the batch that every query scores > 20 above all others: feature 0
            # is 32 on every query, 22 on the planted key and 0 on every other key -> +88 on its
            # score, against a spread of about 60 of the N(0, 9) rest (the CPU file asserts the lead);
            # no more than that, so that the other keys' probabilities stay above fp32 underflow
            x = qkv.view(B, S, 3, H, 64)
            x[:, :, 0, :, 0] = 32.0
            x[:, :, 1, :, 0] = 0.0
            for b, k in enumerate(self.plant):
                x[b, k, 1, :, 0] = 22.0
        if self.varlen:
            rows = torch.arange(S)[None, :] < torch.tensor(self.lens)[:, None]
            dctx = dctx * rows.reshape(-1, 1)
        if self.q_live:
            first = torch.zeros(B, S, 1)
            first[:, :self.q_live] = 1.0
            dctx = dctx * first.reshape(-1, 1)
        return qkv.to(torch.bfloat16), dctx.to(torch.bfloat16)

    def packed_rows(self):
        """varlen: indices of the real tokens in the padded layout, in packed order."""
        rows = torch.arange(self.S)[None, :] < torch.tensor(self.lens)[:, None]
        return torch.nonzero(rows.reshape(-1)).squeeze(1)


def prefix(lens, S):
    m = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    m[:, 0] = 1  # (an empty varlen sequence: see the module docstring)
    return m


def _rand_lens(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, S + 1, (B,), generator=g).tolist()


def mask_patterns(S):
    """The masks group's four rows."""
    k = torch.arange(S)
    dead0 = 16 if S == 64 else 64
    return torch.stack([k >= dead0,                       # (i) first key tile dead
                        (k // 16) % 2 == 1,               # (ii) alternating 16-key blocks, first dead
                        k == S - 1,                       # (iii) only the last key live
                        (k < 16) | (k >= 48)]).long()     # (iv) all live but keys 16..47


def varlen_batches(S):
    """Every length of {1, 63, 64, 65, 128, 129, S} that fits S, two per batch, between a leading
    and a trailing empty sequence."""
    vals = sorted({v for v in (1, 63, 64, 65, 128, 129, S) if v <= S}, reverse=True)
    if len(vals) % 2:
        vals.append(1)
    half = len(vals) // 2
    return [[0, a, b, 0] for a, b in zip(vals[:half], vals[half:])]  # a long one beside a short one


def group_cases(group):
    out, n = [], [GROUPS.index(group) * 100]

    def add(name, S, H, mask, p, **kw):
        n[0] += 1
        out.append(Case(group, name, S, H, mask, p, n[0], **kw))

    if group == "lengths":
        for S in range(64, 513, 64):
            for p in (0.0, 0.1):
                add(f"S{S}-p{p}", S, 2, prefix([S, 1, S - 63], S), p)
    elif group == "masks":
        for S in (64, 128, 192, 512):
            for p in (0.0, 0.1):
                add(f"S{S}-p{p}", S, 2, mask_patterns(S), p)
    elif group == "heads":
        for S in (128, 192):
            for H in (1, 3, 12):
                for p in (0.0, 0.1):
                    add(f"S{S}-H{H}-p{p}", S, H, prefix(_rand_lens(2, S, 10 * S + H), S), p)
    elif group == "range":
        for S in (128, 256):
            # batch row 0: planted in the first key tile; row 1: in the last one (a prefix mask that
            # keeps it live, so the late tile brings the new maximum)
            add(f"S{S}", S, 2, prefix([S, S - 7], S), 0.0, scale=3.0, plant=[5, S - 10])
    elif group == "varlen":
        for S in (128, 192, 320, 512):
            for i, lens in enumerate(varlen_batches(S)):
                for p in (0.0, 0.1):
                    add(f"S{S}-b{i}-p{p}", S, 2, prefix(lens, S), p, lens=lens)
        for p in (0.0, 0.1):
            add(f"S256-short-p{p}", 256, 2, prefix([0, 128, 65, 0], 256), p, lens=[0, 128, 65, 0], short=True)
    elif group == "q_live":
        for S in (64, 128):
            for p in (0.0, 0.1):
                add(f"S{S}-padded-p{p}", S, 2, prefix([S, 1, S - 27, 17], S), p, q_live=1)
                lens = [0, S - 27, 1, S]
                add(f"S{S}-varlen-p{p}", S, 2, prefix(lens, S), p, lens=lens, q_live=1)
    elif group == "dropout":
        for S in (128, 320):
            add(f"S{S}", S, 2, prefix([S, S // 2 + 3], S), 0.5)
    else:
        raise KeyError(group)
    return out


def all_cases():
    return [c for g in GROUPS for c in group_cases(g)]
