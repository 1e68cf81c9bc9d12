"""The float64 attention oracle and its error bound (ops/reference.py attention_oracle), without a GPU.

Three things make the bound usable as the GPU tests' net (tests/test_attention_oracle_gpu.py):
 * the oracle's explicit backward is the float64 autograd of its own forward;
 * the fp32 ``attention_ref`` with bf16 outputs -- a correct implementation -- stays inside the bound
   on the inputs of every GPU case, and none of those cases has an empty mask row;
 * typical kernel faults, injected into a float64 copy of the computation and rounded to bf16,
   exceed it.
"""
import math

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import reference as R
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops.dropout import keep_mask

import attn_cases as AC

LSE_TOL = 1e-3


def _parts(H):
    D = H * 64
    return {"dq": slice(0, D), "dk": slice(D, 2 * D), "dv": slice(2 * D, 3 * D)}


def ratios(orc, ctx, dqkv, H, rows=None):
    """err / (2.5 u E) of ctx and the three thirds of dqkv (``rows``: the ctx rows to compare)."""
    sel = slice(None) if rows is None else rows
    out = {"ctx": R.attention_bound_ratio(ctx[sel], orc["ctx"][sel], orc["A"][sel])}
    for name, sl in _parts(H).items():
        out[name] = R.attention_bound_ratio(dqkv[:, sl], orc["dqkv"][:, sl], orc["E"][:, sl])
    return out


def test_oracle_backward_is_autograd_of_its_forward():
    B, S, H, p = 2, 128, 2, 0.1
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * S, 3 * H * 64, generator=g, dtype=torch.float64)
    dctx = torch.randn(B * S, H * 64, generator=g, dtype=torch.float64)
    for mask in (AC.prefix([S, 37], S), AC.mask_patterns(S)[1:3]):
        q = qkv.clone().requires_grad_(True)
        orc = R.attention_oracle(q, mask, B, S, H, p, 5, 20, dctx)
        (gr,) = torch.autograd.grad(orc["ctx"], q, dctx)
        rel = ((orc["dqkv"].detach() - gr).abs().max() / gr.abs().max()).item()
        print(f"explicit dqkv vs autograd: {rel:.3e}")
        assert rel < 1e-10
        # lse and the forward against the fp32 reference's definitions, in float64
        rctx, rlse = R.attention_ref(qkv, mask, B, S, H, p, 5, 20)
        assert (orc["ctx"].detach() - rctx).abs().max().item() < 1e-12
        assert (orc["lse"].detach() - rlse).abs().max().item() < 1e-12


def test_bound_ratio_zero_sum_demands_exact_zero():
    E = torch.tensor([0.0, 1.0])
    want = torch.tensor([0.0, 1.0])
    assert R.attention_bound_ratio(torch.tensor([0.0, 1.0]), want, E) == 0.0
    assert R.attention_bound_ratio(torch.tensor([1e-20, 1.0]), want, E) > 1e9
    assert R.attention_bound_ratio(torch.tensor([0.0, 1.0 + 2.4 * R.BF16_U]), want, E) < 1.0
    assert R.attention_bound_ratio(torch.tensor([0.0, 1.0 + 2.6 * R.BF16_U]), want, E) > 1.0
    assert R.attention_bound_ratio(torch.tensor([0.0, float("nan")]), want, E) == math.inf


@pytest.mark.parametrize("group", AC.GROUPS)
def test_fp32_reference_passes_the_bound_on_the_gpu_cases(group):
    """``attention_ref`` in fp32 with bf16-rounded outputs is a correct implementation with fewer
    roundings than the kernels: it must pass the GPU tests' assertion on every case's inputs."""
    worst = {}
    for c in AC.group_cases(group):
        B, S, H = c.B, c.S, c.H
        assert c.mask.sum(1).min().item() >= 1, c.name
        qkv, dctx = c.inputs()
        if c.plant is not None:
            x = qkv.double().view(B, S, 3, H, 64)
            s = torch.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1]) * 0.125
            s = s.masked_fill(c.mask.view(B, 1, 1, S) == 0, float("-inf"))
            for b, k in enumerate(c.plant):
                rest = s[b].clone()
                rest[:, :, k] = float("-inf")
                gap = (s[b, :, :, k] - rest.max(-1).values).min().item()
                print(f"{c.name} row {b}: planted key {k} leads by {gap:.1f}")
                assert gap > 20 and c.mask[b, k] == 1
        orc = R.attention_oracle(qkv, c.mask, B, S, H, c.p, c.counter, c.site, dctx)
        q = qkv.float().requires_grad_(True)
        rctx, rlse = R.attention_ref(q, c.mask, B, S, H, c.p, c.counter, c.site)
        (gr,) = torch.autograd.grad(rctx, q, dctx.float())
        r = ratios(orc, rctx.detach().to(torch.bfloat16), gr.to(torch.bfloat16), H)
        r["lse"] = (rlse.detach().double() - orc["lse"]).abs().max().item()
        print(f"{group} {c.name}: " + " ".join(f"{k}={v:.3f}" if k != "lse" else f"lse={v:.2e}" for k, v in r.items()))
        for k in ("ctx", "dq", "dk", "dv"):
            assert r[k] <= 1.0, (c.name, k, r[k])
        assert r["lse"] < LSE_TOL, (c.name, r["lse"])
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{group} worst: {worst}")


def test_case_table_is_complete():
    """The cases the net is meant to hold (a dropped group or length would otherwise go unnoticed)."""
    cases = AC.all_cases()
    by = {g: [c for c in cases if c.group == g] for g in AC.GROUPS}
    assert sorted({c.S for c in by["lengths"]}) == list(range(64, 513, 64))
    assert sorted({c.S for c in by["masks"]}) == [64, 128, 192, 512]
    assert {(c.S, c.H) for c in by["heads"]} == {(S, H) for S in (128, 192) for H in (1, 3, 12)}
    assert sorted({c.S for c in by["varlen"] if not c.short}) == [128, 192, 320, 512]
    assert any(c.short and c.S == 256 and max(c.lens) <= 128 for c in by["varlen"])
    assert {(c.S, c.varlen) for c in by["q_live"]} == {(S, v) for S in (64, 128) for v in (False, True)}
    assert {(c.S, c.p) for c in by["dropout"]} == {(128, 0.5), (320, 0.5)}
    assert {c.S for c in by["range"]} == {128, 256} and all(c.scale == 3.0 and c.p == 0.0 for c in by["range"])
    for S in (192, 320, 512):
        seen = {v for c in by["varlen"] if c.S == S and not c.short for v in c.lens}
        assert seen == {0, 1, 63, 64, 65, 128, 129, S}
    assert all(c.B <= 4 and (c.H <= 3 or (c.group == "heads" and c.H == 12)) for c in cases)


# ------------------------------------------------------------------ negative controls
def faulty(qkv, mask, B, S, H, p, counter, site, dctx, fault=None, arg=None):
    """The oracle's computation in float64 with one fault, outputs rounded to bf16:
    (ctx [B*S, D], dqkv [B*S, 3D])."""
    D = H * 64
    x = qkv.to(torch.float64).view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2].clone()
    mask = mask.clone()
    scale = 0.125
    if fault == "leak":            # the key just past each prefix is let in
        for b, L in enumerate(arg):
            mask[b, L] = 1
    elif fault in ("lose_last", "skip_tile"):  # the last live key (alone in its key tile) drops out
        for b, L in enumerate(arg):
            mask[b, L - 1] = 0
    elif fault == "scale":
        scale = 0.12
    elif fault == "v_clamp":       # a live key reads the clamped V row len - 1
        for b, L in enumerate(arg):
            v[b, :, L - 2] = v[b, :, L - 1]
    live = mask.view(B, 1, 1, S) != 0
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~live, float("-inf"))
    lse = torch.logsumexp(s, -1, keepdim=True)
    P = torch.exp(s - lse)
    keep = torch.ones_like(P)
    if p > 0:
        keep = keep_mask(counter, site, P.numel(), p).view(P.shape).double() / (1.0 - p)
    if fault == "drop_scale":      # 1 / (1 - p) missing on the 16-key sub-tile 16..31
        keep[..., 16:32] *= (1.0 - p)
    Pd = P * keep
    ctx = Pd @ v
    dO = dctx.to(torch.float64).view(B, S, H, 64).permute(0, 2, 1, 3)
    Pb = P
    if fault == "lse_tile":        # the backward's lse misses key tile 0
        Pb = torch.exp(s - torch.logsumexp(s[..., 64:], -1, keepdim=True))
    delta = (dO * ((P @ v) if fault == "delta_p" else ctx)).sum(-1, keepdim=True)
    dS = Pb * ((dO @ v.transpose(-1, -2)) * keep - delta)
    Pdb = Pb * keep

    def rows(t):
        return t.permute(0, 2, 1, 3).reshape(B * S, D)

    dqkv = torch.cat([rows(dS @ k * scale), rows(dS.transpose(-1, -2) @ q * scale), rows(Pdb.transpose(-1, -2) @ dO)], 1)
    return rows(ctx).to(torch.bfloat16), dqkv.to(torch.bfloat16)


_CTRL_LENS = [100, 77]
CONTROLS = [  # fault, p, mask lens, argument, backward only
    ("leak", 0.1, _CTRL_LENS, _CTRL_LENS, False),
    ("lose_last", 0.1, _CTRL_LENS, _CTRL_LENS, False),
    ("skip_tile", 0.1, [65, 65], [65, 65], False),  # key 64 is the only live key of tile 1
    ("drop_scale", 0.1, _CTRL_LENS, None, False),
    ("scale", 0.0, _CTRL_LENS, None, False),
    ("delta_p", 0.1, _CTRL_LENS, None, True),
    ("v_clamp", 0.0, _CTRL_LENS, _CTRL_LENS, False),
    ("lse_tile", 0.0, _CTRL_LENS, None, True),
]


@pytest.fixture(scope="module")
def control_inputs():
    B, S, H = 2, 128, 2
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(B * S, 3 * H * 64, generator=g).to(torch.bfloat16)
    dctx = torch.randn(B * S, H * 64, generator=g).to(torch.bfloat16)
    return B, S, H, qkv, dctx


@pytest.mark.parametrize("fault,p,lens,arg,bwd_only", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_negative_control_trips_the_bound(control_inputs, fault, p, lens, arg, bwd_only):
    """N(0, 1) inputs at S = 128 -- the flat softmax where a single key weighs least."""
    B, S, H, qkv, dctx = control_inputs
    if fault == "skip_tile":  # the tile's last key is its only live one: keys 0..63 and key 127
        mask = AC.prefix([64, 64], S)
        mask[:, S - 1] = 1
        arg = [S, S]
    else:
        mask = AC.prefix(lens, S)
    orc = R.attention_oracle(qkv, mask, B, S, H, p, 9, 24, dctx)
    # the unfaulted copy passes (so the control measures the fault, not the copy) ...
    ctx, dqkv = faulty(qkv, mask, B, S, H, p, 9, 24, dctx)
    clean = ratios(orc, ctx, dqkv, H)
    assert max(clean.values()) <= 1.0, clean
    # ... and the faulted one does not
    ctx, dqkv = faulty(qkv, mask, B, S, H, p, 9, 24, dctx, fault, arg)
    r = ratios(orc, ctx, dqkv, H)
    print(f"control {fault}: " + " ".join(f"{k}={v:.2f}" for k, v in r.items()) + f"  (clean max {max(clean.values()):.2f})")
    if bwd_only:
        assert r["ctx"] <= 1.0
    assert max(r.values()) > 1.0, r
