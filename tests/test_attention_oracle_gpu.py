"""The attention HIP kernels against the float64 oracle, elementwise, at every admitted shape.

Every case runs ``attn_fwd`` and ``attn_bwd`` on bf16 inputs and demands
|kernel - oracle| <= 2.5 u E + 1e-30 per element (ops/reference.py attention_oracle /
attention_bound_ratio: u = 2^-8, E the absolute-weighted sum behind the element; where E is
exactly 0 -- dK / dV of a masked key -- the kernel must return exactly 0) and |lse - oracle| < 1e-3.
The cases (tests/attn_cases.py; tests/test_attention_oracle_cpu.py shows that a correct fp32
implementation passes the same assertion on them and that typical kernel faults do not):

  lengths  every S = 64 .. 512 with lens [S, 1, S - 63] (odd tile counts, one live key in the last tile)
  masks    a dead first key tile, alternating 16-key blocks, a single last key, a 32-key hole
  heads    H = 1, 3, 12 (strides, grid, lse / delta / dropout indices)
  range    inputs x 3 and a planted key > 20 ahead, in the first and in the last key tile
  varlen   packed rows with empty sequences and filler rows; length split off and on; short=True
  q_live   the pruned block's [CLS]-row form, both layouts
  dropout  p = 0.5

At S <= 128 (or short=True) with dropout every case runs with and without the keep-bits buffer.
"""
import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as kn
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import reference as R
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops.dropout import threshold

import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda"
LSE_TOL = 1e-3
CASES = AC.all_cases()


def seed_t(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _keep_bits_variants(c):
    s128 = c.S <= 128 or c.short
    return (False, True) if s128 and c.p > 0 else (False,)


def _check(c, tag, orc, ctx, lse, dqkv, ctx_rows, lse_valid):
    """Print every figure, then assert.  ctx_rows: the rows of ctx that are compared (None: all);
    lse_valid: bool [B, H, S] of the lse entries that are."""
    D = c.H * 64
    sel = slice(None) if ctx_rows is None else ctx_rows
    r = {"ctx": R.attention_bound_ratio(ctx[sel], orc["ctx"][sel], orc["A"][sel])}
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * D, (i + 1) * D)
        r[name] = R.attention_bound_ratio(dqkv[:, sl], orc["dqkv"][:, sl], orc["E"][:, sl])
    r["lse"] = (lse.double() - orc["lse"])[lse_valid].abs().max().item()
    print(f"ORACLE group={c.group} case={c.name} run={tag} " + " ".join(f"{k}={v:.4g}" for k, v in r.items()))
    for name in ("ctx", "dq", "dk", "dv"):
        assert r[name] <= 1.0, (c.group, c.name, tag, name, r[name])
    assert r["lse"] < LSE_TOL, (c.group, c.name, tag, r["lse"])


def _run_padded(c):
    B, S, H = c.B, c.S, c.H
    qkv, dctx = (t.to(DEV) for t in c.inputs())
    mask = c.mask.to(DEV)
    kb = kn.mask_bias(mask)
    orc = R.attention_oracle(qkv, mask, B, S, H, c.p, c.counter, c.site, dctx)
    rows, valid = None, torch.ones(B, H, S, dtype=torch.bool, device=DEV)
    if c.q_live:
        rows = (torch.arange(B, device=DEV)[:, None] * S + torch.arange(c.q_live, device=DEV)[None, :]).reshape(-1)
        valid[:, :, c.q_live:] = False
    for bits in _keep_bits_variants(c):
        dm = kn.attn_keep_bits(B, S, H, c.p, DEV) if bits else None
        assert (dm is not None) == bits
        ctx, lse = kn.attn_fwd(qkv, kb, B, S, H, seed_t(c.counter), c.site, c.p, dmask=dm, q_live=c.q_live)
        dqkv = kn.attn_bwd(qkv, kb, ctx, lse, dctx, B, S, H, seed_t(c.counter), c.site, c.p, dmask=dm, q_live=c.q_live)
        torch.cuda.synchronize()
        _check(c, f"bits{int(bits)}", orc, ctx, lse, dqkv, rows, valid)


def _run_varlen(c):
    B, S, H, D = c.B, c.S, c.H, c.H * 64
    qkv_pad, dctx_pad = (t.to(DEV) for t in c.inputs())
    mask = c.mask.to(DEV)
    lens = torch.tensor(c.lens)
    assert lens[0] == 0 and (c.q_live or lens[-1] == 0)  # a leading and a trailing empty sequence
    idx = c.packed_rows().to(DEV)
    n = idx.numel()
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    cu = cu.to(DEV)
    qkv = torch.cat([qkv_pad[idx], torch.zeros(AC.FILLER, 3 * D, dtype=torch.bfloat16, device=DEV)])
    dctx = torch.cat([dctx_pad[idx], torch.zeros(AC.FILLER, D, dtype=torch.bfloat16, device=DEV)])
    kb = kn.mask_bias(torch.ones(B, S, dtype=torch.int64, device=DEV))  # (varlen: not read)
    full = R.attention_oracle(qkv_pad, mask, B, S, H, c.p, c.counter, c.site, dctx_pad)
    # the padded oracle gathered to the packed rows; lse keeps its [B, H, S] layout
    orc = {"ctx": full["ctx"][idx], "A": full["A"][idx], "dqkv": full["dqkv"][idx], "E": full["E"][idx], "lse": full["lse"]}
    qn = c.q_live if c.q_live else S
    valid = (torch.arange(S)[None, :] < torch.clamp(lens, max=qn)[:, None]).to(DEV)[:, None, :].expand(B, H, S)
    rows = None
    if c.q_live:
        live = lens > 0
        rows = (cu[:-1].long()[live.to(DEV)][:, None] + torch.arange(c.q_live, device=DEV)[None, :]).reshape(-1)
    empty = (lens == 0).to(DEV)
    splits = (0, 1) if S > 128 and not c.short else (None,)
    prev = kn.ext().attn_set_split(1)
    try:
        for split in splits:
            if split is not None:
                kn.ext().attn_set_split(split)
            for bits in _keep_bits_variants(c):
                dm = kn.attn_keep_bits(B, S, H, c.p, DEV, short=c.short) if bits else None
                assert (dm is not None) == bits
                ctx, lse = kn.attn_fwd(qkv, kb, B, S, H, seed_t(c.counter), c.site, c.p, cu=cu, dmask=dm,
                                       q_live=c.q_live, short=c.short)
                dqkv = kn.attn_bwd(qkv, kb, ctx, lse, dctx, B, S, H, seed_t(c.counter), c.site, c.p, cu=cu, dmask=dm,
                                   q_live=c.q_live, short=c.short)
                torch.cuda.synchronize()
                tag = f"split{split}-bits{int(bits)}"
                assert not ctx[n:].any() and not dqkv[n:].any(), (c.name, tag, "filler rows")
                _check(c, tag, orc, ctx[:n], lse, dqkv[:n], rows, valid)
            # an empty sequence owns nothing: its lse rows stay as the caller left them
            lse_s = torch.full((B, H, S), 12345.0, device=DEV)
            ctx_s = torch.empty(n + AC.FILLER, D, dtype=torch.bfloat16, device=DEV)
            thr = threshold(c.p)
            sc = 1.0 / (1.0 - c.p) if thr else 1.0
            kn.ext().attn_fwd(qkv, kb, ctx_s, lse_s, B, S, H, seed_t(c.counter), c.site, thr, sc, cu, None, c.q_live,
                              split=2 if c.short else -1)
            torch.cuda.synchronize()
            assert (lse_s[empty] == 12345.0).all(), (c.name, split, "lse of an empty sequence written")
    finally:
        kn.ext().attn_set_split(prev)


@pytest.mark.parametrize("c", CASES, ids=[f"{c.group}-{c.name}" for c in CASES])
def test_attention_against_oracle(c):
    if c.varlen:
        _run_varlen(c)
    else:
        _run_padded(c)


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int32, torch.int64])
def test_mask_bias_every_dtype(dtype):
    """``mask != 0`` at the mask's own width (values whose low byte or low word is 0 included), at a
    size that is no multiple of the 256-thread block."""
    B, S = 5, 67
    assert (B * S) % 256 != 0
    g = torch.Generator().manual_seed(3)
    m = torch.randint(0, 2, (B, S), generator=g)
    if dtype == torch.bool:
        mask = m.bool()
    else:
        odd = {torch.uint8: [2, 255, 128], torch.int32: [256, -1, 1 << 16, -(1 << 31)],
               torch.int64: [256, -1, 1 << 32, 1 << 40, -(1 << 63)]}[dtype]
        mask = m.to(dtype)
        live = torch.nonzero(m.reshape(-1)).squeeze(1)
        for i, v in enumerate(odd):
            mask.view(-1)[live[3 * i + 1]] = v
    mask = mask.to(DEV)
    want = torch.where(mask != 0, torch.zeros((), device=DEV), torch.full((), float("-inf"), device=DEV))
    got = kn.mask_bias(mask)
    assert got.dtype == torch.float32 and got.shape == mask.shape
    assert torch.equal(got, want)
    assert (want == 0).any() and (want != 0).any()
