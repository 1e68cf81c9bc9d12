"""Numerics of every gfx950 HIP kernel against a plain PyTorch fp32 reference.

Inputs are bf16-rounded once; the reference runs in fp32 on those same values,
so the tolerance only covers bf16 output rounding and accumulation order.
"""
import math

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as kn
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import reference as R
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops.dropout import keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def seed_t(v=7):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("M,N,K", [(256, 768, 768), (320, 2304, 768), (4096, 768, 3072), (192, 128, 64)])
def test_gemm_nt_bias(M, N, K):
    x, w = bf(M, K, seed=1), bf(N, K, scale=0.05, seed=2)
    b = torch.randn(N, device=DEV)
    y = kn.linear_fwd(x, w, b)
    ref = x.float() @ w.float().t() + b
    assert rel_err(y, ref) < 1e-2


def test_gemm_nt_gelu():
    x, w = bf(512, 768, seed=3), bf(3072, 768, scale=0.05, seed=4)
    b = torch.randn(3072, device=DEV) * 0.1
    g, u = kn.linear_fwd(x, w, b, gelu=True)
    uref = x.float() @ w.float().t() + b
    assert rel_err(u, uref) < 1e-2
    assert rel_err(g, torch.nn.functional.gelu(u.float())) < 1e-2
    # a forward without autograd: the activation alone, bitwise the same (u is never written)
    g2, u2 = kn.linear_fwd(x, w, b, gelu=True, keep_u=False)
    assert u2 is None and torch.equal(g2, g)


@pytest.mark.parametrize("M", [4096, 4000])
def test_gemm_nt_gelu_wide_tile(M):
    # N = 3072 at M >= 2048 takes the 8-wave 256x192 tile; M = 4000 leaves a partial row tile.
    x, w = bf(M, 768, seed=21), bf(3072, 768, scale=0.05, seed=22)
    b = torch.randn(3072, device=DEV) * 0.1
    g, u = kn.linear_fwd(x, w, b, gelu=True)
    uref = x.float() @ w.float().t() + b
    assert rel_err(u, uref) < 1e-2
    assert rel_err(g, torch.nn.functional.gelu(u.float())) < 1e-2
    # a forward without autograd: the activation alone, bitwise the same (u is never written)
    g2, u2 = kn.linear_fwd(x, w, b, gelu=True, keep_u=False)
    assert u2 is None and torch.equal(g2, g)


def test_gemm_identity_asymmetric():
    # A = I with an asymmetric B catches a transposed C write (guide §3).
    x = torch.eye(128, dtype=torch.bfloat16, device=DEV)
    w = (torch.arange(128 * 128, device=DEV).view(128, 128) % 97).to(torch.bfloat16)
    y = kn.linear_fwd(x, w, None)
    assert torch.equal(y.float(), w.float().t())


@pytest.mark.parametrize("cfg", [0, 1, 6, 10, 13, 18, 21, 24])
def test_gemm_forced_configs(cfg):
    """Every instantiated NT tile configuration (gemm.hip launch_id) on every fused epilogue of the
    NT path, forced through the config override; odd and even K-tile counts, a partial row tile,
    and fewer K tiles than ring slots."""
    from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops._ext import ext
    N = 2304 if cfg == 6 else 3072 if cfg in (1, 10, 21) else 768
    try:
        ext().gemm_set_cfg(0, cfg, -1)
        for M, K in ((2600, 768), (640, 704), (2688, 3072), (300, 128), (200, 64)):
            x, w = bf(M, K, seed=31), bf(N, K, scale=0.05, seed=32)
            b = torch.randn(N, device=DEV) * 0.1
            ref = x.float() @ w.float().t()
            assert rel_err(kn.linear_fwd(x, w, b), ref + b) < 1e-2
            g, u = kn.linear_fwd(x, w, b, gelu=True)
            assert rel_err(u, ref + b) < 1e-2
            assert rel_err(g, torch.nn.functional.gelu((ref + b).float())) < 2e-2
            res = bf(M, N, seed=33)
            wt = w.t().contiguous()  # dx = x W^T: the NN dX kernel on W^T [K, N]
            assert rel_err(kn.linear_dx(x, wt, res=res), ref + res.float()) < 1e-2
            uu = bf(M, N, seed=34).float().requires_grad_(True)
            gref = torch.autograd.grad(torch.nn.functional.gelu(uu), uu, ref)[0]
            assert rel_err(kn.linear_dx(x, wt, gelu_u=uu.detach().to(torch.bfloat16)), gref) < 1e-2
    finally:
        ext().gemm_set_cfg(0, -1, -1)


@pytest.mark.parametrize("M,N,K", [(256, 768, 768), (4096, 3072, 768), (320, 768, 2304)])
def test_gemm_nn(M, N, K):
    dy, w = bf(M, K, seed=5), bf(K, N, scale=0.05, seed=6)
    dx = kn.linear_dx(dy, w)
    assert rel_err(dx, dy.float() @ w.float()) < 1e-2


@pytest.mark.parametrize("M", [256, 4000])
def test_gemm_nn_gelu_bwd_and_add(M):
    dy, w = bf(M, 768, seed=7), bf(768, 3072, scale=0.05, seed=8)
    u = bf(M, 3072, seed=9)
    x = torch.nn.functional.gelu(u.float()).requires_grad_(False)
    du = kn.linear_dx(dy, w, gelu_u=u)
    uu = u.float().requires_grad_(True)
    g = torch.autograd.grad(torch.nn.functional.gelu(uu), uu, dy.float() @ w.float())[0]
    assert rel_err(du, g) < 1e-2
    res = bf(M, 3072, seed=10)
    dx = kn.linear_dx(dy, w, res=res)
    assert rel_err(dx, dy.float() @ w.float() + res.float()) < 1e-2


@pytest.mark.parametrize("M,N,T", [(768, 768, 4096), (3072, 768, 4096), (768, 3072, 2048), (2304, 768, 512)])
def test_gemm_tn(M, N, T):
    dy, x = bf(T, M, seed=11), bf(T, N, seed=12)
    out = torch.empty(M, N, device=DEV)
    kn.linear_dw(dy, x, out)
    ref = dy.float().t() @ x.float()
    assert rel_err(out, ref) < 2e-3
    kn.linear_dw(dy, x, out, accumulate=True)
    assert rel_err(out, 2 * ref) < 2e-3


@pytest.mark.parametrize("shapes,T", [(((768, 3072), (3072, 768)), 4096),   # lin2 + lin1 (no split)
                                      (((768, 768), (2304, 768)), 4096),    # out_lin + qkv (split-K)
                                      (((768, 768), (2304, 768)), 512)])
def test_gemm_tn_grouped(shapes, T):
    """Two dW GEMMs in one grouped launch == two separate torch fp32 products (plain and accumulate)."""
    (M0, N0), (M1, N1) = shapes
    dy0, x0, dy1, x1 = bf(T, M0, seed=21), bf(T, N0, seed=22), bf(T, M1, seed=23), bf(T, N1, seed=24)
    o0, o1 = torch.empty(M0, N0, device=DEV), torch.empty(M1, N1, device=DEV)
    kn.linear_dw2(dy0, x0, o0, dy1, x1, o1)
    r0, r1 = dy0.float().t() @ x0.float(), dy1.float().t() @ x1.float()
    assert rel_err(o0, r0) < 2e-3 and rel_err(o1, r1) < 2e-3
    kn.linear_dw2(dy0, x0, o0, dy1, x1, o1, accumulate=True)
    assert rel_err(o0, 2 * r0) < 2e-3 and rel_err(o1, 2 * r1) < 2e-3
    single = torch.empty(M1, N1, device=DEV)
    kn.linear_dw(dy1, x1, single)
    assert rel_err(o1, 2 * single) < 1e-5  # same tile math as the single launch


def test_colsum():
    x = bf(4096, 3072, seed=13)
    out = torch.empty(3072, device=DEV)
    kn.colsum(x, out)
    assert rel_err(out, x.float().sum(0)) < 1e-3


def make_mask(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(S // 3, S + 1, (B,), generator=g)
    lens[0] = S
    m = (torch.arange(S)[None, :] < lens[:, None]).long()
    return m.to(DEV)


def test_attention_skips_padded_key_tiles():
    # rows 1 and 2 leave whole 64-key tiles fully masked (skipped by all three kernels)
    B, S, H, p = 3, 256, 12, 0.1
    lens = torch.tensor([256, 70, 130])
    mask = (torch.arange(S)[None, :] < lens[:, None]).long().to(DEV)
    qkv = bf(B * S, 3 * H * 64, seed=31)
    kb = kn.mask_bias(mask)
    ctx, lse = kn.attn_fwd(qkv, kb, B, S, H, seed_t(7), 24, p)
    q = qkv.float().requires_grad_(True)
    rctx, rlse = R.attention_ref(q, mask, B, S, H, p, 7, 24)
    assert rel_err(ctx, rctx) < 2e-2
    assert (lse - rlse).abs().max().item() < 1e-3
    dctx = bf(B * S, H * 64, seed=32)
    dqkv = kn.attn_bwd(qkv, kb, ctx, lse, dctx, B, S, H, seed_t(7), 24, p)
    (g,) = torch.autograd.grad(rctx, q, dctx.float())
    for part in range(3):
        sl = slice(part * H * 64, (part + 1) * H * 64)
        assert rel_err(dqkv[:, sl], g[:, sl]) < 3e-2, part
    # masked keys get exactly zero dK / dV
    dk = dqkv.view(B, S, 3, H * 64)[1, 128:, 1:]
    assert torch.count_nonzero(dk) == 0


@pytest.mark.parametrize("S,varlen", [(128, False), (64, False), (128, True)])
def test_attention_keep_bits_match_hash(S, varlen):
    """The S <= 128 forward records its dropout keep bits; the backward that reads them is
    bitwise the backward that re-hashes every probability (and the forward is unchanged)."""
    B, H, p = 5, 12, 0.1
    g = torch.Generator().manual_seed(S)
    lens = torch.randint(S // 3, S + 1, (B,), generator=g)
    lens[0] = S
    if varlen:
        cu = torch.zeros(B + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(lens, 0)
        rows = (int(cu[-1]) + 127) // 128 * 128
        cu, kb = cu.to(DEV), torch.zeros(1, device=DEV)
    else:
        cu, rows = None, B * S
        kb = kn.mask_bias((torch.arange(S)[None, :] < lens[:, None]).long().to(DEV))
    qkv = bf(rows, 3 * H * 64, seed=41)
    dctx = bf(rows, H * 64, seed=42)
    dm = kn.attn_keep_bits(B, S, H, p, DEV)
    assert dm is not None and kn.attn_keep_bits(B, 256, H, p, DEV) is None and kn.attn_keep_bits(B, S, H, 0.0, DEV) is None
    ctx0, lse0 = kn.attn_fwd(qkv, kb, B, S, H, seed_t(9), 21, p, cu=cu)
    ctx1, lse1 = kn.attn_fwd(qkv, kb, B, S, H, seed_t(9), 21, p, cu=cu, dmask=dm)
    valid = (torch.arange(S)[None, :] < lens[:, None]).to(DEV)[:, None, :].expand(B, H, S)  # (varlen: rows past a
    assert torch.equal(ctx0, ctx1) and torch.equal(lse0[valid], lse1[valid])           # sequence are not written)
    d0 = kn.attn_bwd(qkv, kb, ctx0, lse0, dctx, B, S, H, seed_t(9), 21, p, cu=cu)
    d1 = kn.attn_bwd(qkv, kb, ctx1, lse1, dctx, B, S, H, seed_t(9), 21, p, cu=cu, dmask=dm)
    torch.cuda.synchronize()
    assert torch.equal(d0, d1)


@pytest.mark.parametrize("B,S,p", [(2, 128, 0.0), (3, 128, 0.1), (2, 256, 0.1), (1, 64, 0.0), (2, 512, 0.1),
                                   (1, 512, 0.0)])
def test_attention_fwd(B, S, p):
    H = 12
    qkv = bf(B * S, 3 * H * 64, seed=14)
    mask = make_mask(B, S, 1)
    kb = kn.mask_bias(mask)
    ctx, lse = kn.attn_fwd(qkv, kb, B, S, H, seed_t(3), 16, p)
    rctx, rlse = R.attention_ref(qkv.float(), mask, B, S, H, p, 3, 16)
    assert rel_err(ctx, rctx) < 2e-2
    assert (lse - rlse).abs().max().item() < 1e-3


@pytest.mark.parametrize("B,S,p", [(2, 128, 0.0), (2, 128, 0.1), (1, 256, 0.1), (2, 512, 0.1), (1, 512, 0.0),
                                   (1, 64, 0.0), (2, 64, 0.1)])
def test_attention_bwd(B, S, p):
    H = 12
    qkv = bf(B * S, 3 * H * 64, seed=15)
    mask = make_mask(B, S, 2)
    kb = kn.mask_bias(mask)
    ctx, lse = kn.attn_fwd(qkv, kb, B, S, H, seed_t(5), 20, p)
    dctx = bf(B * S, H * 64, seed=16)
    dqkv = kn.attn_bwd(qkv, kb, ctx, lse, dctx, B, S, H, seed_t(5), 20, p)
    q = qkv.float().requires_grad_(True)
    rctx, _ = R.attention_ref(q, mask, B, S, H, p, 5, 20)
    (g,) = torch.autograd.grad(rctx, q, dctx.float())
    for part in range(3):
        sl = slice(part * H * 64, (part + 1) * H * 64)
        assert rel_err(dqkv[:, sl], g[:, sl]) < 3e-2, part


@pytest.mark.parametrize("p,res", [(0.0, True), (0.1, True)])
def test_layernorm(p, res):
    T, D = 1000, 768
    x, r = bf(T, D, seed=17), bf(T, D, seed=18)
    gamma = torch.randn(D, device=DEV) * 0.2 + 1
    beta = torch.randn(D, device=DEV) * 0.1
    y, mean, rstd = kn.ln_fwd(x, r if res else None, gamma, beta, 1e-12, seed_t(9), 33, p)
    xf, rf = x.float().requires_grad_(True), r.float().requires_grad_(True)
    gf, bf_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = R.add_ln_ref(xf, rf if res else None, gf, bf_, 1e-12, p, 9, 33)
    assert rel_err(y, yr) < 1e-2
    dy = bf(T, D, seed=19)
    dgamma, dbeta, dbias = (torch.empty(D, device=DEV) for _ in range(3))
    dz, dx = kn.ln_bwd(dy, x, r if res else None, gamma, mean, rstd, dgamma, dbeta, dbias, seed_t(9), 33, p)
    gx, gr, gg, gb = torch.autograd.grad(yr, [xf, rf, gf, bf_], dy.float())
    assert rel_err(dx, gx) < 2e-2
    assert rel_err(dz, gr) < 2e-2
    assert rel_err(dgamma, gg) < 1e-2
    assert rel_err(dbeta, gb) < 1e-2
    assert rel_err(dbias, gx.sum(0)) < 1e-2


def test_embedding():
    B, S, V, P, D = 4, 128, 30522, 512, 768
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 300, (B, S), generator=g).to(DEV)
    ids[:, -20:] = 0
    word, pos = bf(V, D, scale=0.02, seed=20), bf(P, D, scale=0.02, seed=21)
    gamma = torch.randn(D, device=DEV) * 0.1 + 1
    beta = torch.randn(D, device=DEV) * 0.1
    p = 0.1
    y, mean, rstd = kn.emb_fwd(ids, word, pos, gamma, beta, S, 1e-12, seed_t(4), 1, p)
    wf, pf = word.float().requires_grad_(True), pos.float().requires_grad_(True)
    gf, bf_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = R.embedding_ref(ids, wf, pf, gf, bf_, 1e-12, p, 4, 1)
    assert rel_err(y, yr) < 1e-2
    dy = bf(B * S, D, seed=22)
    dword = torch.full((V, D), 5.0, device=DEV)
    dpos = torch.full((P, D), 5.0, device=DEV)
    dgamma, dbeta = torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    srt, perm = kn.group_ids(ids)
    rs, rp = torch.sort(ids.reshape(-1), stable=True)
    assert torch.equal(srt, rs) and torch.equal(perm, rp)
    kn.emb_bwd(dy, ids, srt, perm, word, pos, gamma, mean, rstd, dword, dpos, dgamma, dbeta, S, seed_t(4), 1, p)
    gw, gp, gg, gb = torch.autograd.grad(yr, [wf, pf, gf, bf_], dy.float())
    assert rel_err(dword, gw) < 1e-2
    assert rel_err(dpos, gp) < 1e-2
    assert rel_err(dgamma, gg) < 1e-2 and rel_err(dbeta, gb) < 1e-2


def test_head():
    B, S, D = 32, 128, 768
    hidden = bf(B * S, D, seed=23)
    W = torch.randn(2, D, device=DEV) * 0.05
    b = torch.randn(2, device=DEV)
    labels = torch.randint(0, 2, (B,), device=DEV)
    logits, loss, dlog = kn.head_fwd(hidden, B, S, W, b, seed_t(2), 2, 0.3, labels)
    hf = hidden.float().requires_grad_(True)
    Wf, bf_ = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lr = R.head_ref(hf, B, S, Wf, bf_, 0.3, 2, 2)
    assert rel_err(logits, lr) < 1e-4
    lref = torch.nn.functional.cross_entropy(lr, labels)
    assert abs(loss.item() - lref.item()) < 1e-4
    gh, gW, gb = torch.autograd.grad(lref, [hf, Wf, bf_])
    dW, db = torch.empty(2, D, device=DEV), torch.empty(2, device=DEV)
    dh = kn.head_bwd(hidden, B, S, W, seed_t(2), 2, 0.3, dlog, dW, db)
    assert rel_err(dW, gW) < 1e-4 and rel_err(db, gb) < 1e-4
    assert rel_err(dh, gh) < 1e-2


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_emb_fwd_groups_ids_like_rank_sort(dtype):
    """The embedding forward's extra blocks group the ids for the word gradient exactly as the
    standalone rank sort does (same sorted ids, same stable permutation), and the rows' outputs
    do not change."""
    T, S, D = 2688, 128, 768
    g = torch.Generator(device=DEV).manual_seed(41)
    ids = torch.randint(0, 30522, (T,), device=DEV, generator=g)
    ids[::7] = 101  # heavy duplicates (a template word per row)
    ids = ids.to(dtype)
    word = bf(30522, D, seed=42)
    pos = bf(512, D, seed=43)
    gamma, beta = torch.randn(D, device=DEV), torch.randn(D, device=DEV)
    y0, m0, r0 = kn.emb_fwd(ids, word, pos, gamma, beta, S, 1e-12, seed_t(4), 1, 0.1)
    y1, m1, r1, grp = kn.emb_fwd(ids, word, pos, gamma, beta, S, 1e-12, seed_t(4), 1, 0.1, group=True)
    srt, perm = kn.group_ids(ids)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(m0, m1) and torch.equal(r0, r1)
    assert torch.equal(grp[0], srt) and torch.equal(grp[1], perm)
    ref_s, ref_p = torch.sort(ids.long(), stable=True)
    assert torch.equal(grp[0], ref_s) and torch.equal(grp[1], ref_p)


@pytest.mark.parametrize("B", [32, 1500])
def test_head_loss_mean_and_device_accumulator(B):
    """With labels the head forward's mean loss comes from one launch for B <= 1024 (16 waves take
    every row, wave 0 reduces -- head_fwd_mean_kernel) and from head_fwd + head_loss_mean beyond;
    both add it to an optional device running sum (bench.py's graph-replayed loop)."""
    S, D = 1, 768
    hidden = bf(B * S, D, seed=29)
    W = torch.randn(2, D, device=DEV) * 0.05
    b = torch.randn(2, device=DEV)
    labels = torch.randint(0, 2, (B,), device=DEV)
    acc = torch.full((1,), 0.5, device=DEV)
    losses = []
    for _ in range(3):
        logits, loss, _ = kn.head_fwd(hidden, B, S, W, b, seed_t(2), 2, 0.0, labels, loss_acc=acc)
        losses.append(loss.clone())
    torch.cuda.synchronize()
    ref = torch.nn.functional.cross_entropy(hidden.float() @ W.t() + b, labels)
    assert abs(losses[0].item() - ref.item()) < 1e-4
    assert all(torch.equal(losses[0], x) for x in losses)
    assert abs(acc.item() - (0.5 + 3 * losses[0].item())) < 1e-5
    _, loss_plain, _ = kn.head_fwd(hidden, B, S, W, b, seed_t(2), 2, 0.0, labels)
    assert torch.equal(loss_plain, losses[0])


def test_adam_matches_torch():
    n = 4096 + 64
    p0 = torch.randn(n, device=DEV)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    shadow = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for it in range(5):
        g = torch.randn(n, device=DEV)
        ref.grad = g.clone()
        opt.step()
        kn.step_inc(step, None)
        kn.adam(p, g, m, v, shadow, step, 1e-3, 0.9, 0.999, 1e-8, 0.0, False)
    assert (p - ref.detach()).abs().max().item() < 1e-6
    assert torch.equal(shadow, p.to(torch.bfloat16))


def test_eval_metrics():
    logits = torch.randn(37, 2, device=DEV)
    labels = torch.randint(0, 2, (37,), device=DEV)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    counts = torch.zeros(5, dtype=torch.int64, device=DEV)
    prob = torch.empty(37, device=DEV)
    kn.eval_metrics(logits, labels, acc, counts, prob)
    pred = logits.argmax(1)
    assert counts[0].item() == (pred == labels).sum().item()
    assert counts[1].item() == ((pred == 1) & (labels == 1)).sum().item()
    assert abs(acc.item() - torch.nn.functional.cross_entropy(logits, labels).item()) < 1e-5
    assert rel_err(prob, torch.softmax(logits, 1)[:, 1]) < 1e-5


def test_dropout_hash_matches_kernel():
    # LN kernel with x = 1, r = None and gamma=1,beta=0 is not directly a mask probe;
    # use the head-free path: ln_fwd output on constant rows equals (mask-pattern LN).
    T, D = 8, 768
    x = torch.ones(T, D, dtype=torch.bfloat16, device=DEV)
    gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    y, _, _ = kn.ln_fwd(x, None, gamma, beta, 1e-12, seed_t(11), 5, 0.5)
    keep = keep_mask(11, 5, T * D, 0.5, device=DEV).view(T, D)
    # kept elements share one value per row, dropped another
    for t in range(T):
        kept = y[t][keep[t]].float()
        assert kept.numel() > 0 and (kept - kept[0]).abs().max().item() == 0


def test_sparse_word_grad_and_adam_skip():
    """Flagged (sparse) word-embedding grad + Adam row skipping == dense path."""
    B, S, V, P, D = 2, 64, 30522, 512, 768
    ids = torch.randint(5, 50, (B, S)).to(DEV)
    word, pos = bf(V, D, scale=0.02, seed=30), bf(P, D, scale=0.02, seed=31)
    gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    y, mean, rstd = kn.emb_fwd(ids, word, pos, gamma, beta, S, 1e-12, seed_t(1), 1, 0.1)
    dy = bf(B * S, D, seed=32)
    srt, perm = torch.sort(ids.reshape(-1))
    dense = torch.full((V, D), 3.0, device=DEV)
    sparse = torch.full((V, D), 7.0, device=DEV)  # stale garbage outside the batch rows
    dpos, dg, db = torch.empty(P, D, device=DEV), torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    kn.emb_bwd(dy, ids, srt, perm, word, pos, gamma, mean, rstd, dense, dpos, dg, db, S, seed_t(1), 1, 0.1)
    now = torch.zeros(V, dtype=torch.uint8, device=DEV)
    ever = torch.zeros(V, dtype=torch.uint8, device=DEV)
    kn.emb_bwd(dy, ids, srt, perm, word, pos, gamma, mean, rstd, sparse, dpos, dg, db, S, seed_t(1), 1, 0.1,
               False, now, ever)
    rows = torch.unique(ids)
    assert now.sum().item() == rows.numel() and ever.sum().item() == rows.numel()
    assert torch.equal(sparse[rows], dense[rows])
    # Adam: full arena = [pad 64 | word table], skip rows by flags
    n = 64 + V * D
    p0 = torch.randn(n, device=DEV)
    gd = torch.zeros(n, device=DEV)
    gd[64:] = dense.view(-1)
    gs = torch.zeros(n, device=DEV)
    gs[64:] = sparse.view(-1)
    pd_, ps_ = p0.clone(), p0.clone()
    md, vd, ms, vs = (torch.zeros(n, device=DEV) for _ in range(4))
    st1, st2 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    kn.step_inc(st1)
    kn.step_inc(st2)
    kn.adam(pd_, gd, md, vd, None, st1, 1e-3, 0.9, 0.999, 1e-8, 0.0, False)
    kn.adam(ps_, gs, ms, vs, None, st2, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, ever, now, 64, V, D)
    assert torch.equal(pd_, ps_) and torch.equal(md, ms) and torch.equal(vd, vs)


@pytest.mark.parametrize("T", [4096, 1000, 37])
def test_rank_sort_matches_stable_sort(T):
    g = torch.Generator().manual_seed(T)
    ids = torch.randint(0, 300, (T,), generator=g).to(DEV)
    ids[: T // 4] = 0  # a long run (padding id)
    srt, perm = kn.group_ids(ids)
    ref_s, ref_p = torch.sort(ids, stable=True)
    assert torch.equal(srt, ref_s) and torch.equal(perm, ref_p)


@pytest.mark.parametrize("M,N,K,epi", [(2688, 3072, 768, 3), (2700, 768, 3072, 4), (300, 3072, 768, 3)])
def test_gemm_epilogue_column_sums(M, N, K, epi):
    """NN dX GEMM (dx = dy W, W read MN-major) with GELU' / residual epilogue + per-tile column
    sums of its bf16 output."""
    dy, w = bf(M, K, seed=31), bf(K, N, seed=32)
    aux = bf(M, N, seed=33)
    ref_dx = kn.linear_dx(dy, w, gelu_u=aux if epi == 3 else None, res=aux if epi == 4 else None)
    dx = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    tiles = (M + 127) // 128
    part = torch.full((tiles * N,), float("nan"), device=DEV)
    nblk = kn.ext().gemm_colsum(epi, dy, w, dx, aux if epi == 3 else None, aux if epi == 4 else None, part, None, 1)
    torch.cuda.synchronize()
    assert nblk == tiles
    assert torch.equal(dx, ref_dx)
    col = part.view(tiles, N).sum(0)
    ref = dx.float().sum(0)
    assert rel_err(col, ref) < 1e-5


def test_head_bwd_packed_rows_and_zeroing():
    """Packed layout ([CLS] = first row of each sequence, one empty sequence): the [CLS] rows
    carry the gradient, every other row of dhidden is exactly 0 (written by the kernel)."""
    lens = torch.tensor([5, 0, 7, 1, 3] + [4] * 27)
    B, D = len(lens), 768
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    T = int(cu[-1]) + 11  # + filler rows
    hidden = bf(T, D, seed=24)
    W = torch.randn(2, D, device=DEV) * 0.05
    b = torch.randn(2, device=DEV)
    labels = torch.randint(0, 2, (B,), device=DEV)
    cls = cu[:-1].to(DEV)
    logits, loss, dlog = kn.head_fwd(hidden, B, 1, W, b, seed_t(2), 2, 0.0, labels, cls)
    junk = torch.full((T, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    del junk  # the caching allocator hands this block to dhidden: stale NaNs unless zeroed
    dW, db = torch.empty(2, D, device=DEV), torch.empty(2, device=DEV)
    dh = kn.head_bwd(hidden, B, 1, W, seed_t(2), 2, 0.0, dlog, dW, db, cls=cls)
    torch.cuda.synchronize()
    rows = torch.clamp(cls.long(), max=T - 1)
    want = torch.zeros(T, D, device=DEV)
    for i in range(B):  # a repeated row (empty sequence) takes the later sequence's value
        want[rows[i]] = dlog[i, 0] * W[0] + dlog[i, 1] * W[1]
    assert rel_err(dh, want) < 1e-2
    other = torch.ones(T, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert (dh[other] == 0).all()
    x = hidden.float()[rows]
    assert rel_err(dW, dlog.t() @ x) < 1e-4


@pytest.mark.parametrize("M,N,K", [(2688, 3072, 768), (4000, 3072, 768), (256, 3072, 768)])
def test_gelu_bwd_rematerialises_activation(M, N, K):
    # The GELU' dX epilogue's aux_out re-creates the forward activation gelu(u) bitwise
    # (forward: EPI_BIAS_GELU on x W1^T + b), on both dX paths: NN, NN + fused column sums.
    x, w1, b1 = bf(M, K, seed=60), bf(N, K, scale=0.05, seed=61), bf(N, seed=62).float()
    g, u = kn.linear_fwd(x, w1, b1, gelu=True)
    dy, w2 = bf(M, 768, seed=63), bf(768, N, scale=0.05, seed=64)
    base = kn.linear_dx(dy, w2, gelu_u=u)
    out = torch.full_like(u, float("nan"))
    du = kn.linear_dx(dy, w2, gelu_u=u, aux_out=out)
    assert torch.equal(out, g) and torch.equal(du, base)
    jobs = []
    bgrad = torch.zeros(N, device=DEV)
    out = torch.full_like(u, float("nan"))
    du = kn.linear_dx(dy, w2, gelu_u=u, colsum=(jobs, bgrad, False), aux_out=out)
    assert torch.equal(out, g) and torch.equal(du, base)
