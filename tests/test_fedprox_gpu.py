"""FedProx on the GPU: the proximal term ``mu * (p - anchor)`` inside every launch that applies Adam
-- the run-table and row-flag launches, the fused weight-gradient epilogues, the qkv-bias column
update and the rest blocks of the all-layer dW launch -- and the anchor's re-snapshot under captured
graphs.

Everything is compared bit for bit against the plain launches with the same term (one launch per
run, the dense table update, gradient-then-Adam, the unfused step), and the run table against fp32
torch (``p.grad += mu * (p - anchor)``, then torch.optim)."""
import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier, DistilBertConfig)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2, EPS, WD, MU = 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.05
HF_NO_DECAY = ("bias", "LayerNorm", "layer_norm")


@pytest.fixture
def nosplit():
    """Weight-gradient GEMMs unsplit in every arm (as tests/test_fused_adam_gpu.py)."""
    K.ext().gemm_set_cfg(2, -1, 1)
    yield
    K.ext().gemm_set_cfg(2, -1, -1)


def _state(p0):
    n = p0.numel()
    return [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(torch.bfloat16)]


# ---------------------------------------------------------------- run table
@pytest.mark.parametrize("decoupled", [False, True])
def test_run_table_prox(decoupled):
    """One run-table launch with a proximal term (and a decay per run) == one launch per run with
    that run's slice of the anchor, bitwise (p, m, v, shadow; 3 steps); within 1e-6 of fp32 torch
    Adam / AdamW fed ``g + mu * (p - anchor)`` (the bound of tests/test_adamw_gpu.py's run-table
    test); elements outside the runs untouched; mu = 0 with an anchor == no anchor, bitwise."""
    runs = [(0, 64), (128, 8), (256, 260), (1024, 1024)]
    decays = [0.01, 0.0, 0.01, 0.0]
    n = 2048 + 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    p0 = torch.randn(n, device=DEV, generator=gen)
    anc = p0 + 0.05 * torch.randn(n, device=DEV, generator=gen)  # (a client some steps into its round)
    a, b, z, nz = _state(p0), _state(p0), _state(p0), _state(p0)
    refs = [p0[o:o + ln].clone().requires_grad_(True) for o, ln in runs]
    groups = [{"params": [r], "weight_decay": wd} for r, wd in zip(refs, decays)]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=LR, betas=(B1, B2), eps=EPS)
    table, rdec = K.adam_runs(runs, DEV), K.adam_run_decay(decays, DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(3):
        g = torch.randn(n, device=DEV, generator=gen)
        K.step_inc(step, None)
        K.adam(a[0], g, a[1], a[2], a[3], step, LR, B1, B2, EPS, 0.5, decoupled, runs=table, run_decay=rdec,
               prox=(MU, anc))
        for (o, ln), wd in zip(runs, decays):
            sl = slice(o, o + ln)
            K.adam(b[0][sl], g[sl], b[1][sl], b[2][sl], b[3][sl], step, LR, B1, B2, EPS, wd, decoupled,
                   prox=(MU, anc[sl]))
        K.adam(z[0], g, z[1], z[2], z[3], step, LR, B1, B2, EPS, 0.5, decoupled, runs=table, run_decay=rdec,
               prox=(0.0, anc))
        K.adam(nz[0], g, nz[1], nz[2], nz[3], step, LR, B1, B2, EPS, 0.5, decoupled, runs=table, run_decay=rdec)
        for r, (o, ln) in zip(refs, runs):
            with torch.no_grad():
                r.grad = g[o:o + ln] + MU * (r.detach() - anc[o:o + ln])
        opt.step()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(z, nz):
        assert torch.equal(x, y)
    untouched = torch.ones(n, dtype=torch.bool, device=DEV)
    for (o, ln), r in zip(runs, refs):
        untouched[o:o + ln] = False
        err = (a[0][o:o + ln] - r.detach()).abs().max().item()
        print(f"decoupled={decoupled} run ({o}, {ln}): max |hip - torch| = {err:.3e}")
        assert err <= 1e-6
        assert not torch.equal(a[0][o:o + ln], nz[0][o:o + ln])  # the term changes the result
    assert torch.equal(a[0][untouched], p0[untouched]) and not a[1][untouched].any() and not a[2][untouched].any()
    assert torch.equal(a[3][untouched], p0.to(torch.bfloat16)[untouched])


# ---------------------------------------------------------------- row flags
PAD, TAIL = 64, 256
SCHEDULE = {1: [3, 4, 17, 17], 3: [5, 249], 5: [3, 100]}


@pytest.mark.parametrize("rl", [768, 64])
def test_row_flags_prox_matches_dense_table(rl):
    """A [250][rl] table behind a 64-float pad, followed by a 256-float dense run; rows first touched
    at steps 1 (with a duplicate id), 3 and 5 of 6; the anchor is the starting point, as after
    reset_state().  Sparse arm: adam_rows + the run table for the rest; flag arm: one flat launch
    that skips rows without state; dense arm: one flat launch over everything.  Same mu: the three
    are bitwise equal after every step, and the rows never touched still equal their anchor."""
    rows = 250
    n = PAD + rows * rl + TAIL
    gen = torch.Generator(device=DEV).manual_seed(11)
    p0 = torch.randn(n, device=DEV, generator=gen)
    anc = p0.clone()
    t0, t1 = PAD, PAD + rows * rl
    tab = slice(t0, t1)
    dense, sparse, flag, plain = _state(p0), _state(p0), _state(p0), _state(p0)
    ever = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    rest = K.adam_runs([(0, PAD), (t1, TAIL)], DEV)
    for t in range(1, 7):
        ids = SCHEDULE.get(t, [])
        g = torch.randn(n, device=DEV, generator=gen)
        now = torch.zeros(rows, dtype=torch.uint8, device=DEV)
        if ids:
            now[torch.tensor(sorted(set(ids)), device=DEV)] = 1
        ever |= now
        gd = g.clone()
        gd[tab] = (g[tab].view(rows, rl) * now[:, None].float()).reshape(-1)
        K.step_inc(step, None)
        K.adam(dense[0], gd, dense[1], dense[2], dense[3], step, LR, B1, B2, EPS, 0.0, False, prox=(MU, anc))
        K.adam(plain[0], gd, plain[1], plain[2], plain[3], step, LR, B1, B2, EPS, 0.0, False)
        K.adam_rows(sparse[0][tab], g[tab], sparse[1][tab], sparse[2][tab], sparse[3][tab], step, LR, B1, B2, EPS,
                    ever, now, rl, prox=(MU, anc[tab]))
        K.adam(sparse[0], g, sparse[1], sparse[2], sparse[3], step, LR, B1, B2, EPS, 0.0, False, runs=rest,
               prox=(MU, anc))
        K.adam(flag[0], g, flag[1], flag[2], flag[3], step, LR, B1, B2, EPS, 0.0, False, ever, now, PAD, rows, rl,
               prox=(MU, anc))
        torch.cuda.synchronize()
        for x, y, w in zip(sparse, dense, flag):
            assert torch.equal(x, y), t
            assert torch.equal(w, y), t
    never = ever == 0
    assert int(never.sum()) == rows - 6
    for arm in (dense, sparse):
        assert torch.equal(arm[0][tab].view(rows, rl)[never], anc[tab].view(rows, rl)[never])
    # the rows with state and the dense run did feel the term
    assert not torch.equal(dense[0][tab].view(rows, rl)[~never], plain[0][tab].view(rows, rl)[~never])
    assert not torch.equal(dense[0][t1:], plain[0][t1:])


# ---------------------------------------------------------------- fused epilogue
def test_dw_batch_fused_prox_matches_gradient_then_adam():
    """The all-layer dW launch with Adam and a proximal term in its epilogues == the same launch
    storing fp32 gradients + the flat Adam kernel with the same term, bitwise.  The shapes of
    tests/test_fused_adam_gpu.py::test_dw_fused_adam_matches_gradient_then_adam at T = 2688, and a
    768 x 768 problem of K = 64 rows: one K step (the pruned last block's case).  Decoupled decay, so
    the term is seen to come from the parameter as loaded."""
    shapes = [(768, 3072, 2688), (3072, 768, 2688), (768, 768, 64)]
    g = torch.Generator(device=DEV).manual_seed(5)

    def bf(*s):
        return (torch.randn(*s, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    dys, xs = [bf(T, M) for M, N, T in shapes], [bf(T, N) for M, N, T in shapes]
    sizes = [M * N for M, N, T in shapes]
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    n = sum(sizes)
    p0 = torch.randn(n, device=DEV, generator=g)
    anc = p0 + 0.05 * torch.randn(n, device=DEV, generator=g)
    m0, v0 = torch.rand(n, device=DEV, generator=g) * 1e-3, torch.rand(n, device=DEV, generator=g) * 1e-6
    arms = [[p0.clone(), m0.clone(), v0.clone(), p0.to(torch.bfloat16)] for _ in range(3)]
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    hp = [LR, B1, B2, EPS, WD, 1.0]

    def views(buf):
        return [buf[o:o + s].view(M, N) for o, s, (M, N, T) in zip(offs, sizes, shapes)]

    # reference: gradients (the same launch, storing them), then the flat Adam kernel
    grad = torch.empty(n, device=DEV)
    K.linear_dw_batch([(dy, x, out, False) for dy, x, out in zip(dys, xs, views(grad))])
    p, m_, v_, sh = arms[1]
    K.adam(p, grad, m_, v_, sh, step, LR, B1, B2, EPS, WD, True, prox=(MU, anc))
    p, m_, v_, sh = arms[2]
    K.adam(p, grad, m_, v_, sh, step, LR, B1, B2, EPS, WD, True)  # (no term: must differ)
    # fused
    p, m_, v_, sh = arms[0]
    st = []
    for o, s in zip(offs, sizes):
        st += [p[o:o + s], m_[o:o + s], v_[o:o + s], sh[o:o + s]]
    st.append(step)
    junk = torch.full((n,), 7.0, device=DEV)
    K.linear_dw_batch([(dy, x, out, False) for dy, x, out in zip(dys, xs, views(junk))], adam=lambda outs: (st, hp),
                      prox=(MU, [anc[o:o + s] for o, s in zip(offs, sizes)]))
    torch.cuda.synchronize()
    assert (junk == 7.0).all()  # the gradient itself is never stored
    for x, y in zip(arms[0], arms[1]):
        assert torch.equal(x, y)
    for o, s in zip(offs, sizes):
        assert not torch.equal(arms[0][0][o:o + s], arms[2][0][o:o + s])
    # mu = 0 with anchors passed == the launch without them
    za, zb = [t.clone() for t in arms[2]], [t.clone() for t in arms[2]]
    for arm, kw in ((za, dict(prox=(0.0, [anc[o:o + s] for o, s in zip(offs, sizes)]))), (zb, {})):
        p, m_, v_, sh = arm
        st = []
        for o, s in zip(offs, sizes):
            st += [p[o:o + s], m_[o:o + s], v_[o:o + s], sh[o:o + s]]
        st.append(step)
        K.linear_dw_batch([(dy, x, out, False) for dy, x, out in zip(dys, xs, views(junk))],
                          adam=lambda outs, st=st: (st, hp), **kw)
    torch.cuda.synchronize()
    for x, y in zip(za, zb):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- model level
def _batch(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(S // 3, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = ids * mask
    ids[:, 0] = 101
    labels = torch.randint(0, 2, (B,), generator=g)
    return ids.cuda(), mask.cuda(), labels.cuda(), int(lens.sum())


def _train(fuse, graph, mu=MU, steps=5, reset_after=None, seeds=None, **kw):
    """``steps`` steps of a 2-layer model on bs16 x seq128 batches (batch ``it`` from seed
    ``seeds[it]``, default 300 + it; ``reset_after``: reset_state() before that step) -> (losses,
    master, m, v, shadow, model, optimizer, step function)."""
    m = DDoSClassifier(config=DistilBertConfig(n_layers=2), device=DEV, impl="hip", seed=13)
    m.train()
    opt = ArenaAdam(m, lr=LR, fuse_dw=fuse, prox_mu=mu, **kw)
    assert opt.can_fuse() == fuse
    st = GraphedTrainStep(make_step_fn(m, opt), warmup=1, enabled=graph, bucket=m.packed_rows)
    losses = []
    for it in range(steps):
        if reset_after is not None and it == reset_after:
            opt.reset_state()
            st.graphs_at_reset = len(st.graphs)
        ids, mask, labels, tokens = _batch(16, 128, seed=300 + it if seeds is None else seeds[it])
        losses.append(float(st(ids, mask, labels, tokens)))
    torch.cuda.synchronize()
    A = m.arena
    return losses, A.master.clone(), opt.m.clone(), opt.v.clone(), A.shadow.clone(), m, opt, st


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for x, y in zip(a[1:5], b[1:5]):
        assert torch.equal(x, y)


_REF = {}


def _unfused_ref():
    """The unfused eager arm (row-flag Adam + run-table launch after the backward), computed once."""
    if "ref" not in _REF:
        _REF["ref"] = _train(False, False)[:5]
    return _REF["ref"]


@pytest.mark.parametrize("graph", [False, True])
def test_prox_fused_training_matches_unfused(graph, nosplit):
    """fuse_dw=True (Adam in the dW epilogues, the qkv bias by the tiles that sum it, the rest of the
    step -- run table and flagged word rows -- by the launch's rest blocks) against fuse_dw=False:
    losses, master, m, v and shadow bitwise, eager and through captured graphs; the term is felt."""
    fused = _train(True, graph)
    _same(fused, _unfused_ref())
    if graph:
        _same(_train(False, True), _unfused_ref())
        assert fused[7].graph is not None and fused[7].failed is None
    else:
        plain = _train(True, False, mu=0.0)
        assert not torch.equal(plain[1], fused[1])
        assert plain[6].anchor is None and fused[6].anchor is not None
        # the word rows the batches never touched still equal their anchor
        m, opt = fused[5], fused[6]
        woff, rows, rl = m.word_embedding_span()
        never = m.emb_ever == 0
        assert 0 < int((~never).sum()) < rows
        assert torch.equal(fused[1][woff:woff + rows * rl].view(rows, rl)[never],
                           opt.anchor[woff:woff + rows * rl].view(rows, rl)[never])


def test_prox_fused_training_rest_outside_the_dw_launch(nosplit, monkeypatch):
    """FD_ADAM_IN_DW=0: the fused epilogues, then step()'s own row-flag and run-table launches."""
    monkeypatch.setattr(K, "ADAM_IN_DW", False)
    _same(_train(True, False), _unfused_ref())


def test_prox_fused_training_mixed_tile_schedule(nosplit):
    """The mixed tile schedule forced (256 x 128 half tiles for one problem): the same bits."""
    old = K.ext().gemm_dwb_set_mix(2)
    try:
        before = K.ext().gemm_dwb_mixed_launches()
        fused = _train(True, False)
        assert K.ext().gemm_dwb_mixed_launches() > before
    finally:
        K.ext().gemm_dwb_set_mix(old)
    _same(fused, _unfused_ref())


def test_prox_with_decaying_word_table_trains_dense(nosplit):
    """AdamW 0.01 with the HF no-decay group -- the word table decays -- and a proximal term: both
    arms take the dense word path, and fused == unfused bitwise."""
    kw = dict(weight_decay=WD, decoupled=True, no_decay=HF_NO_DECAY)
    fused, unfused = _train(True, False, **kw), _train(False, False, **kw)
    for arm in (fused, unfused):
        assert arm[5].sparse_word_grad is False and not arm[6].lazy_active() and arm[6].word_wd == WD
    _same(fused, unfused)
    assert not torch.equal(fused[1], _unfused_ref()[1])


def test_schedule_prox_and_parameter_groups_in_one_step(nosplit):
    """A linear schedule (2 warmup steps of 8), a proximal term and AdamW parameter groups in the
    same 5 steps -- the three travel in one hyper-parameter descriptor (csrc/kernels/adam_epi.h
    FdAdamHyper).  The word table is in the no-decay group, so the sparse word path and the rest of
    the step stay inside the dW launch.  Fused eager, fused graphed and unfused eager agree bitwise
    (losses, master, m, v, shadow; _train asserts can_fuse() for the fused arms), and the result
    is not that of the same run with prox_mu = 0."""
    kw = dict(schedule="linear", warmup_steps=2, total_steps=8, weight_decay=WD, decoupled=True,
              no_decay=HF_NO_DECAY + ("word_embeddings",))
    unfused, fused, graphed = _train(False, False, **kw), _train(True, False, **kw), _train(True, True, **kw)
    for arm in (fused, graphed):
        assert arm[6].can_fuse() and arm[6].word_wd == 0.0 and arm[6].grouped_decay
        assert arm[5].sparse_word_grad and arm[6].sched_args() == (1, 2, 8, 0)
    assert graphed[7].graph is not None and graphed[7].failed is None
    _same(fused, unfused)
    _same(graphed, unfused)
    plain = _train(True, False, mu=0.0, **kw)
    assert not torch.equal(plain[1], fused[1])


def test_prox_anchor_resnapshot_is_what_graph_replays_read(nosplit):
    """Capture, train 3 steps, reset_state(), train 3 more through the same captured graphs (two
    batches in turn, so every step after the reset finds its graph: no new capture): bitwise the
    eager arm.  The anchor keeps its address and holds the weights of the reset; with the anchor of
    the first half left in place the second half is another run."""
    seeds = [300, 301, 300, 301, 300, 301]
    eager = _train(True, False, steps=6, reset_after=3, seeds=seeds)
    graphed = _train(True, True, steps=6, reset_after=3, seeds=seeds)
    _same(graphed, eager)
    st, opt = graphed[7], graphed[6]
    assert st.graph is not None and st.failed is None
    assert 1 <= st.graphs_at_reset == len(st.graphs)  # steps 4-6 were replays
    init = DDoSClassifier(config=DistilBertConfig(n_layers=2), device=DEV, impl="hip", seed=13).arena.master
    assert not torch.equal(opt.anchor, init) and torch.equal(opt.anchor, eager[6].anchor)
    m = DDoSClassifier(config=DistilBertConfig(n_layers=2), device=DEV, impl="hip", seed=13)
    m.train()
    opt2 = ArenaAdam(m, lr=LR, prox_mu=MU)
    ptr = opt2.anchor.data_ptr()
    step_fn = make_step_fn(m, opt2)
    for it in range(6):
        if it == 3:
            keep = opt2.anchor.clone()
            opt2.reset_state()
            assert opt2.anchor.data_ptr() == ptr and torch.equal(opt2.anchor, m.arena.master)
            opt2.anchor.copy_(keep)  # (the stale anchor)
        step_fn(*_batch(16, 128, seed=seeds[it]))
    torch.cuda.synchronize()
    assert not torch.equal(m.arena.master, eager[1])


# ---------------------------------------------------------------- launcher refusals
def test_launchers_refuse_a_term_without_a_matching_anchor():
    n = 1024
    p0 = torch.randn(n, device=DEV)
    s = _state(p0)
    g = torch.randn(n, device=DEV)
    step = torch.ones(1, dtype=torch.int32, device=DEV)
    ever = torch.ones(16, dtype=torch.uint8, device=DEV)
    anc = p0.clone()
    bad = [(MU, None), (MU, anc[:n - 4]), (MU, anc.to(torch.bfloat16)), (MU, anc.cpu()), (-0.1, anc),
           (float("nan"), anc), (0.0, anc[:n - 4])]
    for prox in bad:
        with pytest.raises(RuntimeError):
            K.adam(s[0], g, s[1], s[2], s[3], step, LR, B1, B2, EPS, 0.0, False, prox=prox)
        with pytest.raises(RuntimeError):
            K.adam_rows(s[0], g, s[1], s[2], s[3], step, LR, B1, B2, EPS, ever, None, 64, prox=prox)
    # a decaying table whose rows may be skipped takes no term
    with pytest.raises(RuntimeError):
        K.adam_rows(s[0], g, s[1], s[2], s[3], step, LR, B1, B2, EPS, ever, None, 64, WD, True, prox=(MU, anc))
    with pytest.raises(RuntimeError):
        K.adam(s[0], g, s[1], s[2], s[3], step, LR, B1, B2, EPS, WD, True, ever, None, 0, 16, 64, prox=(MU, anc))
    # the all-layer launch: no anchors, a short one, a term without the fused Adam
    T, M, N = 128, 256, 256
    dy = torch.randn(T, M, device=DEV).to(torch.bfloat16)
    x = torch.randn(T, N, device=DEV).to(torch.bfloat16)
    out = torch.full((M, N), 7.0, device=DEV)
    w = _state(torch.randn(M * N, device=DEV))
    w0 = [t.clone() for t in w]
    st, hp = [w[0], w[1], w[2], w[3], step], [LR, B1, B2, EPS, 0.0, 0.0]
    wanc = w[0].clone()
    ext = K.ext()
    with pytest.raises(RuntimeError):
        ext.gemm_dw_batch([dy], [x], [out], [0], st, hp, -1, prox_mu=MU)
    with pytest.raises(RuntimeError):
        ext.gemm_dw_batch([dy], [x], [out], [0], st, hp, -1, prox_mu=MU, anchor=[wanc[:M * N - 4]])
    with pytest.raises(RuntimeError):
        ext.gemm_dw_batch([dy], [x], [out], [0], st, hp, -1, prox_mu=MU, anchor=[wanc, wanc])
    with pytest.raises(RuntimeError):
        ext.gemm_dw_batch([dy], [x], [out], [0], [], [], -1, prox_mu=MU, anchor=[wanc])
    with pytest.raises(RuntimeError):
        ext.gemm_dw_batch([dy], [x], [out], [0], st, hp, -1, prox_mu=-1.0, anchor=[wanc])
    # the per-layer fused launches refuse the term as they refuse a schedule
    hpx = type("HP", (list,), {"prox": (MU, wanc), "sched": None})(hp)
    with pytest.raises(ValueError, match="proximal"):
        K.linear_dw(dy, x, out, adam=(st, hpx))
    with pytest.raises(ValueError, match="proximal"):
        K.linear_dw2(dy, x, out, dy, x, out, adam=(st + st, hpx))
    torch.cuda.synchronize()
    # nothing was launched
    assert (out == 7.0).all()
    for a, b in zip(s, _state(p0)):
        assert torch.equal(a, b)
    for a, b in zip(w, w0):
        assert torch.equal(a, b)
