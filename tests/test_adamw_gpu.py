"""AdamW on the GPU: per-run weight decay in the run-table Adam, the lazy decoupled decay of
word-embedding rows without Adam state (kernel level and through a training run), and the
parameter groups in the fused weight-gradient epilogues.

Everything is compared bit for bit against the plain launches it replaces: one launch per run with
that run's scalar decay, and the dense table update with the same decay."""
import numpy as np
import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.data import (
    CICIDS2017Dataset, DeviceLoader)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn, train_model)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier, DistilBertConfig)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
HF_NO_DECAY = ("bias", "LayerNorm", "layer_norm")


@pytest.fixture
def nosplit():
    """Weight-gradient GEMMs unsplit in every arm (as tests/test_fused_adam_gpu.py)."""
    K.ext().gemm_set_cfg(2, -1, 1)
    yield
    K.ext().gemm_set_cfg(2, -1, -1)


# ---------------------------------------------------------------- run table with per-run decay
@pytest.mark.parametrize("decoupled", [False, True])
def test_run_table_per_run_decay(decoupled):
    """One run-table launch with a decay per run == one launch per run with that run's scalar
    decay, bitwise (p, m, v, shadow; 3 steps), and the per-run arm agrees with fp32 torch
    Adam / AdamW with two parameter groups within the bound of
    tests/test_kernels_gpu.py::test_adam_matches_torch (max |diff| < 1e-6)."""
    runs = [(0, 64), (128, 8), (256, 260), (1024, 1024)]
    decays = [0.01, 0.0, 0.01, 0.0]
    n = 2048 + 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    p0 = torch.randn(n, device=DEV, generator=gen)
    a = [p0.clone(), None, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [p0.clone(), None, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    sha, shb = p0.to(torch.bfloat16), p0.to(torch.bfloat16)
    refs = [p0[o:o + ln].clone().requires_grad_(True) for o, ln in runs]
    groups = [{"params": [r], "weight_decay": wd} for r, wd in zip(refs, decays)]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=LR, betas=(B1, B2), eps=EPS)
    table, rdec = K.adam_runs(runs, DEV), K.adam_run_decay(decays, DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(3):
        g = torch.randn(n, device=DEV, generator=gen)
        K.step_inc(step, None)
        # (the scalar 0.5 must be ignored when a decay per run is given)
        K.adam(a[0], g, a[2], a[3], sha, step, LR, B1, B2, EPS, 0.5, decoupled, runs=table, run_decay=rdec)
        for (o, ln), wd in zip(runs, decays):
            sl = slice(o, o + ln)
            K.adam(b[0][sl], g[sl], b[2][sl], b[3][sl], shb[sl], step, LR, B1, B2, EPS, wd, decoupled)
        for r, (o, ln) in zip(refs, runs):
            r.grad = g[o:o + ln].clone()
        opt.step()
    torch.cuda.synchronize()
    for x, y in zip([a[0], a[2], a[3], sha], [b[0], b[2], b[3], shb]):
        assert torch.equal(x, y)
    untouched = torch.ones(n, dtype=torch.bool, device=DEV)
    for (o, ln), r in zip(runs, refs):
        untouched[o:o + ln] = False
        err = (b[0][o:o + ln] - r.detach()).abs().max().item()
        print(f"decoupled={decoupled} run ({o}, {ln}): max |hip - torch| = {err:.3e}")
        assert err < 1e-6
    assert torch.equal(a[0][untouched], p0[untouched])
    # the decay is really per run: the decayed runs differ from a launch without decay
    # (moments from the run above: a first Adam step is lr * sign(g) whatever L2 decay adds to g)
    c = [p0.clone(), b[2].clone(), b[3].clone()]
    st1 = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    g = torch.randn(n, device=DEV, generator=gen)
    d = [t.clone() for t in c]
    K.adam(c[0], g, c[1], c[2], None, st1, LR, B1, B2, EPS, 0.0, decoupled, runs=table)
    K.adam(d[0], g, d[1], d[2], None, st1, LR, B1, B2, EPS, 0.0, decoupled, runs=table, run_decay=rdec)
    for (o, ln), wd in zip(runs, decays):
        assert torch.equal(c[0][o:o + ln], d[0][o:o + ln]) == (wd == 0.0)


# ---------------------------------------------------------------- lazy rows, kernel level
PAD, TAIL = 64, 256
SCHEDULE = {1: [3, 4, 17, 17], 3: [5, 249], 5: [3, 100]}


def _table_arena(rows, rl, seed):
    n = PAD + rows * rl + TAIL
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(n, device=DEV, generator=gen)
    return n, gen, p


@pytest.mark.parametrize("rl", [768, 64])
def test_lazy_row_decay_matches_dense_table(rl):
    """A [250][rl] table behind a 64-float pad, followed by one dense run.  Rows are first touched
    at steps 1 (with a duplicate id), 3 and 5 of 6.  The lazy arm (catch-up launch on the batch's
    ids, row-flag Adam with the real decay, run table for the rest) is bitwise the dense arm (one
    flat launch over everything, same decay): the batch's rows after each catch-up (master and
    shadow), and after the final flush the whole arena, m and v."""
    rows = 250
    n, gen, p0 = _table_arena(rows, rl, 11)
    t0, t1 = PAD, PAD + rows * rl
    tab = slice(t0, t1)
    dense = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(torch.bfloat16)]
    lazy = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(torch.bfloat16)]
    ever = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    done = torch.zeros(rows, dtype=torch.int32, device=DEV)
    sd = torch.zeros(1, dtype=torch.int32, device=DEV)
    sl = torch.zeros(1, dtype=torch.int32, device=DEV)
    rest = K.adam_runs([(0, PAD), (t1, TAIL)], DEV)

    def rows_of(buf, ids):
        return buf[tab].view(rows, rl)[sorted(set(ids))]

    for t in range(1, 7):
        ids = SCHEDULE.get(t, [])
        if ids:
            idt = torch.tensor(ids, dtype=torch.int64, device=DEV)
            K.adam_lazy_decay(lazy[0][tab], lazy[3][tab], done, ever, sl, 0, LR, WD, rl, idt)
            torch.cuda.synchronize()
            assert torch.equal(rows_of(lazy[0], ids), rows_of(dense[0], ids)), t
            assert torch.equal(rows_of(lazy[3], ids), rows_of(dense[3], ids)), t
        g = torch.randn(n, device=DEV, generator=gen)
        now = torch.zeros(rows, dtype=torch.uint8, device=DEV)
        if ids:
            now[torch.tensor(sorted(set(ids)), device=DEV)] = 1
        ever |= now
        gd = g.clone()
        gd[tab] = (g[tab].view(rows, rl) * now[:, None].float()).reshape(-1)
        K.step_inc(sd, None)
        K.adam(dense[0], gd, dense[1], dense[2], dense[3], sd, LR, B1, B2, EPS, WD, True)
        K.step_inc(sl, None)
        K.adam_rows(lazy[0][tab], g[tab], lazy[1][tab], lazy[2][tab], lazy[3][tab], sl, LR, B1, B2, EPS, ever, now,
                    rl, WD, True)
        K.adam(lazy[0], g, lazy[1], lazy[2], lazy[3], sl, LR, B1, B2, EPS, WD, True, runs=rest)
    torch.cuda.synchronize()
    never = ever == 0
    assert int(never.sum()) == rows - 6
    # rows without state are behind until the flush ...
    assert not torch.equal(lazy[0][tab].view(rows, rl)[never], dense[0][tab].view(rows, rl)[never])
    for _ in range(2):  # ... which is idempotent
        K.adam_lazy_decay(lazy[0][tab], lazy[3][tab], done, ever, sl, 0, LR, WD, rl, None)
        torch.cuda.synchronize()
        for x, y in zip(lazy, dense):
            assert torch.equal(x, y)
    assert torch.equal(done[never], torch.full_like(done[never], 6))


def test_lazy_flush_of_300_steps():
    """300 completed steps owed at once: one flush == 300 dense launches ([250][64] table)."""
    rows, rl = 250, 64
    n = rows * rl
    gen = torch.Generator(device=DEV).manual_seed(12)
    p0 = torch.randn(n, device=DEV, generator=gen)
    dense = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(torch.bfloat16)]
    zero = torch.zeros(n, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(300):
        K.step_inc(step, None)
        K.adam(dense[0], zero, dense[1], dense[2], dense[3], step, LR, B1, B2, EPS, WD, True)
    p, sh = p0.clone(), p0.to(torch.bfloat16)
    ever = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    ever[7] = 1  # a row with Adam state is not the flush's business
    done = torch.zeros(rows, dtype=torch.int32, device=DEV)
    K.adam_lazy_decay(p, sh, done, ever, step, 0, LR, WD, rl, None)
    torch.cuda.synchronize()
    assert int(step) == 300
    keep = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep[7] = False
    assert torch.equal(p.view(rows, rl)[keep], dense[0].view(rows, rl)[keep])
    assert torch.equal(sh.view(rows, rl)[keep], dense[3].view(rows, rl)[keep])
    assert torch.equal(p.view(rows, rl)[7], p0.view(rows, rl)[7])
    assert not dense[1].any() and not dense[2].any()
    assert not torch.equal(p, p0)


# ---------------------------------------------------------------- lazy rows, model level
QKV_BIASES = [f"distilbert.transformer.layer.{i}.attention.{n}_lin.bias" for i in range(2) for n in "qkv"]


def _batch(B, S, seed, lo=None, hi=None):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(S // 3 if lo is None else lo, S + 1 if hi is None else hi + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = ids * mask
    ids[:, 0] = 101
    labels = torch.randint(0, 2, (B,), generator=g)
    return ids.cuda(), mask.cuda(), labels.cuda(), int(lens.sum())


def _model(seed=21):
    m = DDoSClassifier(config=DistilBertConfig(n_layers=2), device=DEV, impl="hip", seed=seed)
    for name in QKV_BIASES:  # (zero-initialised: give the decay something to show on)
        m.arena.view(name).fill_(0.25)
    m.sync_shadow(force=True)
    m.train()
    return m


def _arm(lazy, graph, weight_decay=WD):
    m = _model()
    opt = ArenaAdam(m, lr=LR, weight_decay=weight_decay, decoupled=True, no_decay=HF_NO_DECAY, fuse_dw=lazy)
    if not lazy:
        m.sparse_word_grad = False
        m._hip_cache = None
    assert opt.can_fuse() == lazy and opt.lazy_active() == (lazy and weight_decay != 0.0)
    return m, opt, GraphedTrainStep(make_step_fn(m, opt), warmup=1, enabled=graph, bucket=m.packed_rows)


def test_lazy_adamw_training_matches_dense(nosplit, monkeypatch):
    """AdamW 0.01 with the HF no-decay group, 5 steps of a 2-layer model (B alternating 4 and 3, so
    two graphs replay): {graph, eager} x {lazy sparse word rows + fused dW epilogues + the rest of
    the step in the dW launch, dense word table + unfused} give bitwise equal losses and
    ``state_dict()``s.  The qkv biases -- updated by the dW tiles in the fused arm -- take no
    decay: after the first step they equal a weight_decay = 0 run's, the matrices do not."""
    rest_seen = []
    real_rest = ArenaAdam.rest_args

    def spy(self):
        r = real_rest(self)
        rest_seen.append((self.fuse_dw, r is not None))
        return r

    monkeypatch.setattr(ArenaAdam, "rest_args", spy)
    arms = [_arm(lazy, graph) for lazy in (True, False) for graph in (True, False)]
    plain = _arm(True, False, weight_decay=0.0)
    # B = 4 with 160..192 real tokens (192 packed rows), B = 3 with 102..126 (128 packed rows): one
    # graph each -- step 1 runs eagerly, 2 and 3 capture, 4 and 5 replay
    batches = [_batch(4, 64, 500 + it, 40, 48) if it % 2 == 0 else _batch(3, 64, 500 + it, 34, 42) for it in range(5)]
    losses = [[] for _ in arms]
    first = None
    for it, (ids, mask, labels, tokens) in enumerate(batches):
        for i, (_, _, st) in enumerate(arms):
            losses[i].append(float(st(ids, mask, labels, tokens)))
        if it == 0:
            plain[2](ids, mask, labels, tokens)
            first = ({k: v.clone() for k, v in arms[1][0].state_dict().items()},
                     {k: v.clone() for k, v in plain[0].state_dict().items()})
    torch.cuda.synchronize()
    assert all(x == losses[0] for x in losses[1:]), losses
    sds = [m.state_dict() for m, _, _ in arms]
    for sd in sds[1:]:
        assert list(sd) == list(sds[0])
        for k in sd:
            assert torch.equal(sd[k], sds[0][k]), k
    for (m, opt, st), (_, o0, _) in zip(arms[1:], arms[:1] * 3):
        assert torch.equal(opt.m, o0.m) and torch.equal(opt.v, o0.v)
        assert torch.equal(m.arena.shadow, arms[0][0].arena.shadow)
    for m, opt, st in arms[:2]:
        assert m.sparse_word_grad and opt.lazy_active()
    assert arms[0][2].graph is not None and arms[0][2].failed is None and len(arms[0][2].graphs) == 2
    assert arms[2][2].graph is not None and arms[2][2].failed is None
    # the lazy arms ran the rest of the step inside the dW launch, the unfused arms never asked
    assert rest_seen and all(ok for fused, ok in rest_seen if fused)
    assert any(fused for fused, _ in rest_seen)
    # untouched word rows really were decayed (5 steps), and the table was not walked densely
    word = "distilbert.embeddings.word_embeddings.weight"
    init = _model().state_dict()[word]
    row = sds[0][word][5000]
    assert not torch.equal(row, init[5000])
    want = init[5000].clone()
    for _ in range(5):
        want *= torch.tensor(1.0, device=DEV) - torch.tensor(LR, device=DEV) * torch.tensor(WD, device=DEV)
    assert torch.equal(row, want)
    assert int(arms[0][0].emb_ever.sum()) < 1000
    # first step: the no-decay parameters took exactly the weight_decay = 0 step
    fused1, plain1 = first
    for k in fused1:
        same = torch.equal(fused1[k], plain1[k])
        if any(s in k for s in HF_NO_DECAY):
            assert same, k
        else:
            assert not same, k
    assert all(k in fused1 for k in QKV_BIASES)


def test_eval_right_after_train_model_needs_no_flush(nosplit):
    """``train_model`` settles the lazy decay before it returns: an evaluation right after it --
    on ids the training never touched -- gives the dense arm's logits, bitwise."""
    n, S = 16, 64
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(1000, 2000, (n, S), generator=g)
    ids[:, 0] = 101
    lens = torch.randint(S // 3, S + 1, (n,), generator=g)
    ids = ids * (torch.arange(S)[None] < lens[:, None]).long()
    labels = torch.randint(0, 2, (n,), generator=g)
    ds = CICIDS2017Dataset([""] * n, labels.tolist(), ids=ids.numpy(), lengths=lens.numpy().astype(np.int64),
                           max_len=S)
    e_ids = torch.randint(3000, 4000, (4, S), generator=g)  # rows without Adam state
    e_ids[:, 0] = 101
    e_mask = torch.ones(4, S, dtype=torch.long)
    outs = []
    for lazy in (True, False):
        m, opt, _ = _arm(lazy, True)
        seen = []
        train_model(m, DeviceLoader(ds, 4, device=torch.device(DEV)), None, opt, num_epochs=1,
                    on_epoch=lambda e, avg, m=m, s=seen: s.append(m.arena.master.clone()))
        assert torch.equal(seen[0], m.arena.master)  # (flushed before the callback already)
        m.eval()
        with torch.no_grad():
            outs.append((m(e_ids.cuda(), e_mask.cuda()).clone(), m.arena.master.clone(), m.arena.shadow.clone()))
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert torch.equal(x, y)
