"""Learning-rate schedules on the GPU: the device function's own table against the fp64 reference,
and every Adam launch under a schedule against the same launch fed the table's value as a plain
rate -- bit for bit (the constant-rate launches are pinned to torch by tests/test_kernels_gpu.py,
tests/test_adamw_gpu.py and tests/test_fused_adam_gpu.py).  Then the lazy word-row decay with a
moving rate, a training run whose graph replays honour the schedule, and the federated runner's
one-ramp-per-run scope."""
import os

import pytest
import torch

from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd import data
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.config import FedConfig
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.engine import (
    ArenaAdam, GraphedTrainStep, make_step_fn, train_model)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.fed import runner
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.models import (
    DDoSClassifier, DistilBertConfig)
from detecting_cyber_attacks_with_distilled_large_language_models_in_distributed_networks_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
HF_NO_DECAY = ("bias", "LayerNorm", "layer_norm")
BASE_RATES = (2e-5, 3e-4, 1e-3)
GRID = ((0, 7), (3, 10), (1, 2), (5, 5), (4, 6), (100, 1272), (127, 3816))
# three fp32 roundings (the base rate, the divide, the multiply), each <= 2^-24, plus one to spare
REL_BOUND = 4 * 2.0 ** -24
LINEAR, WARM = K.LR_SCHEDULES["linear"], K.LR_SCHEDULES["constant_with_warmup"]


@pytest.fixture
def nosplit():
    """Weight-gradient GEMMs unsplit in every arm (as tests/test_adamw_gpu.py)."""
    K.ext().gemm_set_cfg(2, -1, 1)
    yield
    K.ext().gemm_set_cfg(2, -1, -1)


def _reference(kind, base, w, T, n):
    """fp64: the base rate times HF's lambda of c = step - 1."""
    out = []
    for c in range(n):
        if c < w:
            f = c / max(1, w)
        elif kind == LINEAR:
            f = max(0, (T - c) / max(1, T - w))
        else:
            f = 1.0
        out.append(base * f)
    return out


# ---------------------------------------------------------------- the device's own numbers
def test_device_table_matches_reference():
    host = ArenaAdam(DDoSClassifier(config=DistilBertConfig(n_layers=1), seed=0), schedule="linear", total_steps=7)
    differ = entries = 0
    worst = 0.0
    for kind, name in ((LINEAR, "linear"), (WARM, "constant_with_warmup")):
        host.schedule = name
        for base in BASE_RATES:
            host.lr = base
            for w, T in GRID:
                got = K.lr_schedule_table(base, (kind, w, T, 0), T + 2).cpu().tolist()
                ref = _reference(kind, base, w, T, T + 2)
                host.set_schedule(total_steps=T, warmup_steps=w)
                for t, (g, r) in enumerate(zip(got, ref), start=1):
                    if r == 0.0:
                        assert g == 0.0, (name, base, w, T, t, g)
                    else:
                        rel = abs(g - r) / abs(r)
                        worst = max(worst, rel)
                        assert rel <= REL_BOUND, (name, base, w, T, t, g, r, rel)
                    differ += g != host.lr_at(t)
                    entries += 1
    print(f"device table: {entries} entries, worst relative error {worst:.3e} (bound {REL_BOUND:.3e}); "
          f"{differ} differ from the host mirror lr_at")
    # the offset shifts the ramp; the constant kind hands the rate back untouched
    full = K.lr_schedule_table(LR, (LINEAR, 3, 10, 0), 10)
    assert torch.equal(K.lr_schedule_table(LR, (LINEAR, 3, 10, 4), 6), full[4:])
    assert torch.equal(K.lr_schedule_table(LR, (0, 3, 10, 0), 4), torch.full((4,), LR, device=DEV))
    with pytest.raises(RuntimeError, match="kind"):
        K.lr_schedule_table(LR, (3, 0, 10, 0), 4)
    with pytest.raises(RuntimeError, match="warmup"):
        K.lr_schedule_table(LR, (LINEAR, 11, 10, 0), 4)


# ---------------------------------------------------------------- flat / run-table / row launches
SCHED = (LINEAR, 2, 6, 0)


@pytest.fixture(scope="module")
def table6():
    """The device's rates of steps 1..6 under SCHED with base LR (fed back as plain rates)."""
    t = K.lr_schedule_table(LR, SCHED, 6)
    vals = [float(x) for x in t.cpu()]
    assert vals[0] == 0.0 and vals[2] == float(torch.tensor(LR, dtype=torch.float32)) and len(set(vals)) == 5
    return vals


@pytest.mark.parametrize("decoupled", [False, True])
def test_scheduled_adam_equals_per_step_rate(table6, decoupled):
    """sched= with the base rate == no schedule and lr = table[step - 1], bitwise after every step:
    the run table with a decay per run (the runs of test_run_table_per_run_decay) and the flat launch."""
    runs = [(0, 64), (128, 8), (256, 260), (1024, 1024)]
    decays = [0.01, 0.0, 0.01, 0.0]
    n = 2048 + 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    p0 = torch.randn(n, device=DEV, generator=gen)
    table, rdec = K.adam_runs(runs, DEV), K.adam_run_decay(decays, DEV)

    def state():
        return [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(torch.bfloat16)]

    ra, rb, fa, fb = state(), state(), state(), state()
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for t in range(1, 7):
        g = torch.randn(n, device=DEV, generator=gen)
        K.step_inc(step, None)
        K.adam(ra[0], g, ra[1], ra[2], ra[3], step, LR, B1, B2, EPS, 0.5, decoupled, runs=table, run_decay=rdec,
               sched=SCHED)
        K.adam(rb[0], g, rb[1], rb[2], rb[3], step, table6[t - 1], B1, B2, EPS, 0.5, decoupled, runs=table,
               run_decay=rdec)
        K.adam(fa[0], g, fa[1], fa[2], fa[3], step, LR, B1, B2, EPS, WD, decoupled, sched=SCHED)
        K.adam(fb[0], g, fb[1], fb[2], fb[3], step, table6[t - 1], B1, B2, EPS, WD, decoupled)
        torch.cuda.synchronize()
        for x, y in zip(ra + fa, rb + fb):
            assert torch.equal(x, y), t
        if t == 1:  # the first step of the warmup runs at 0: moments move, parameters do not
            assert torch.equal(fa[0], p0) and fa[1].any() and fa[2].any()
    assert not torch.equal(fa[0], p0)


@pytest.mark.parametrize("rl", [768, 64])
def test_scheduled_adam_rows_equals_per_step_rate(table6, rl):
    rows = 250
    n = rows * rl
    gen = torch.Generator(device=DEV).manual_seed(6)
    p0 = torch.randn(n, device=DEV, generator=gen)
    a = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(torch.bfloat16)]
    b = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(torch.bfloat16)]
    ever = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    flagged = {1: [3, 4, 17], 2: [249], 4: [3, 100]}
    for t in range(1, 7):
        g = torch.randn(n, device=DEV, generator=gen)
        now = torch.zeros(rows, dtype=torch.uint8, device=DEV)
        if t in flagged:
            now[torch.tensor(flagged[t], device=DEV)] = 1
        ever |= now
        K.step_inc(step, None)
        K.adam_rows(a[0], g, a[1], a[2], a[3], step, LR, B1, B2, EPS, ever, now, rl, WD, True, sched=SCHED)
        K.adam_rows(b[0], g, b[1], b[2], b[3], step, table6[t - 1], B1, B2, EPS, ever, now, rl, WD, True)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y), t
    touched = ever.bool()
    assert int(touched.sum()) == 5
    assert not torch.equal(a[0].view(rows, rl)[touched], p0.view(rows, rl)[touched])
    assert torch.equal(a[0].view(rows, rl)[~touched], p0.view(rows, rl)[~touched])


# ---------------------------------------------------------------- lazy rows with a moving rate
PAD, TAIL = 64, 256
TOUCHES = {1: [3, 4, 17, 17], 3: [5, 249], 5: [3, 100]}


@pytest.mark.parametrize("rl", [768, 64])
def test_lazy_row_decay_follows_the_schedule(table6, rl):
    """The kernel-level setup of tests/test_adamw_gpu.py::test_lazy_row_decay_matches_dense_table
    with every launch scheduled: the lazy arm is bitwise the dense arm -- the batch's rows after
    each catch-up, the whole arena, m and v after the flush -- because each missed step's
    multiplication takes that step's rate, in step order."""
    rows = 250
    n = PAD + rows * rl + TAIL
    gen = torch.Generator(device=DEV).manual_seed(11)
    p0 = torch.randn(n, device=DEV, generator=gen)
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
        ids = TOUCHES.get(t, [])
        if ids:
            idt = torch.tensor(ids, dtype=torch.int64, device=DEV)
            K.adam_lazy_decay(lazy[0][tab], lazy[3][tab], done, ever, sl, 0, LR, WD, rl, idt, sched=SCHED)
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
        K.adam(dense[0], gd, dense[1], dense[2], dense[3], sd, LR, B1, B2, EPS, WD, True, sched=SCHED)
        K.step_inc(sl, None)
        K.adam_rows(lazy[0][tab], g[tab], lazy[1][tab], lazy[2][tab], lazy[3][tab], sl, LR, B1, B2, EPS, ever, now,
                    rl, WD, True, sched=SCHED)
        K.adam(lazy[0], g, lazy[1], lazy[2], lazy[3], sl, LR, B1, B2, EPS, WD, True, runs=rest, sched=SCHED)
    torch.cuda.synchronize()
    never = ever == 0
    assert int(never.sum()) == rows - 6
    assert not torch.equal(lazy[0][tab].view(rows, rl)[never], dense[0][tab].view(rows, rl)[never])
    for _ in range(2):  # the flush, idempotent
        K.adam_lazy_decay(lazy[0][tab], lazy[3][tab], done, ever, sl, 0, LR, WD, rl, None, sched=SCHED)
        torch.cuda.synchronize()
        for x, y in zip(lazy, dense):
            assert torch.equal(x, y)
    # a row never touched: the initial row times the six factors 1 - table[s] * wd, in order, in fp32
    row = int(torch.nonzero(never)[0])
    want = p0[tab].view(rows, rl)[row].clone()
    wd32 = torch.tensor(WD, dtype=torch.float32, device=DEV)
    for s in range(6):
        want *= torch.tensor(1.0, device=DEV) - torch.tensor(table6[s], dtype=torch.float32, device=DEV) * wd32
    assert torch.equal(lazy[0][tab].view(rows, rl)[row], want)
    # ... which a constant rate does not give
    const = p0[tab].clone()
    K.adam_lazy_decay(const, None, torch.zeros_like(done), torch.zeros_like(ever), sl, 0, LR, WD, rl, None)
    torch.cuda.synchronize()
    assert not torch.equal(const.view(rows, rl)[row], want)


# ---------------------------------------------------------------- model level: graph replays
QKV_BIASES = [f"distilbert.transformer.layer.{i}.attention.{n}_lin.bias" for i in range(2) for n in "qkv"]
SCHED5 = dict(schedule="linear", warmup_steps=2, total_steps=5)


def _batch(B, S, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(lo, hi + 1, (B,), generator=g)
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


def _arm(lazy, graph, **sched):
    m = _model()
    opt = ArenaAdam(m, lr=LR, weight_decay=WD, decoupled=True, no_decay=HF_NO_DECAY, fuse_dw=lazy, **sched)
    if not lazy:
        m.sparse_word_grad = False
        m._hip_cache = None
    assert opt.can_fuse() == lazy and opt.lazy_active() == lazy
    return m, opt, GraphedTrainStep(make_step_fn(m, opt), warmup=1, enabled=graph, bucket=m.packed_rows)


def test_training_graph_replays_honour_the_schedule(nosplit):
    """AdamW 0.01 with the HF no-decay group under linear (2, 5), 5 steps of a 2-layer model (B
    alternating 4 and 3: two graphs capture and replay; the batches of
    tests/test_adamw_gpu.py::test_lazy_adamw_training_matches_dense).  {graph, eager} x {fused dW
    epilogues + lazy sparse word rows + the rest of the step in the dW launch, unfused + dense word
    table}, and an eager unfused arm with a constant schedule whose rate the test sets to the device
    table's value before each step: bitwise equal losses, state_dict()s, m, v and shadow."""
    table = [float(x) for x in K.lr_schedule_table(LR, (LINEAR, 2, 5, 0), 5).cpu()]
    arms = [_arm(lazy, graph, **SCHED5) for lazy in (True, False) for graph in (True, False)]
    arms.append(_arm(False, False))
    const = _arm(True, False)
    batches = [_batch(4, 64, 500 + it, 40, 48) if it % 2 == 0 else _batch(3, 64, 500 + it, 34, 42) for it in range(5)]
    losses = [[] for _ in arms]
    for it, (ids, mask, labels, tokens) in enumerate(batches):
        arms[4][1].lr = table[it]
        for i, (_, _, st) in enumerate(arms):
            losses[i].append(float(st(ids, mask, labels, tokens)))
        const[2](ids, mask, labels, tokens)
    torch.cuda.synchronize()
    assert all(x == losses[0] for x in losses[1:]), losses
    sds = [m.state_dict() for m, _, _ in arms]
    for sd in sds[1:]:
        assert list(sd) == list(sds[0])
        for k in sd:
            assert torch.equal(sd[k], sds[0][k]), k
    for m, opt, _ in arms[1:]:
        assert torch.equal(opt.m, arms[0][1].m) and torch.equal(opt.v, arms[0][1].v)
        assert torch.equal(m.arena.shadow, arms[0][0].arena.shadow)
    # both graphed arms really captured: one graph per packed-row bucket in the fused arm
    assert arms[0][2].graph is not None and arms[0][2].failed is None and len(arms[0][2].graphs) == 2
    assert arms[2][2].graph is not None and arms[2][2].failed is None
    for m, opt, _ in arms[:2]:
        assert m.sparse_word_grad and opt.lazy_active()
    # the schedule shows: a constant-rate run ends elsewhere
    csd = const[0].state_dict()
    assert any(not torch.equal(csd[k], sds[0][k]) for k in csd)
    # an untouched word row took the five scheduled decay factors, in order
    word = "distilbert.embeddings.word_embeddings.weight"
    want = _model().state_dict()[word][5000].clone()
    for s in range(5):
        want *= torch.tensor(1.0, device=DEV) - torch.tensor(table[s], dtype=torch.float32, device=DEV) * \
            torch.tensor(WD, dtype=torch.float32, device=DEV)
    assert torch.equal(sds[0][word][5000], want)
    # a sixth step, past total, replays at rate 0: every master parameter stays put
    m, opt, st = arms[0]
    opt.finish()
    before, m_before = m.arena.master.clone(), opt.m.clone()
    st(*batches[0])
    opt.finish()
    torch.cuda.synchronize()
    assert len(st.graphs) == 2 and st.failed is None
    assert torch.equal(m.arena.master, before)
    assert not torch.equal(opt.m, m_before)


# ---------------------------------------------------------------- scope "run" across two rounds
def test_scope_run_spans_two_virtual_rounds(tmp_path, nosplit):
    """``run_virtual_clients`` (1 client, 2 rounds, scope "run"): round 2 continues the ramp at
    step_offset = steps_per_round.  Equal, bit for bit, to a hand-driven loop over the same loader
    that calls ``reset_state()`` and sets the offset itself."""
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    cfg = FedConfig(out_dir=str(tmp_path), synthetic_rows=1000, data_fraction=0.1, max_len=64, epochs=1,
                    batch_size=8, eval_batch_size=32, plots=False, resume=False, rounds=2, verbose=False,
                    heartbeat_s=0.0, save_checkpoints=False, lr=LR, weight_decay=WD, decoupled_weight_decay=True,
                    no_decay=",".join(HF_NO_DECAY), lr_schedule="linear", warmup_steps=2, lr_schedule_scope="run")
    frame = data.generate_cicids2017(cfg.synthetic_rows, seed=0)

    def client():
        return runner.FederatedClient(cfg, frame=frame, model_config=DistilBertConfig(n_layers=1)).setup()

    c = client()
    assert c.model.device.type == "cuda" and c.model.impl == "hip"
    res = runner.run_virtual_clients(c, 1, rounds=2)
    spr = res["rounds"][0]["clients"][0]["train"]["steps"]
    assert spr >= 3 and res["rounds"][1]["clients"][0]["train"]["steps"] == spr
    assert all(r["clients"][0]["train"]["graph"] for r in res["rounds"])

    h = client()
    model = h.model
    d = data.build_client_data(frame, 0, cfg.data_fraction, cfg.base_seed, cfg.max_len, h.tokenizer, cfg.partition, 1)
    loader = data.DeviceLoader(d.train, cfg.batch_size, shuffle=True, device=model.device, seed=cfg.client_seed(0))
    assert cfg.epochs * len(loader) == spr
    opt = ArenaAdam(model, lr=LR, weight_decay=WD, decoupled=True, no_decay=HF_NO_DECAY, schedule="linear",
                    warmup_steps=2, total_steps=2 * spr)
    for r in range(2):
        opt.reset_state()
        opt.set_schedule(step_offset=r * spr)
        train_model(model, loader, None, opt, cfg.epochs)
    torch.cuda.synchronize()
    assert torch.equal(model.arena.master, c.model.arena.master)
    # scope "round" restarts the ramp instead: a different end point
    cfg.lr_schedule_scope = "round"
    c2 = client()
    runner.run_virtual_clients(c2, 1, rounds=2)
    assert not torch.equal(c2.model.arena.master, c.model.arena.master)
